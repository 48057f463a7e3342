"""GPU: the acceleration-relative opening criterion of the convergent Barnes-Hut force (NB_FLAG_TREE_RELATIVE, nb_tree_alpha)
against its numpy statement (tests/tree_rel_model.py) — bit for bit with the Quake rsqrt, within the fast tree mode's bar with the
hardware rsqrt — against the handle without the flag where the test is off, across a restart, and composed with the tree energy."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tree_energy_model as tem  # noqa: E402
import tree_leaves_model as tlm  # noqa: E402
import tree_model as tm  # noqa: E402
import tree_quad_model as tqm  # noqa: E402
import tree_rel_model as trm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
# 333 = 5 * 64 + 13: more than one window, a ragged last one, and one position that two bodies share
FIXTURES = {"random_333": ("ic_random_333.npy", 0.5), "plummer_1024": ("ic_plummer_1024.npy", 0.05), "plummer_4096": ("ic_plummer_4096.npy", 0.05)}
THETAS = [1.0, 0.5]
ALPHAS = [0.02, 0.005]
MAX_ERR, MEDIAN_ERR = 2e-5, 2e-6          # of max |a|: the bar of the fast tree mode (tests/test_tree_quad_gpu.py)
ENERGY_BAR = 1e-10                        # tests/test_tree_energy_gpu.py
_cache = {}


def bodies_of(flat: np.ndarray) -> np.ndarray:
    b = nb.bodies_array(flat.shape[0])
    b["pos"], b["vel"], b["acc"] = flat[:, 0:2], flat[:, 2:4], flat[:, 4:6]
    b["mass"], b["radius"] = flat[:, 6], flat[:, 7]
    return b


def tree_of(key, flat):
    if (key, "tree") not in _cache:
        x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
        tree = tm.build_canonical(x, y, m)
        _cache[key, "tree"] = (x, y, m, tree, tqm.moments(tree))
    return _cache[key, "tree"]


def fixture(name, aprev="theta1"):
    """The fixture with a previous acceleration in the records' acc field: the model's theta = 1 result (per-lane walk, exact
    rsqrt), or ("wild") an arbitrary random field of that size, so that the predicate is exercised away from physical values."""
    if (name, aprev) not in _cache:
        file, eps = FIXTURES[name]
        flat = np.load(GOLD / file).astype(np.float32)
        flat[:, 7] = 0.0
        x, y, m, tree, _ = tree_of(name, flat)
        a1 = np.stack(tlm.walk(tree, x, y, m, eps, 1.0, False, None), axis=1)
        if aprev == "wild":
            rng = np.random.default_rng(23)
            a1 = (rng.normal(0, 1, a1.shape) * np.abs(a1).max() * 10.0 ** rng.uniform(-3, 1, (a1.shape[0], 1))).astype(np.float32)
        flat[:, 4:6] = a1
        _cache[name, aprev] = (flat, eps)
    return _cache[name, aprev]


def model(key, flat, eps, theta, alpha, quake, group, quad):
    """(float32 accelerations, their terms re-summed in float64) of the model for the a_prev in flat[:, 4:6]; the tree once per
    input, the terms once per (input, a_prev, theta, alpha, walk)."""
    x, y, m, tree, mom = tree_of(key, flat)
    aprev = np.ascontiguousarray(flat[:, 4:6])
    pkey = (key, aprev.tobytes(), theta, alpha, group)
    if pkey not in _cache:
        _cache[pkey] = trm.pairs_of(tree, x, y, m, aprev, eps, theta, alpha, group)[0]
    pairs = _cache[pkey]
    mo = mom if quad else None
    a = np.stack(trm.sum_terms(tree, mo, x, y, pairs, eps, quake), axis=1)
    return a, (None if quake else np.stack(trm.resum_f64(tree, mo, x, y, pairs, eps), axis=1))


def rel_sim(bodies, alpha, quad=False, **kw):
    return nb.Simulation(bodies, force="tree", tree_leaves=True, tree_quadrupole=quad, tree_alpha=alpha, device=0, **kw)


def leaves_sim(bodies, quad=False, **kw):
    return nb.Simulation(bodies, force="tree", tree_leaves=True, tree_quadrupole=quad, device=0, **kw)


def group_of(sim):
    d = sim.describe()
    assert " leaves=1 walk=" in d, d
    walk = d.split(" walk=")[1].split()[0]
    assert walk in ("lane", "group")
    return 64 if walk == "group" else None


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    for c in range(got.shape[1]):
        g, w = np.ascontiguousarray(got[:, c], np.float32), np.ascontiguousarray(want[:, c], np.float32)
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, f"{what}: column {c} differs in {bad.size} of {g.size} bodies, first {bad[:6]} ({g[bad[:3]]} vs {w[bad[:3]]})"


def assert_within_bar(got, want, what):
    got, want = got.astype(np.float64), np.asarray(want, np.float64)
    scale = np.hypot(want[:, 0], want[:, 1]).max()
    err = np.hypot(got[:, 0] - want[:, 0], got[:, 1] - want[:, 1]) / scale
    print(f"{what}: max {err.max():.3g} median {np.median(err):.3g} of max |a|")
    assert err.max() <= MAX_ERR and np.median(err) <= MEDIAN_ERR, what


CASES = [(n, "theta1") for n in FIXTURES] + [("plummer_1024", "wild")]


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("name,aprev", CASES)
def test_quake_mode_equals_the_model_bit_for_bit(name, aprev, quad, theta, alpha):
    flat, eps = fixture(name, aprev)
    with rel_sim(bodies_of(flat), alpha, quad, eps=eps, theta=theta, rsqrt="quake") as sim:
        assert "leaves=1 walk=lane" in sim.describe() and sim.describe().endswith(f" alpha={alpha:g}")
        got = sim.accelerations()
    assert_bits(got, model(name, flat, eps, theta, alpha, True, None, quad)[0], f"{name} {aprev} quad {quad} theta {theta} alpha {alpha}")
    with leaves_sim(bodies_of(flat), quad, eps=eps, theta=theta, rsqrt="quake") as sim:      # (the test is there: other bits without it)
        assert not np.array_equal(sim.accelerations(), got)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("name,aprev", CASES)
def test_exact_mode_error_against_the_models_terms(name, aprev, quad, theta, alpha):
    """The walk nb_describe names takes the model's terms: against their float64 sum at most 2e-5 of max |a|, median 2e-6."""
    flat, eps = fixture(name, aprev)
    with rel_sim(bodies_of(flat), alpha, quad, eps=eps, theta=theta, rsqrt="exact") as sim:
        group = group_of(sim)
        got = sim.accelerations()
    assert_within_bar(got, model(name, flat, eps, theta, alpha, False, group, quad)[1],
                      f"{name} {aprev} quad {quad} theta {theta} alpha {alpha} group {group}")


# ---------------------------------------------------------------------------------------------------------------------
# 3: the test switched off
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rsqrt", ["quake", "exact"])
@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("name", ["random_333", "plummer_1024"])
def test_alpha_zero_and_zero_acc_are_the_handle_without_the_flag(name, quad, rsqrt):
    flat, eps = fixture(name)
    fresh = flat.copy()
    fresh[:, 4:6] = 0.0
    with leaves_sim(bodies_of(flat), quad, eps=eps, theta=0.5, rsqrt=rsqrt) as sim:
        want = sim.accelerations()
    assert want.any()
    with rel_sim(bodies_of(flat), 0.005, quad, eps=eps, theta=0.5, rsqrt=rsqrt) as sim:
        sim.set_tree_alpha(0.0)
        assert sim.describe().endswith(" alpha=0")
        assert_bits(sim.accelerations(), want, f"{name} alpha 0 through the setter")
        sim.upload(bodies_of(flat))
        sim.set_tree_alpha(0.005)
        assert not np.array_equal(sim.accelerations(), want)                   # (and back on)
    with rel_sim(bodies_of(fresh), 0.005, quad, eps=eps, theta=0.5, rsqrt=rsqrt) as sim:
        assert_bits(sim.accelerations(), want, f"{name} acc = 0 in the records")


# ---------------------------------------------------------------------------------------------------------------------
# 4: fresh initial conditions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rsqrt", ["quake", "exact"])
def test_the_second_evaluation_uses_the_first(rsqrt):
    flat, eps = fixture("plummer_1024")
    fresh = flat.copy()
    fresh[:, 4:6] = 0.0
    theta, alpha, quake = 1.0, 0.005, rsqrt == "quake"
    with leaves_sim(bodies_of(fresh), True, eps=eps, theta=theta, rsqrt=rsqrt) as sim:
        plain = sim.accelerations()
    with rel_sim(bodies_of(fresh), alpha, True, eps=eps, theta=theta, rsqrt=rsqrt) as sim:
        group = group_of(sim)
        first = sim.accelerations()
        second = sim.accelerations()
        third = sim.accelerations()
    assert_bits(first, plain, "the first evaluation is the theta walk")
    fed = fresh.copy()
    fed[:, 4:6] = first
    want = model("plummer_1024", fed, eps, theta, alpha, quake, group, True)
    fed2 = fresh.copy()
    fed2[:, 4:6] = second
    want2 = model("plummer_1024", fed2, eps, theta, alpha, quake, group, True)
    if quake:
        assert_bits(second, want[0], "the second evaluation")
        assert_bits(third, want2[0], "the third evaluation")
    else:
        assert_within_bar(second, want[1], "the second evaluation")
        assert_within_bar(third, want2[1], "the third evaluation")
    assert not np.array_equal(second, first)


# ---------------------------------------------------------------------------------------------------------------------
# 5: restart
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rsqrt", ["quake", "exact"])
def test_a_restart_from_synced_records_continues_bit_for_bit(rsqrt):
    flat, eps = fixture("plummer_1024")
    fresh = flat.copy()
    fresh[:, 4:6] = 0.0
    kw = dict(eps=eps, theta=1.0, rsqrt=rsqrt, extras=L.NB_EXTRA_VCLAMP)
    dt = 1e-3
    with rel_sim(bodies_of(fresh), 0.005, True, **kw) as sim:
        sim.advance(6, dt)
        whole = sim.sync().copy()
        assert sim.frame == 6
    with rel_sim(bodies_of(fresh), 0.005, True, **kw) as sim:
        sim.advance(3, dt)
        half = sim.sync().copy()
    assert half["acc"].any()
    with rel_sim(half, 0.005, True, first_frame=3, **kw) as sim:
        sim.advance(3, dt)
        resumed = sim.sync().copy()
        assert sim.frame == 6
    for f in ("pos", "vel", "acc"):
        assert_bits(resumed[f], whole[f], f"{f} after the restart")
    # (a_prev matters: the same restart with the acc field cleared ends elsewhere)
    lost = half.copy()
    lost["acc"] = 0.0
    with rel_sim(lost, 0.005, True, first_frame=3, **kw) as sim:
        sim.advance(3, dt)
        assert not np.array_equal(sim.sync()["vel"], whole["vel"])


# ---------------------------------------------------------------------------------------------------------------------
# 6: determinism
# ---------------------------------------------------------------------------------------------------------------------
def determinism_input():
    """As tests/test_tree_leaves_gpu.py builds it: ic_plummer_1024 with 8 bodies duplicated onto others' positions, one more pair
    made to straddle the boundary between the first two windows of 64, and three massless tracers; a_prev (the model's theta = 1
    result on this input) in the acc field."""
    if "determinism" not in _cache:
        flat = fixture("plummer_1024")[0].copy()
        rng = np.random.default_rng(17)
        pick = rng.choice(flat.shape[0], 24, replace=False)
        flat[pick[:8], 0:2] = flat[pick[8:16], 0:2]
        order = tlm.key_order(flat[:, 0], flat[:, 1], flat[:, 6])
        at63 = order[63]
        mover = [b for b in pick[16:20] if b > at63 and b not in order[56:72]][0]
        flat[mover, 0:2] = flat[at63, 0:2]
        flat[pick[20:23], 6] = 0.0
        order = tlm.key_order(flat[:, 0], flat[:, 1], flat[:, 6])
        assert order[63] == at63 and order[64] == mover             # one position on both sides of a window boundary
        x, y, m, tree, _ = tree_of("determinism", flat)
        flat[:, 4:6] = np.stack(tlm.walk(tree, x, y, m, 0.05, 1.0, False, None), axis=1)
        _cache["determinism"] = flat
    return _cache["determinism"]


@pytest.mark.parametrize("rsqrt", ["quake", "exact"])
def test_two_handles_agree_and_a_permutation_permutes_the_bits(rsqrt):
    flat = determinism_input()
    perm = np.random.default_rng(18).permutation(flat.shape[0])
    out = []
    for f in (flat, flat, flat[perm]):
        with rel_sim(bodies_of(f), 0.005, True, eps=0.05, theta=1.0, rsqrt=rsqrt) as sim:
            group = group_of(sim)
            out.append(sim.accelerations())
    assert out[0].any()
    assert_bits(out[1], out[0], "second handle")
    assert_bits(out[2], out[0][perm], "permuted bodies")
    want = model("determinism", flat, 0.05, 1.0, 0.005, rsqrt == "quake", group, True)
    if rsqrt == "exact":
        assert_within_bar(out[0], want[1], f"duplicates and tracers, group {group}")
    else:
        assert_bits(out[0], want[0], "duplicates and tracers")


# ---------------------------------------------------------------------------------------------------------------------
# 7: with the tree energy
# ---------------------------------------------------------------------------------------------------------------------
def close(got, want, bar, what):
    print(f"{what}: got {got:.15e} want {want:.15e} relative {abs(got - want) / abs(want) if want else abs(got):.3g} (bar {bar:g})")
    return abs(got - want) <= bar * abs(want)


@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("name,aprev", CASES)
def test_energy_walks_with_the_same_predicate(name, aprev, quad):
    """nb_energy takes the nodes a force evaluation issued now would take (windows of 64, acc[] of this moment): the model's
    potential over the relative walk's terms to 1e-10, and not the theta walk's value."""
    flat, eps = fixture(name, aprev)
    theta, alpha = 1.0, 0.005
    x, y, m, tree, mom = tree_of(name, flat)
    with rel_sim(bodies_of(flat), alpha, quad, eps=eps, theta=theta, rsqrt="exact", tree_energy=True) as sim:
        assert sim.describe().endswith(f" energy=tree alpha={alpha:g}")
        k, u = sim.energy()
    pairs = trm.pairs_of(tree, x, y, m, flat[:, 4:6], eps, theta, alpha, 64)[0]
    w = m.astype(np.float64)
    mu = float(0.5 * np.sum(np.where(w != 0, w * tem.phi(tree, mom, x, y, m, eps, theta, quad, pairs), 0.0)))
    plain = tem.potential(x, y, m, eps, theta, quad, tree, mom)
    ok_u = close(u, mu, ENERGY_BAR, f"{name} {aprev} quad {quad} U")
    ok_k = close(k, tem.kinetic(flat[:, 2], flat[:, 3], m), 1e-12, f"{name} {aprev} quad {quad} K")
    assert ok_u and ok_k
    assert not close(u, plain, ENERGY_BAR, "U of the theta walk")


def test_energy_at_theta_zero_is_the_direct_energy_and_touches_nothing():
    flat, eps = fixture("plummer_1024")
    kw = dict(eps=eps, rsqrt="exact", tree_energy=True)
    with rel_sim(bodies_of(flat), 0.005, True, theta=0.0, **kw) as t, nb.Simulation(bodies_of(flat), eps=eps, device=0) as d:
        (k, u), (dk, du) = t.energy(), d.energy()
    assert close(u, du, ENERGY_BAR, "theta 0 U against the direct handle") and close(k, dk, 1e-12, "theta 0 K against the direct handle")
    end = []
    for interleave in (True, False):
        with rel_sim(bodies_of(flat), 0.005, True, theta=1.0, **kw) as sim:
            before = sim.sync()["acc"].copy()
            if interleave:
                sim.energy()
                assert_bits(sim.sync()["acc"], before, "acc after energy()")
            for _ in range(4):
                if interleave:
                    sim.energy()
                sim.advance(1, 1e-3)
            assert sim.frame == 4
            end.append({f: sim.sync()[f].copy() for f in ("pos", "vel", "acc")})
    for f in ("pos", "vel", "acc"):
        assert end[0][f].any()
        assert_bits(end[0][f], end[1][f], f"{f} with and without interleaved energy()")


# ---------------------------------------------------------------------------------------------------------------------
# 8: the setter
# ---------------------------------------------------------------------------------------------------------------------
def test_the_setter_and_describe():
    flat, eps = fixture("random_333")
    lib = nb.load()
    for kw in (dict(), dict(force="tree"), dict(force="tree", tree_leaves=True), dict(force="tree", tree_leaves=True, tree_quadrupole=True)):
        with nb.Simulation(bodies_of(flat), eps=eps, device=0, **kw) as sim:
            assert "alpha=" not in sim.describe()
            with pytest.raises(L.NBodyError) as e:
                sim.set_tree_alpha(0.005)
            assert e.value.code == L.NB_ESTATE and "NB_FLAG_TREE_RELATIVE" in str(e.value)
    with rel_sim(bodies_of(flat), 0.005, eps=eps) as sim:
        assert sim.describe().endswith(" alpha=0.005")
        for bad in (-1.0, -1e-30, float("nan"), float("inf")):
            with pytest.raises(L.NBodyError) as e:
                sim.set_tree_alpha(bad)
            assert e.value.code == L.NB_EINVAL and "finite and >= 0" in str(e.value)
            assert lib.nb_last_error_code() == L.NB_EINVAL
        assert sim.describe().endswith(" alpha=0.005")                          # a refused value changes nothing
        sim.set_tree_alpha(0.0025)
        assert sim.describe().endswith(" alpha=0.0025")
    with pytest.raises(L.NBodyError) as e:                                      # the constructor passes a bad value on, and no handle is left
        rel_sim(bodies_of(flat), -0.5, eps=eps)
    assert e.value.code == L.NB_EINVAL


def test_the_c_driver_takes_alpha():
    exe = ROOT / "build" / "nbody_main"
    if not exe.exists():
        subprocess.run(["make", "-C", str(ROOT / "nbodysim_amd" / "host")], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), "-n", "4096", "-s", "5", "-tree", "1.0", "-leaves", "-quad", "-alpha", "0.0025"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " leaves=1 walk=group quad=1 alpha=0.0025" in r.stdout
    r = subprocess.run([str(exe), "-n", "4096", "-s", "5", "-tree", "1.0", "-alpha", "0.0025"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NB_FLAG_TREE_RELATIVE without NB_FLAG_TREE_LEAVES" in r.stderr
