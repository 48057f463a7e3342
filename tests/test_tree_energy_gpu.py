"""GPU: nb_energy of a NB_FLAG_TREE_ENERGY handle against its numpy statement (tests/tree_energy_model.py), against the direct
nb_energy of a twin handle at theta = 0, and what the call must leave alone."""
import re
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

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
# the fixtures and softenings of tests/test_tree_leaves_gpu.py: 333 = 5 * 64 + 13 is a ragged last wave
FIXTURES = {"random_333": ("ic_random_333.npy", 0.5), "plummer_1024": ("ic_plummer_1024.npy", 0.05), "default_4096": ("default_ics_first4096.npy", 1.0)}
THETAS = [1.0, 0.5, 0.0]
ENERGY_BAR = 1e-10                        # the project's energy bar (tests/test_headline_gpu.py)
_cache = {}


def bodies_of(flat: np.ndarray) -> np.ndarray:
    b = nb.bodies_array(flat.shape[0])
    b["pos"], b["vel"], b["acc"] = flat[:, 0:2], flat[:, 2:4], flat[:, 4:6]
    b["mass"], b["radius"] = flat[:, 6], flat[:, 7]
    return b


def fixture(name):
    if name not in _cache:
        file, eps = FIXTURES[name]
        flat = np.load(GOLD / file).astype(np.float32)
        flat[:, 7] = 0.0
        _cache[name] = (flat, eps)
    return _cache[name]


def small_cases():
    """The small cases of tests/test_tree_leaves_gpu.py, with velocities."""
    rng = np.random.default_rng(11)
    n = 300
    flat = np.zeros((n, 8), np.float32)
    flat[:, 0:2] = rng.normal(0, 1, (n, 2))
    flat[:, 6] = rng.uniform(0.5, 2.0, n)
    flat[:, 2:4] = np.random.default_rng(12).normal(0, 1, (n, 2))
    co = flat.copy()
    co[100:110, 0:2] = co[99, 0:2]                           # ten bodies on one position, different masses
    co[100, 6] = 1e8
    tracer = flat.copy()
    tracer[[5, 77, 299], 6] = 0.0
    point = flat[:40].copy()
    point[:, 0:2] = point[0, 0:2]
    pair = flat[:2].copy()                                   # nothing but two bodies on one position
    pair[1, 0:2] = pair[0, 0:2]
    return {"coincident": co, "tracer": tracer, "one": flat[:1].copy(), "two": flat[:2].copy(), "one_point": point, "coincident_pair": pair}


SHARED = {"coincident", "one_point", "coincident_pair"}      # the small cases with more than one body on a position


def model(key, flat, eps, theta, quad):
    """(K, U) of the model; the tree, the moments and the terms of (input, theta) are computed once."""
    x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
    if (key, "tree") not in _cache:
        tree = tm.build_canonical(x, y, m)
        _cache[key, "tree"] = (tree, tqm.moments(tree))
    tree, mom = _cache[key, "tree"]
    if (key, "pairs", eps, theta) not in _cache:
        _cache[key, "pairs", eps, theta] = tlm.walk(tree, x, y, m, eps, theta, False, 64, True)[2]
    phi = tem.phi(tree, mom, x, y, m, eps, theta, quad, _cache[key, "pairs", eps, theta])
    w = m.astype(np.float64)
    return tem.kinetic(flat[:, 2], flat[:, 3], m), float(0.5 * np.sum(np.where(w != 0, w * phi, 0.0)))


def energy_sim(bodies, **kw):
    kw.setdefault("tree_energy", True)
    return nb.Simulation(bodies, force="tree", tree_leaves=True, device=0, **kw)


def close(got, want, bar, what):
    print(f"{what}: got {got:.15e} want {want:.15e} relative {abs(got - want) / abs(want) if want else abs(got):.3g} (bar {bar:g})")
    return abs(got - want) <= bar * abs(want)


# ---------------------------------------------------------------------------------------------------------------------
# 5: against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_energy_equals_the_model(name, theta, quad):
    """The cells visited are bit-determined and both sides add the same float64 terms: 1e-10."""
    flat, eps = fixture(name)
    with energy_sim(bodies_of(flat), eps=eps, theta=theta, rsqrt="exact", tree_quadrupole=quad) as sim:
        k, u = sim.energy()
    mk, mu = model(name, flat, eps, theta, quad)
    ok_u = close(u, mu, ENERGY_BAR, f"{name} theta {theta} quad {quad} U")
    ok_k = close(k, mk, 1e-12, f"{name} theta {theta} quad {quad} K")
    assert ok_u and ok_k


def test_the_potential_walk_does_not_depend_on_the_rsqrt_mode():
    """A Quake handle's force walks per lane; its potential takes the windows of 64 all the same: the model's value, and the bits
    of the hardware-rsqrt handle's."""
    flat, eps = fixture("plummer_1024")
    out = []
    for rsqrt in ("quake", "exact"):
        with energy_sim(bodies_of(flat), eps=eps, theta=0.5, rsqrt=rsqrt, tree_quadrupole=True) as sim:
            assert ("walk=lane" if rsqrt == "quake" else "walk=") in sim.describe()
            out.append(sim.energy())
    assert close(out[0][1], model("plummer_1024", flat, eps, 0.5, True)[1], ENERGY_BAR, "quake handle U")
    assert out[0] == out[1]


# ---------------------------------------------------------------------------------------------------------------------
# 6: theta = 0 is the direct energy
# ---------------------------------------------------------------------------------------------------------------------
def twin_energies(flat, eps, **kw):
    with energy_sim(bodies_of(flat), eps=eps, theta=0.0, **kw) as t, nb.Simulation(bodies_of(flat), eps=eps, device=0) as d:
        assert "force=direct" in d.describe() and " energy=tree" in t.describe()
        return t.energy(), d.energy()


@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_theta_zero_is_the_direct_energy_on_the_fixtures(name, quad):
    """U within 1e-10 and K within 1e-12 of nb_energy of a direct-sum handle on the same bodies.

    ic_random_333 holds one pair of bodies on one position (bodies 7 and 8, masses 1.943331 and 1.5235044).  Their leaf's record
    carries the float32 sum of the two masses, one rounding of up to 2^-24 relative, which every other body would see: 3.67e-10 of
    U there.  The potential walk therefore takes a shared leaf's mass as the float64 sum of its bodies (tree_leaf_residual,
    nb_tree.hip.h), which this case holds to the bar.  plummer_1024 and default_4096 share no position."""
    flat, eps = fixture(name)
    (k, u), (dk, du) = twin_energies(flat, eps, tree_quadrupole=quad)
    ok_u = close(u, du, ENERGY_BAR, f"{name} quad {quad} U against the direct handle")
    ok_k = close(k, dk, 1e-12, f"{name} quad {quad} K against the direct handle")
    assert ok_u and ok_k


@pytest.mark.parametrize("case", ["coincident", "tracer", "one", "two", "one_point", "coincident_pair"])
def test_theta_zero_is_the_direct_energy_on_the_small_cases(case):
    """2e-6 where positions are shared (the bound of a leaf's float32 mass sum over k bodies, (k - 1) 2^-24, k <= 40; the walk's
    float64 leaf masses stay far inside it), 1e-10 otherwise."""
    flat, eps = small_cases()[case], 0.05
    (k, u), (dk, du) = twin_energies(flat, eps)
    ok_u = close(u, du, 2e-6 if case in SHARED else ENERGY_BAR, f"{case} U against the direct handle")
    ok_k = close(k, dk, 1e-12, f"{case} K against the direct handle")
    assert ok_u and ok_k
    if case == "one":
        assert u == 0.0
    if case == "coincident_pair":
        want = -float(flat[0, 6]) * float(flat[1, 6]) / float(np.float32(eps))
        assert close(u, want, 1e-12, "the one pair, -m1 m2 / eps")
    if case == "tracer":                                     # massless bodies weigh nothing, moving or not
        assert flat[5, 2:4].any()
        assert close(k, tem.kinetic(flat[:, 2], flat[:, 3], flat[:, 6]), 1e-12, "K without the tracers")


# ---------------------------------------------------------------------------------------------------------------------
# 7: eps = 0
# ---------------------------------------------------------------------------------------------------------------------
def test_without_softening_coincident_pairs_are_skipped():
    cases = small_cases()
    for theta in (0.0, 1.0):
        two = cases["two"]
        with energy_sim(bodies_of(two), eps=0.0, theta=theta) as sim:
            _, u = sim.energy()
        r = np.hypot(float(two[1, 0]) - float(two[0, 0]), float(two[1, 1]) - float(two[0, 1]))
        assert close(u, -float(two[0, 6]) * float(two[1, 6]) / r, 1e-12, f"two bodies, eps 0, theta {theta}")
        for case in ("coincident_pair", "one_point"):
            with energy_sim(bodies_of(cases[case]), eps=0.0, theta=theta) as sim:
                k, u = sim.energy()
            assert np.isfinite(u) and u == 0.0 and k > 0, case


# ---------------------------------------------------------------------------------------------------------------------
# 8: no side effects
# ---------------------------------------------------------------------------------------------------------------------
def test_energy_leaves_the_trajectory_alone():
    flat, eps = fixture("plummer_1024")
    end = []
    for flag in (True, False):
        with energy_sim(bodies_of(flat), eps=eps, theta=0.5, tree_quadrupole=True, tree_energy=flag) as sim:
            assert (" energy=tree" in sim.describe()) == flag
            sim.accelerations()
            before = sim.sync()["acc"].copy()
            assert before.any()
            sim.energy()
            assert np.array_equal(sim.sync()["acc"].view(np.uint32), before.view(np.uint32))
            for _ in range(5):
                sim.energy()
                sim.advance(1, 1e-3)
            assert sim.frame == 5
            e = sim.energy()
            assert sim.frame == 5
            end.append({f: sim.sync()[f].copy() for f in ("pos", "vel", "acc")})
            assert np.isfinite(e).all() and sim.tree_stats()["overflow_steps"] == 0
    for f in ("pos", "vel", "acc"):
        assert end[0][f].any() and np.array_equal(end[0][f].view(np.uint32), end[1][f].view(np.uint32)), f


# ---------------------------------------------------------------------------------------------------------------------
# 9: determinism
# ---------------------------------------------------------------------------------------------------------------------
def determinism_input():
    """As tests/test_tree_leaves_gpu.py builds it: ic_plummer_1024 with 8 bodies duplicated onto others' positions, one more pair
    made to straddle the boundary between the first two windows of 64, and three massless tracers."""
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
    return flat


@pytest.mark.parametrize("quad", [False, True])
def test_two_handles_agree_and_a_permutation_agrees(quad):
    flat = determinism_input()
    perm = np.random.default_rng(18).permutation(flat.shape[0])
    out = []
    for f in (flat, flat, flat[perm]):
        with energy_sim(bodies_of(f), eps=0.05, theta=0.5, tree_quadrupole=quad) as sim:
            out.append(sim.energy())
    assert out[0] == out[1]                                  # the same bits of (K, U)
    assert close(out[2][0], out[0][0], 1e-12, "permuted K") and close(out[2][1], out[0][1], 1e-12, "permuted U")
    mk, mu = model("determinism", flat, 0.05, 0.5, quad)
    assert close(out[0][1], mu, ENERGY_BAR, "duplicates and tracers U") and close(out[0][0], mk, 1e-12, "duplicates and tracers K")


# ---------------------------------------------------------------------------------------------------------------------
# 10: a failed build
# ---------------------------------------------------------------------------------------------------------------------
def test_a_failed_build_is_reported_by_the_energy_call():
    """Pairs of positions one ulp apart that no rounded child centre separates, as tests/test_tree_leaves_gpu.py builds them."""
    n = 512
    j = np.arange(n // 2)
    flat = np.zeros((n, 8), np.float32)
    flat[0::2, 0], flat[0::2, 1] = (j % 16) - 7.25, (j // 16) - 7.25
    flat[1::2, 0], flat[1::2, 1] = np.nextafter(flat[0::2, 0], np.float32(99)), flat[0::2, 1]
    flat[:, 2], flat[:, 6] = 0.5, 1.0 / n
    with pytest.raises(OverflowError):
        tm.build_canonical(flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy())
    ic = bodies_of(flat)
    with energy_sim(ic, eps=0.05) as sim:
        with pytest.raises(L.NBodyError) as e:
            sim.energy()
        assert e.value.code == L.NB_ENOMEM and "not separated within 63 levels" in str(e.value)
        got = sim.sync()                                     # reported once: the next synchronising call passes
        assert np.array_equal(got["pos"], ic["pos"]) and np.array_equal(got["vel"], ic["vel"]) and sim.frame == 0
        assert sim.tree_stats()["overflow_steps"] == 1
        good, eps = fixture("plummer_1024")
        sim.upload(bodies_of(good[:n]))
        k, u = sim.energy()
        assert sim.tree_stats()["overflow_steps"] == 1
    mk, mu = model("plummer_first512", good[:n], 0.05, 1.0, False)
    assert close(u, mu, ENERGY_BAR, "U after the failed build") and close(k, mk, 1e-12, "K after the failed build")


# ---------------------------------------------------------------------------------------------------------------------
# 11: describe, the C driver
# ---------------------------------------------------------------------------------------------------------------------
def test_describe_and_the_c_driver():
    ic = nb.plummer_2d(4096, 42)
    with energy_sim(ic, eps=0.01, theta=0.5) as sim:
        assert sim.describe().endswith(" energy=tree")
    with energy_sim(ic, eps=0.01, theta=0.5, tree_quadrupole=True) as sim:
        assert sim.describe().endswith(" quad=1 energy=tree")
    for kw in (dict(force="tree", tree_leaves=True), dict(force="tree"), dict()):
        with nb.Simulation(ic, eps=0.01, device=0, **kw) as sim:
            assert "energy=" not in sim.describe()
    exe = ROOT / "build" / "nbody_main"
    if not exe.exists():
        subprocess.run(["make", "-C", str(ROOT / "nbodysim_amd" / "host")], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), "-n", "4096", "-s", "5", "-tree", "0.5", "-leaves", "-tree-energy"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " energy=tree" in r.stdout
    m = re.search(r"energy: E0=([-+0-9.e]+)  E1=([-+0-9.e]+)  drift=([-+0-9.e]+)", r.stdout)
    assert m and np.isfinite([float(v) for v in m.groups()]).all() and float(m.group(1)) < 0
