"""GPU: the quadrupole term of the convergent Barnes-Hut force (NB_FLAG_TREE_QUADRUPOLE) against its numpy statement
(tests/tree_quad_model.py) — bit for bit with the Quake rsqrt, within the fast tree mode's bar with the hardware rsqrt — against the
handle without the bit at theta = 0, against the float64 direct sum for what the term buys, and composed with the rest of a tree
handle."""
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
import tree_leaves_model as tlm  # noqa: E402
import tree_model as tm  # noqa: E402
import tree_quad_model as tqm  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
# 333 = 5 * 64 + 13: a ragged last wave; the first 4096 default bodies carry the 1e9 central mass
FIXTURES = {"random_333": ("ic_random_333.npy", 0.5), "plummer_1024": ("ic_plummer_1024.npy", 0.05), "default_4096": ("default_ics_first4096.npy", 1.0)}
THETAS = [1.0, 0.5]
MAX_ERR, MEDIAN_ERR = 2e-5, 2e-6          # of max |a|: the bar of the fast tree mode (test_tree_gpu.py), DESIGN.md 2
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


def model(key, flat, eps, theta, quake, group):
    """The model's accelerations and, for the exact mode, its terms re-summed in float64; computed once per (input, theta, walk)."""
    key = (key, theta, quake, group)
    if key not in _cache:
        x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
        tkey = (key[0], "tree")
        if tkey not in _cache:
            tree = tm.build_canonical(x, y, m)
            _cache[tkey] = (tree, tqm.moments(tree))
        tree, mom = _cache[tkey]
        if quake:
            _cache[key] = (np.stack(tqm.walk(tree, mom, x, y, m, eps, theta, quake=True, group=group), axis=1), None)
        else:
            ax, ay, pairs = tqm.walk(tree, mom, x, y, m, eps, theta, quake=False, group=group, visited=True)
            _cache[key] = (np.stack([ax, ay], axis=1), np.stack(tqm.resum_f64(tree, mom, x, y, pairs, eps), axis=1))
    return _cache[key]


def quad_sim(bodies, **kw):
    return nb.Simulation(bodies, force="tree", tree_leaves=True, tree_quadrupole=True, device=0, **kw)


def leaves_sim(bodies, **kw):
    return nb.Simulation(bodies, force="tree", tree_leaves=True, device=0, **kw)


def group_of(sim, quad=True):
    d = sim.describe()
    assert " leaves=1 walk=" in d and (" quad=1" in d) == quad, d
    walk = d.split(" walk=")[1].split()[0]
    assert walk in ("lane", "group")
    if quad:
        assert f"leaves=1 walk={walk} quad=1" in d, d
    return 64 if walk == "group" else None


def assert_bits(got, want, what):
    for c in range(2):
        g, w = np.ascontiguousarray(got[:, c], np.float32), np.ascontiguousarray(want[:, c], np.float32)
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, f"{what}: column {c} differs in {bad.size} of {g.size} bodies, first {bad[:6]} ({g[bad[:3]]} vs {w[bad[:3]]})"


def assert_within_bar(got, want, what):
    got, want = got.astype(np.float64), np.asarray(want, np.float64)
    scale = np.hypot(want[:, 0], want[:, 1]).max()
    if scale == 0:
        assert not got.any(), what
        return
    err = np.hypot(got[:, 0] - want[:, 0], got[:, 1] - want[:, 1]) / scale
    print(f"{what}: max {err.max():.3g} median {np.median(err):.3g} of max |a|")
    assert err.max() <= MAX_ERR and np.median(err) <= MEDIAN_ERR, what


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_quake_mode_equals_the_model_bit_for_bit(name, theta):
    flat, eps = fixture(name)
    with quad_sim(bodies_of(flat), eps=eps, theta=theta, rsqrt="quake") as sim:
        assert "leaves=1 walk=lane quad=1" in sim.describe()
        got = sim.accelerations()
    want = model(name, flat, eps, theta, True, None)[0]
    assert_bits(got, want, f"{name} theta {theta}")
    # (the term is there: the bits are not those of the walk without it)
    x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
    mono = np.stack(tlm.walk(_cache[(name, "tree")][0], x, y, m, eps, theta, quake=True), axis=1)
    assert not np.array_equal(mono, want)


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_exact_mode_error_against_the_models_terms(name, theta):
    """The walk nb_describe names (walk=lane: every body on its own; walk=group: windows of 64 in key order) takes the model's
    terms: against their float64 sum, the quadrupole part included, at most 2e-5 of max |a|, median at most 2e-6."""
    flat, eps = fixture(name)
    with quad_sim(bodies_of(flat), eps=eps, theta=theta, rsqrt="exact") as sim:
        group = group_of(sim)
        got = sim.accelerations()
    assert_within_bar(got, model(name, flat, eps, theta, False, group)[1], f"{name} theta {theta} group {group}")


# ---------------------------------------------------------------------------------------------------------------------
# 3: theta = 0 accepts no cell
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rsqrt", ["quake", "exact"])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_theta_zero_is_the_leaves_handle_bit_for_bit(name, rsqrt):
    flat, eps = fixture(name)
    with quad_sim(bodies_of(flat), eps=eps, theta=0.0, rsqrt=rsqrt) as q, leaves_sim(bodies_of(flat), eps=eps, theta=0.0, rsqrt=rsqrt) as l:
        assert group_of(q) == group_of(l, quad=False)
        got, want = q.accelerations(), l.accelerations()
    assert want.any()
    assert_bits(got, want, f"{name} theta 0 {rsqrt}")


# ---------------------------------------------------------------------------------------------------------------------
# 4: what the term buys, on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_the_quadrupole_term_pays_on_the_device():
    """ic_plummer_4096, eps 0.05, exact-mode handles, the walk nb_describe names; per body the error relative to its own float64
    direct-sum |a|.  The median with the bit is at most a quarter of the median without it at theta 0.7 and 0.5, and with the bit
    at theta = 0.7 it is below the one without it at theta = 0.5."""
    import nbo
    flat = np.load(GOLD / "ic_plummer_4096.npy").astype(np.float32)
    flat[:, 7] = 0.0
    eps = 0.05
    st = {k: flat[:, i].astype(np.float64) for k, i in (("x", 0), ("y", 1), ("m", 6))}
    ex, ey = nbo.accel_f64(st, eps)
    med, walks = {}, set()
    for theta in (0.7, 0.5):
        for quad in (False, True):
            with (quad_sim if quad else leaves_sim)(bodies_of(flat), eps=eps, theta=theta, rsqrt="exact") as sim:
                walks.add(group_of(sim, quad))
                a = sim.accelerations().astype(np.float64)
            med[theta, quad] = float(np.median(np.hypot(a[:, 0] - ex, a[:, 1] - ey) / np.hypot(ex, ey)))
    assert len(walks) == 1
    print(f"walk group {walks}: " + ", ".join(f"theta {t} {'quadrupole' if q else 'monopole'} {v:.3g}" for (t, q), v in med.items()))
    for theta in (0.7, 0.5):
        assert med[theta, True] <= 0.25 * med[theta, False], theta
    assert med[0.7, True] < med[0.5, False]


# ---------------------------------------------------------------------------------------------------------------------
# 5: small cases
# ---------------------------------------------------------------------------------------------------------------------
def small_cases():
    rng = np.random.default_rng(11)
    n = 300
    flat = np.zeros((n, 8), np.float32)
    flat[:, 0:2] = rng.normal(0, 1, (n, 2))
    flat[:, 6] = rng.uniform(0.5, 2.0, n)
    co = flat.copy()
    co[100, 0:2] = co[99, 0:2]                               # a coincident pair inside the cluster, different masses
    co[100, 6] = 5.0
    tracer = flat.copy()
    tracer[[5, 77, 299], 6] = 0.0
    point = flat[:40].copy()
    point[:, 0:2] = point[0, 0:2]
    return {"coincident_pair": co, "tracer": tracer, "one": flat[:1].copy(), "two": flat[:2].copy(), "one_point": point}


@pytest.mark.parametrize("rsqrt", ["quake", "exact"])
@pytest.mark.parametrize("case", ["coincident_pair", "tracer", "one", "two", "one_point"])
def test_small_cases(case, rsqrt):
    flat, eps, theta = small_cases()[case], 0.05, 0.7
    with quad_sim(bodies_of(flat), eps=eps, theta=theta, rsqrt=rsqrt) as sim:
        group = group_of(sim)
        got = sim.accelerations()
    if rsqrt == "quake":
        assert group is None
        assert_bits(got, model("small_" + case, flat, eps, theta, True, None)[0], case)
    else:
        assert_within_bar(got, model("small_" + case, flat, eps, theta, False, group)[1], f"{case} group {group}")
    tree = _cache[("small_" + case, "tree")][0]
    if case in ("one", "two", "one_point"):                  # no branch is ever accepted: the bits of the handle without the bit
        with leaves_sim(bodies_of(flat), eps=eps, theta=theta, rsqrt=rsqrt) as sim:
            assert_bits(got, sim.accelerations(), case + " against the leaves handle")
    if case in ("one", "one_point"):
        assert not (tree["child"] != 0).any() and not got.any()
    if case == "two":
        assert got.any()
    if case == "coincident_pair":
        assert_bits(got[100:101], got[99:100], "two bodies on one position")
    if case == "tracer":                                     # not inserted, still accelerated: each by its own per-lane walk
        t = [5, 77, 299]
        assert got[t].any(axis=1).all()
        lane = model("small_tracer", flat, eps, theta, rsqrt == "quake", None)
        if rsqrt == "quake":
            assert_bits(got[t], lane[0][t], "tracers")
        else:
            assert_within_bar(got[t], lane[1][t], "tracers against the per-lane walk")


# ---------------------------------------------------------------------------------------------------------------------
# 6: determinism
# ---------------------------------------------------------------------------------------------------------------------
def determinism_input():
    """ic_plummer_1024 with 8 bodies duplicated onto others' positions, one more pair made to straddle the boundary between the
    first two windows of 64 (the body at sorted position 63 and a later body moved onto it), and three massless tracers."""
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


@pytest.mark.parametrize("rsqrt", ["quake", "exact"])
def test_two_handles_agree_and_a_permutation_permutes_the_bits(rsqrt):
    flat = determinism_input()
    perm = np.random.default_rng(18).permutation(flat.shape[0])
    out = []
    for f in (flat, flat, flat[perm]):
        with quad_sim(bodies_of(f), eps=0.05, theta=0.5, rsqrt=rsqrt) as sim:
            group = group_of(sim)
            out.append(sim.accelerations())
    assert out[0].any()
    assert_bits(out[1], out[0], "second handle")
    assert_bits(out[2], out[0][perm], "permuted bodies")
    want = model("determinism", flat, 0.05, 0.5, rsqrt == "quake", group)
    if rsqrt == "exact":
        assert_within_bar(out[0], want[1], f"duplicates and tracers, group {group}")
    else:
        assert_bits(out[0], want[0], "duplicates and tracers")


# ---------------------------------------------------------------------------------------------------------------------
# 7: composition
# ---------------------------------------------------------------------------------------------------------------------
def test_collisions_compose_and_the_profile_counts_one_interval_per_evaluation():
    ic = np.load(GOLD / "collide_isolated_ic.npy")
    for rsqrt in ("quake", "exact"):
        with quad_sim(bodies_of(ic), eps=1.0, collide=True, rsqrt=rsqrt) as sim:
            sim.profile(True)
            sim.advance(3, 1.0 / 64.0)
            sim.wait()
            ms, launches = sim.profile_read()
            assert launches == 3 and ms > 0
            assert sim.frame == 3 and sim.collision_stats()["pairs_total"] > 0
            assert sim.tree_stats()["overflow_steps"] == 0


def test_depth_cap_is_reported_once_and_the_handle_stays_usable():
    """Pairs of positions one ulp apart that no rounded child centre separates, as tests/test_tree_leaves_gpu.py builds them."""
    n = 512
    k = np.arange(n // 2)
    flat = np.zeros((n, 8), np.float32)
    flat[0::2, 0], flat[0::2, 1] = (k % 16) - 7.25, (k // 16) - 7.25
    flat[1::2, 0], flat[1::2, 1] = np.nextafter(flat[0::2, 0], np.float32(99)), flat[0::2, 1]
    flat[:, 2], flat[:, 6] = 0.5, 1.0 / n
    with pytest.raises(OverflowError):
        tm.build_canonical(flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy())
    ic = bodies_of(flat)
    for rsqrt in ("quake", "exact"):
        with quad_sim(ic, eps=0.05, rsqrt=rsqrt) as sim:
            sim.advance(1, 1e-3)
            with pytest.raises(L.NBodyError) as e:
                sim.sync()
            assert e.value.code == L.NB_ENOMEM and "not separated within 63 levels" in str(e.value)
            assert np.array_equal(sim.sync()["pos"], ic["pos"]) and sim.tree_stats()["overflow_steps"] == 1     # reported once
            good, eps = fixture("plummer_1024")
            sim.upload(bodies_of(good[:n]))
            got, group = sim.accelerations(), group_of(sim)
            assert sim.tree_stats()["overflow_steps"] == 1
        want = model("plummer_first512", good[:n], 0.05, 1.0, rsqrt == "quake", group)
        if rsqrt == "quake":
            assert_bits(got, want[0], "after the failed build")
        else:
            assert_within_bar(got, want[1], "after the failed build")
