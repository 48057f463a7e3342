"""GPU: the Barnes-Hut force (NB_FORCE_TREE) against the reference's own step() — committed fixtures and the live compiled
reference — and against the numpy statement (tests/tree_model.py), bit for bit in the reference's arithmetic."""
import ctypes as C
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import collide_model as cm  # noqa: E402
import tree_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
COLS = (("pos", 0), ("pos", 1), ("vel", 0), ("vel", 1), ("acc", 0), ("acc", 1))


def bodies_of(flat: np.ndarray) -> np.ndarray:
    b = nb.bodies_array(flat.shape[0])
    b["pos"], b["vel"], b["acc"] = flat[:, 0:2], flat[:, 2:4], flat[:, 4:6]
    b["mass"], b["radius"] = flat[:, 6], flat[:, 7]
    return b


def flat_of(b: np.ndarray) -> np.ndarray:
    out = np.zeros((b.shape[0], 8), np.float32)
    out[:, 0:2], out[:, 2:4], out[:, 4:6], out[:, 6], out[:, 7] = b["pos"], b["vel"], b["acc"], b["mass"], b["radius"]
    return out


def assert_bits(got: np.ndarray, want: np.ndarray, what: str, cols=range(6)):
    for c in cols:
        g, w = np.ascontiguousarray(got[:, c], np.float32), np.ascontiguousarray(want[:, c], np.float32)
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, f"{what}: column {c} differs in {bad.size} of {g.size} bodies, first {bad[:6]} ({g[bad[:3]]} vs {w[bad[:3]]})"


def tree_sim(bodies, **kw):
    kw.setdefault("rsqrt", "quake")
    return nb.Simulation(bodies, force="tree", device=0, **kw)


def model_acc(flat, eps, theta=1.0):
    ax, ay = tm.accelerations(flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy(), eps, theta)
    return np.stack([ax, ay], axis=1)


def live_reference(flat, eps, dt, steps):
    import nbo
    if not nbo.have_ref():
        pytest.skip("the compiled reference (oracle/_ref/libnbref.so) is not built here")
    f = np.ascontiguousarray(flat.copy())
    t = time.time()
    assert nbo.ref().ref_step(f.reshape(-1), f.shape[0], eps, dt, steps) == steps
    print(f"reference step(): n={f.shape[0]} {steps} step(s) in {time.time() - t:.1f} s")
    return f


# ---------------------------------------------------------------------------------------------------------------------
# bit-exact against the reference's step()
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_frames_of_the_reference_step():
    """NB_FORCE_TREE + NB_RSQRT_QUAKE reproduces ref_step_s{1,10,100}.npy (the reference's real step() on ic_plummer_1024)."""
    ic = np.load(GOLD / "ic_plummer_1024.npy")
    with tree_sim(bodies_of(ic), eps=0.05) as sim:
        assert "force=tree" in sim.describe() and "symmetric=0" in sim.describe()
        for steps in (1, 10, 100):
            sim.advance(steps - sim.frame, 1e-3)
            assert_bits(flat_of(sim.sync()), np.load(GOLD / f"ref_step_s{steps}.npy"), f"step {steps}")
        st = sim.tree_stats()
        assert st["overflow_steps"] == 0 and 1024 < st["nodes"] < 16 * 1024 and 5 < st["max_depth"] < 40


def test_reference_default_workload():
    """The reference's own 25 000 bodies (radius 0), clamp and boundary on, eps = 1, dt = 0.01: 1 and 5 steps of its step()."""
    man = json.loads((GOLD / "tree_manifest.json").read_text())
    ic = nb.default_ics(man["n"])
    ic["radius"] = 0.0
    with tree_sim(ic, eps=man["eps"], extras=L.NB_EXTRA_VCLAMP | L.NB_EXTRA_BOUNDARY) as sim:
        for steps in (1, 5):
            sim.advance(steps - sim.frame, man["dt"])
            got = flat_of(sim.sync())
            entry = man["steps"][str(steps)]
            assert_bits(got[: man["rows"]], np.load(GOLD / entry["file"]), f"default bodies, step {steps}")
            assert hashlib.sha256(got.astype("<f4").tobytes()).hexdigest() == entry["sha256_float32_le"], f"step {steps}: full array"
        print("default bodies:", sim.tree_stats())


def test_one_million_bodies_equal_the_live_reference():
    """N = 1 048 576 Plummer, eps = 0.01, dt = 1e-3, one step, every body (the reference's step takes 1 - 6 s on 16 cores, under the two-minute rule)."""
    n = 1 << 20
    ic = nb.plummer_2d(n, 42)
    want = live_reference(flat_of(ic), 0.01, 1e-3, 1)
    with tree_sim(ic, eps=0.01) as sim:
        sim.advance(1, 1e-3)
        got = flat_of(sim.sync())
        print("1 048 576 bodies:", sim.tree_stats())
    assert_bits(got, want, "1 048 576 bodies")


def test_eight_million_bodies():
    """Beyond the direct path's reach: N = 8 388 608 creates and steps twice in O(n) device memory (under 1 KiB per body; the
    symmetric slabs alone would be ~128 GiB), and its first step equals the live reference in every body (12 - 36 s on 16 cores, under the two-minute rule)."""
    n = 1 << 23
    ic = nb.plummer_2d(n, 42)
    hip = C.CDLL("libamdhip64.so")
    free0, free1, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free0), C.byref(total)) == 0
    with tree_sim(ic, eps=0.01) as sim:
        assert hip.hipMemGetInfo(C.byref(free1), C.byref(total)) == 0
        per_body = (free0.value - free1.value) / n
        print(f"8 388 608 bodies: {per_body:.0f} bytes of device memory per body")
        assert per_body < 1024
        sim.advance(1, 1e-3)
        got = flat_of(sim.sync())
        sim.advance(1, 1e-3)
        sim.wait()
        st = sim.tree_stats()
        print("8 388 608 bodies:", st)
        assert sim.frame == 2 and st["overflow_steps"] == 0 and n < st["nodes"] <= 16 * n + 4096
    want = live_reference(flat_of(ic), 0.01, 1e-3, 1)
    assert_bits(got, want, "8 388 608 bodies")


# ---------------------------------------------------------------------------------------------------------------------
# against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workload", ["plummer_65536", "default"])
def test_fast_mode_error_against_the_accepted_nodes(workload):
    """NB_RSQRT_EXACT: the accelerations against the model's accepted nodes re-summed in float64 with an exact 1/sqrt: at most
    2e-5 of the force scale max |a|, median at most 2e-6 (the bar of the direct fast mode)."""
    if workload == "default":
        ic, eps = nb.default_ics(25000), 1.0
    else:
        ic, eps = nb.plummer_2d(65536, 42), 0.01
    flat = flat_of(ic)
    x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
    tree = tm.build_canonical(x, y, m)
    _, _, pairs = tm.walk(tree, x, y, eps, visited=True)
    ax, ay = tm.resum_f64(tree, x, y, pairs, eps)
    with tree_sim(ic, eps=eps, rsqrt="exact") as sim:
        got = sim.accelerations().astype(np.float64)
    err = np.hypot(got[:, 0] - ax, got[:, 1] - ay) / np.hypot(ax, ay).max()
    print(f"{workload}: max {err.max():.3g} median {np.median(err):.3g} of max |a|")
    assert err.max() <= 2e-5 and np.median(err) <= 2e-6


def test_fast_mode_accepts_the_same_nodes():
    """The acceptance test is the same code in both modes.  theta = 0 accepts nothing: all zero in the exact mode too.  And per
    body, exact and Quake differ by at most 6e-3 of the sum of the magnitudes of that body's accepted terms: the Quake rsqrt is
    within 1.75e-3 of 1/sqrt (Quadtree.hpp:106-111), its cube within 5.3e-3, the rest is rounding.  A coarse net (a light
    wrongly accepted node can hide in it); the bit-exact Quake tests are what pins the acceptance."""
    flat = np.load(GOLD / "ic_plummer_4096.npy")
    with tree_sim(bodies_of(flat), eps=0.05, rsqrt="exact", theta=0.0) as sim:
        assert not sim.accelerations().any()
    with tree_sim(bodies_of(flat), eps=0.05, rsqrt="exact") as e, tree_sim(bodies_of(flat), eps=0.05) as q:
        ae, aq = e.accelerations().astype(np.float64), q.accelerations().astype(np.float64)
    x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
    tree = tm.build_canonical(x, y, m)
    _, _, pairs = tm.walk(tree, x, y, 0.05, visited=True)
    nd = pairs[:, 1]
    dx, dy = tree["px"][nd].astype(np.float64) - x[pairs[:, 0]], tree["py"][nd].astype(np.float64) - y[pairs[:, 0]]
    r2 = dx * dx + dy * dy + 0.05 ** 2
    scale = np.bincount(pairs[:, 0], tree["mass"][nd] * np.hypot(dx, dy) / (r2 * np.sqrt(r2)), flat.shape[0])   # sum of |terms| per body
    assert (np.hypot(ae[:, 0] - aq[:, 0], ae[:, 1] - aq[:, 1]) <= 6e-3 * scale).all()


@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_other_opening_parameters(theta):
    flat = np.load(GOLD / "ic_plummer_1024.npy")
    with tree_sim(bodies_of(flat), eps=0.05, theta=theta) as sim:
        got = sim.accelerations()
    assert_bits(got, model_acc(flat, 0.05, theta), f"theta {theta}", cols=range(2))
    if theta == 0.0:
        assert not got.any()                                # every branch is opened and a leaf adds nothing


def small_cases():
    rng = np.random.default_rng(11)
    n = 300
    flat = np.zeros((n, 8), np.float32)
    flat[:, 0:2] = rng.normal(0, 1, (n, 2))
    flat[:, 6] = rng.uniform(0.5, 2.0, n)
    co = flat.copy()
    co[100:110, 0:2] = co[99, 0:2]                           # ten bodies on one position, different masses
    co[100, 6] = 1e8
    tracer = flat.copy()
    tracer[[5, 77, 299], 6] = 0.0
    one = flat[:1].copy()
    two = flat[:2].copy()
    point = flat[:40].copy()
    point[:, 0:2] = point[0, 0:2]
    return {"coincident": co, "tracer": tracer, "one": one, "two": two, "one_point": point}


@pytest.mark.parametrize("case", ["coincident", "tracer", "one", "two", "one_point"])
def test_small_cases_equal_the_model(case):
    flat = small_cases()[case]
    with tree_sim(bodies_of(flat), eps=0.05) as sim:
        got = sim.accelerations()
        st = sim.tree_stats()
    assert_bits(got, model_acc(flat, 0.05), case, cols=range(2))
    assert st["nodes"] == tm.build_canonical(flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy())["px"].shape[0]
    if case == "tracer":
        assert got[5].any() and got[77].any()


def test_body_order_changes_no_bit():
    flat = np.load(GOLD / "ic_plummer_4096.npy")
    perm = np.random.default_rng(3).permutation(flat.shape[0])
    out = []
    for f in (flat, flat[perm]):
        with tree_sim(bodies_of(f), eps=0.05) as sim:
            sim.advance(3, 1e-3)
            out.append(flat_of(sim.sync()))
    assert_bits(out[1], out[0][perm], "permuted bodies")


def test_two_handles_agree_bit_for_bit():
    ic = nb.plummer_2d(20000, 7)
    out = []
    for _ in range(2):
        with tree_sim(ic, eps=0.01, rsqrt="exact") as sim:
            sim.advance(10, 1e-3)
            out.append(flat_of(sim.sync()))
    assert_bits(out[1], out[0], "second handle")


# ---------------------------------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_combination():
    ic = nb.plummer_2d(64, 1)
    for kw, text in ((dict(precision="fp64", rsqrt="exact"), "NB_FP64"), (dict(dims=3), "dims = 3"),
                     (dict(shard_world=2, shard_rank=0, i_begin=0, i_count=32), "shard_world"), (dict(integrator="kdk"), "KDK")):
        with pytest.raises(L.NBodyError) as e:
            tree_sim(ic, **kw)
        assert e.value.code == L.NB_EINVAL and text in str(e.value) and "NB_FORCE_TREE" in str(e.value)
    with nb.Simulation(ic, device=0) as direct:
        assert "force=direct" in direct.describe()
        with pytest.raises(L.NBodyError) as e:
            direct.tree_stats()
        assert e.value.code == L.NB_ESTATE


IGNORED = [dict(symmetry=False), dict(uniform_mass=False), dict(guided_tail=False), dict(mass_scaling=True), dict(mass_scaling="measured"),
           dict(mass_scaling=None), dict(static_items=True), dict(j_slices=3), dict(lanes_p=2), dict(sym_tile=512), dict(sym_chunks_per_item=4),
           dict(sym_aux_stream=1), dict(sym_late_us=10.0), dict(sym_tail=(0.5, 0.6, 0.7)), dict(sym_chunk_pairs=1)]


@pytest.mark.parametrize("rsqrt", ["exact", "quake"])
def test_ignored_flags_and_tuning_fields_change_nothing(rsqrt):
    """Every field include/nbody.h lists as ignored, on bodies with unequal positive masses (the data the direct-sum
    specialisations look at): same bits, and no direct-sum launch (the handle has no slabs for one to write)."""
    ic = nb.default_ics(25000)
    with tree_sim(ic, eps=1.0, rsqrt=rsqrt) as plain:
        want = plain.accelerations()
    for kw in IGNORED:
        with tree_sim(ic, eps=1.0, rsqrt=rsqrt, **kw) as sim:
            d = sim.describe()
            assert "uniform_mass=0 mass_scaled=0" in d and "symmetric=0" in d, (kw, d)
            assert_bits(sim.accelerations(), want, str(kw), cols=range(2))
            sim.upload(ic)                                   # the upload-time mass-scaling check must not run either
            sim.profile(True)
            sim.advance(1, 0.01)
            assert sim.profile_read()[1] == 1, kw            # one force launch: the walk


def test_caller_owned_position_buffers():
    hip = C.CDLL("libamdhip64.so")
    ic = nb.plummer_2d(4096, 5)
    bufs = [C.c_void_p(), C.c_void_p()]
    for b in bufs:
        assert hip.hipMalloc(C.byref(b), C.c_size_t(ic.shape[0] * 8)) == 0
    try:
        with tree_sim(ic, eps=0.01) as own, tree_sim(ic, eps=0.01, pos_buffers=(bufs[0].value, bufs[1].value)) as ext:
            own.advance(3, 1e-3)
            ext.advance(3, 1e-3)
            assert ext.pos_buffer() in (bufs[0].value, bufs[1].value)
            assert_bits(flat_of(ext.sync()), flat_of(own.sync()), "caller-owned pos_buffers")
    finally:
        for b in bufs:
            assert hip.hipFree(b) == 0


def close_pairs(n: int = 512, one_ulp: bool = False) -> np.ndarray:
    """n / 2 pairs of bodies 2^-18 apart, the pairs a unit apart on a 16 x 16 grid: parting a pair takes about 22 levels of
    four nodes each, some 40 n nodes in all — more than the capacity of 16 n + 4096."""
    k = np.arange(n // 2)
    flat = np.zeros((n, 8), np.float32)
    flat[0::2, 0], flat[0::2, 1] = (k % 16) - 7.25, (k // 16) - 7.25
    flat[1::2, 0], flat[1::2, 1] = flat[0::2, 0] + np.float32(2.0 ** -18), flat[0::2, 1]
    if one_ulp:
        flat[1::2, 0] = np.nextafter(flat[0::2, 0], np.float32(99))
    flat[:, 2], flat[:, 6] = 0.5, 1.0 / n
    return flat


def test_capacity_overflow_is_reported_once_and_the_handle_stays_usable():
    flat = close_pairs()
    n = flat.shape[0]
    need = tm.build_canonical(flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy())["px"].shape[0]
    assert need > 16 * n + 4096
    ic = bodies_of(flat)
    with tree_sim(ic, eps=0.05) as sim:
        sim.advance(1, 1e-3)
        with pytest.raises(L.NBodyError) as e:
            sim.wait()
        assert e.value.code == L.NB_ENOMEM and "frame 0" in str(e.value) and f"needed {need} nodes" in str(e.value)
        assert f"capacity of {16 * n + 4096}" in str(e.value)
        sim.wait()                                          # reported once
        b = sim.sync()
        assert sim.frame == 1 and np.array_equal(b["pos"], ic["pos"]) and np.array_equal(b["vel"], ic["vel"])   # nothing was integrated
        assert sim.tree_stats()["overflow_steps"] == 1
        sim.advance(1, 1e-3)                                # the next evaluation fails again and says so
        with pytest.raises(L.NBodyError):
            sim.sync()
        good = np.load(GOLD / "ic_plummer_1024.npy")[:n]
        sim.upload(bodies_of(good))
        sim.advance(1, 1e-3)
        st = {k: good[:, i].copy() for i, k in enumerate(("x", "y", "vx", "vy", "ax", "ay", "m"))}
        tm.step(st, 0.05, 1e-3, 1)
        assert_bits(flat_of(sim.sync()), np.stack([st[k] for k in ("x", "y", "vx", "vy", "ax", "ay")], axis=1), "after the overflow")
        assert sim.tree_stats()["overflow_steps"] == 2


def test_depth_cap_is_reported():
    """Pairs of positions one ulp apart that no rounded child centre separates (the reference's insert would not return): the
    evaluation fails, integrates nothing and is reported once."""
    flat = close_pairs(one_ulp=True)
    with pytest.raises(OverflowError):
        tm.build_canonical(flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy())
    ic = bodies_of(flat)
    with tree_sim(ic, eps=0.05) as sim:
        sim.advance(1, 1e-3)
        with pytest.raises(L.NBodyError) as e:
            sim.sync()
        assert e.value.code == L.NB_ENOMEM and "not separated within 63 levels" in str(e.value)
        assert np.array_equal(sim.sync()["pos"], ic["pos"]) and sim.tree_stats()["overflow_steps"] == 1


def test_collisions_compose_with_the_tree_force():
    ic = np.load(GOLD / "collide_isolated_ic.npy")
    dt = 1.0 / 64.0
    with tree_sim(bodies_of(ic), eps=1.0, collide=True) as sim:
        sim.advance(1, dt)
        got = sim.sync()
        assert sim.collision_stats()["pairs_total"] > 0
    st = {"x": ic[:, 0].copy(), "y": ic[:, 1].copy(), "vx": ic[:, 2].copy(), "vy": ic[:, 3].copy(), "m": ic[:, 6].copy(), "r": ic[:, 7].copy()}
    tm.step(st, 1.0, dt, 1)
    cm.collide(st)
    for k, (f, c) in zip(("x", "y", "vx", "vy", "ax", "ay"), COLS):
        assert cm.same_bits(np.ascontiguousarray(got[f][:, c]), st[k].astype(np.float32)), k


def test_profile_counts_the_walk():
    ic = nb.plummer_2d(4096, 3)
    with tree_sim(ic, eps=0.01) as sim:
        sim.profile(True)
        sim.advance(5, 1e-3)
        ms, launches = sim.profile_read()
        assert launches == 5 and ms > 0
