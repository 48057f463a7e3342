"""GPU: nb_field — the direct sweeps against the float64 sum (tests/field_model.py), the bit-for-bit ties to nb_potentials and
nb_accelerations at massless tracers, what a row may depend on, the conventions for a point on a body, and what the call must leave
alone."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import field_model as fm  # noqa: E402
import potential_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parents[1] / "tests" / "golden"
BAR_F32 = 4e-6                        # phi, relative: tests/test_potential_cpu.py has the derivation
BAR_ACC = (6.5 + 63) * 2.0 ** -24     # acc per component, of S = sum |term|: tests/test_field_cpu.py has the derivation
BAR_F64 = 1e-12                       # n x 1.1e-16 of sequential float64 adds (n <= 777) + the 1.4e-16 reciprocal square root
SENTINEL = -12345.678


def bodies_of(pos, m, vel=None) -> np.ndarray:
    pos = np.asarray(pos, np.float32)
    b = nb.bodies_array(pos.shape[0])
    v = b.view(L.BODY3_DTYPE) if pos.shape[1] == 3 else b
    v["pos"] = pos
    if vel is not None:
        v["vel"] = vel
    b["mass"] = m
    return b


@functools.lru_cache(maxsize=None)
def gold(name):
    """(pos (n, 2), m, vel) of a golden fixture, read once, shared, read-only."""
    flat = np.load(GOLD / f"{name}.npy").astype(np.float32)
    out = (flat[:, 0:2].copy(), flat[:, 6].copy(), flat[:, 2:4].copy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cloud(n, dims=2, seed=3):
    """n bodies with individual masses (no two on one position), shared, read-only."""
    rng = np.random.default_rng(seed)
    pos = rng.normal(0, 1, (n, dims)).astype(np.float32)
    m = rng.uniform(0.5, 2.0, n).astype(np.float32)
    pos.setflags(write=False); m.setflags(write=False)
    return pos, m


@functools.lru_cache(maxsize=None)
def probes(k, dims=2, seed=29, scale=1.5):
    """k points that lie on no body of a cloud, shared, read-only."""
    pts = np.random.default_rng(seed).normal(0, scale, (k, dims)).astype(np.float32)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def with_tracers(name="ic_plummer_1024", count=64, seed=8):
    """A fixture with `count` of its bodies made massless: (pos, m, tracer indices)."""
    pos, m, _ = gold(name)
    m = m.copy()
    tracers = np.sort(np.random.default_rng(seed).choice(pos.shape[0], count, replace=False))
    m[tracers] = 0.0
    m.setflags(write=False)
    return pos, m, tracers


def direct(bodies, eps=0.05, **kw):
    return nb.Simulation(bodies, eps=eps, device=0, **kw)


def tree_sim(bodies, eps, theta, **kw):
    kw.setdefault("tree_energy", True)
    kw.setdefault("tree_leaves", True)
    return nb.Simulation(bodies, eps=eps, theta=theta, force="tree", device=0, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def within(got, want, bar_phi, bar_acc, what):
    """got = (phi, acc) of the library, want = (phi, acc, S) of field_f64: every figure is printed before it is judged."""
    ephi = pm.rel_err(got[0], want[0])
    eacc = fm.acc_err(got[1], want[1], want[2])
    print(f"{what}: phi max relative error {ephi.max():.3g} at point {int(ephi.argmax())} (bar {bar_phi:.3g}); acc max error / S "
          f"{eacc.max():.3g} at {np.unravel_index(int(eacc.argmax()), eacc.shape)} (bar {bar_acc:.3g})")
    return bool(ephi.max() <= bar_phi and eacc.max() <= bar_acc)


def off_every_body(pts, pos):
    return not (np.asarray(pts)[:, None, :] == np.asarray(pos)[None, :, :]).all(2).any()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sweeps against the float64 sum
# ---------------------------------------------------------------------------------------------------------------------
def input_2d(n):
    if n == 333:
        return gold("ic_random_333")[:2]
    if n == 4096:
        return gold("ic_plummer_4096")[:2]
    return cloud(n)


@pytest.mark.parametrize("n,k", [(1, 65), (2, 1), (255, 63), (257, 257), (333, 1000), (1000, 63), (1000, 257), (4096, 1), (4096, 1000)])
def test_fp32_2d_against_the_fp64_sum(n, k):
    """Ragged lanes, a partial tile, two tiles and several workgroups, on both sides."""
    pos, m = input_2d(n)
    pts = probes(k)
    assert off_every_body(pts, pos)
    with direct(bodies_of(pos, m)) as sim:
        phi, acc = sim.field(pts)
    assert phi.dtype == np.float64 and phi.shape == (k,) and acc.dtype == np.float64 and acc.shape == (k, 2)
    assert within((phi, acc), fm.field_f64(pts, pos, m, 0.05), BAR_F32, BAR_ACC, f"fp32 2-D n {n} npoints {k}")


def test_fp32_2d_on_the_reference_start_with_its_central_mass():
    """default_ics_first4096 at eps = 1: body 0 weighs 1e9 and dominates every sum."""
    pos, m, _ = gold("default_ics_first4096")
    assert m[0] == 1e9
    rng = np.random.default_rng(4)
    pts = rng.uniform(pos.min(0), pos.max(0), (257, 2)).astype(np.float32)
    assert off_every_body(pts, pos)
    with direct(bodies_of(pos, m), eps=1.0) as sim:
        got = sim.field(pts)
    assert within(got, fm.field_f64(pts, pos, m, 1.0), BAR_F32, BAR_ACC, "the reference's first 4096 bodies")


@pytest.mark.parametrize("n,k", [(257, 65), (1000, 257)])
def test_fp32_3d_against_the_fp64_sum(n, k):
    pos, m = cloud(n, 3)
    pts = probes(k, 3)
    with direct(bodies_of(pos, m), dims=3) as sim:
        phi, acc = sim.field(pts)
    assert acc.shape == (k, 3) and np.abs(acc[:, 2]).min() > 0
    assert within((phi, acc), fm.field_f64(pts, pos, m, 0.05), BAR_F32, BAR_ACC, f"fp32 3-D n {n} npoints {k}")


@pytest.mark.parametrize("dims,n", [(2, 777), (3, 500)])
def test_fp64_against_the_fp64_sum(dims, n):
    pos, m = cloud(n, dims)
    pts = probes(300, dims)
    with direct(bodies_of(pos, m), precision="fp64", dims=dims) as sim:
        got = sim.field(pts)
    assert got[1].shape == (300, dims)
    assert within(got, fm.field_f64(pts, pos, m, 0.05), BAR_F64, BAR_F64, f"fp64 {dims}-D n {n}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. coverage: one massive body at j, everything else massless
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 63, 64, 255, 256, 511, 776])
def test_one_hot_mass_reaches_every_point_once(j):
    """phi = -1 / R and acc = d / R^3 of body j alone at 130 points: a dropped or doubled j is off by 100 %."""
    n, eps = 777, 0.05
    pos, _ = cloud(n)
    m = np.zeros(n, np.float32)
    m[j] = 1.0
    pts = probes(130)
    with direct(bodies_of(pos, m), eps=eps) as sim:
        got = sim.field(pts)
    d = pos[j].astype(np.float64) - pts.astype(np.float64)
    r2 = (d * d).sum(1) + pm.eps_of(eps) ** 2
    want_acc = d / r2[:, None] ** 1.5
    assert within(got, (-1.0 / np.sqrt(r2), want_acc, np.abs(want_acc)), BAR_F32, BAR_ACC, f"one-hot mass at {j}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. bit-for-bit ties to the calls that exist: the field at a massless tracer is that tracer's phi and acceleration
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(precision="fp64")], ids=["fp32", "fp64"])
def test_direct_phi_at_a_tracer_has_the_bits_of_nb_potentials(kw):
    pos, m, tracers = with_tracers()
    with direct(bodies_of(pos, m), **kw) as sim:
        want = sim.potentials()[tracers]
        got = sim.field(pos[tracers], acc=False)
    assert (want < 0).all() and same(got, want)


@pytest.mark.parametrize("quad", [False, True], ids=["mono", "quad"])
@pytest.mark.parametrize("rsqrt", ["exact", "quake"])
@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_tree_walk_at_a_tracer_has_the_bits_of_the_bodies_walks(theta, rsqrt, quad):
    """A point walks exactly as a massless body there walks: nb_potentials' phi, and nb_accelerations' float acc widened."""
    pos, m, tracers = with_tracers()
    with tree_sim(bodies_of(pos, m), 0.05, theta, rsqrt=rsqrt, tree_quadrupole=quad) as sim:
        want_acc = sim.accelerations()[tracers]
        want_phi = sim.potentials()[tracers]
        phi, acc = sim.field(pos[tracers])
        nodes = sim.tree_stats()["nodes"]
    assert nodes > 1024 and (want_phi < 0).all() and np.abs(want_acc).min() > 0
    assert same(phi, want_phi)
    assert want_acc.dtype == np.float32 and same(acc, want_acc.astype(np.float64))


def test_the_relative_test_is_not_applied_to_points():
    pos, m, _ = gold("ic_plummer_1024")
    pts = probes(257, scale=1.0)
    with tree_sim(bodies_of(pos, m), 0.05, 1.0, tree_alpha=0.02) as sim:
        assert sim.accelerations().any()                       # a_prev is there: the bodies' own walks would now open more
        loose = sim.field(pts)
        sim.set_tree_alpha(0.0)
        plain = sim.field(pts)
    assert same(loose[0], plain[0]) and same(loose[1], plain[1])
    want = fm.field_f64(pts, pos, m, 0.05)
    assert pm.rel_err(plain[0], want[0]).max() < 0.2           # the theta = 1 walk of all the bodies, not nothing


def test_tree_walk_at_theta_zero_is_the_direct_sum():
    """phi: float64 terms from the float32 leaves, the project's energy bar (1e-10, tests/test_tree_energy_gpu.py).  acc: the walker
    adds its 1024 float32 terms into ONE running sum, so the 63 roundings of a run become 1023."""
    pos, m, _ = gold("ic_plummer_1024")
    pts = probes(257, scale=1.0)
    assert off_every_body(pts, pos)
    with tree_sim(bodies_of(pos, m), 0.05, 0.0) as sim:
        got = sim.field(pts)
    assert within(got, fm.field_f64(pts, pos, m, 0.05), 1e-10, (6.5 + 1023) * 2.0 ** -24, "tree, theta 0")


def test_tree_handle_without_the_energy_flag_runs_the_direct_sweep():
    pos, m, _ = gold("ic_plummer_1024")
    pts = probes(130)
    b = bodies_of(pos, m)
    with nb.Simulation(b, eps=0.05, theta=0.5, force="tree", device=0, tree_leaves=True) as t, direct(b) as d:
        got, want = t.field(pts), d.field(pts)
    assert same(got[0], want[0]) and same(got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. what a row depends on
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [2, 3])
def test_points_per_lane_do_not_change_a_bit(dims):
    """nb_params.lanes_p forces P; 1000 points are one workgroup at P = 4, two at P = 2, four at P = 1."""
    pos, m = cloud(1000, dims)
    pts = probes(1000, dims)
    out = {}
    for p in (0, 1, 2, 4):
        with direct(bodies_of(pos, m), dims=dims, lanes_p=p) as sim:
            out[p] = sim.field(pts)
    assert within(out[4], fm.field_f64(pts, pos, m, 0.05), BAR_F32, BAR_ACC, f"{dims}-D, four point pairs per lane")
    for p in (1, 2, 4):
        assert same(out[p][0], out[0][0]) and same(out[p][1], out[0][1]), p


@pytest.mark.parametrize("dims,make", [(2, lambda b: direct(b)), (2, lambda b: direct(b, precision="fp64")), (3, lambda b: direct(b, dims=3)),
                                       (2, lambda b: tree_sim(b, 0.05, 0.5, tree_quadrupole=True))], ids=["fp32", "fp64", "fp32-3d", "tree"])
def test_a_row_depends_on_its_point_only(dims, make):
    """A permutation of the points permutes the rows; one point alone has the bits it has among 1000; either plane alone has the
    bits of the joint call and the other array keeps its sentinel; two handles agree."""
    k = 1000
    pos, m = cloud(1000, dims)
    pts = probes(k, dims)
    perm = np.random.default_rng(18).permutation(k)
    lib = nb.load()
    b = bodies_of(pos, m)
    with make(b) as sim, make(b) as twin:
        phi, acc = sim.field(pts)
        again = twin.field(pts)
        shuffled = sim.field(pts[perm])
        alone = [sim.field(pts[t:t + 1]) for t in (0, 1, 63, 64, 999)]
        only_phi, untouched_acc = np.full(k, SENTINEL), np.full((k, dims), SENTINEL)
        only_acc, untouched_phi = np.full((k, dims), SENTINEL), np.full(k, SENTINEL)
        assert lib.nb_field(sim._h, pts.ctypes.data, k, only_phi.ctypes.data, None) == L.NB_OK
        assert lib.nb_field(sim._h, pts.ctypes.data, k, None, only_acc.ctypes.data) == L.NB_OK
        assert sim.field(pts, acc=False).shape == (k,) and sim.field(pts, phi=False).shape == (k, dims)
    assert np.isfinite(phi).all() and (phi < 0).all() and np.isfinite(acc).all() and np.abs(acc).min() > 0
    assert same(again[0], phi) and same(again[1], acc)
    assert same(shuffled[0], phi[perm]) and same(shuffled[1], acc[perm])
    for t, (f, a) in zip((0, 1, 63, 64, 999), alone):
        assert same(f, phi[t:t + 1]) and same(a, acc[t:t + 1]), t
    assert same(only_phi, phi) and same(only_acc, acc)
    assert (untouched_acc == SENTINEL).all() and (untouched_phi == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. conventions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(precision="fp64")], ids=["fp32", "fp64"])
def test_a_point_on_a_body_takes_its_softened_potential_and_no_acceleration(kw):
    pos, m = cloud(1000)
    on = [0, 255, 256, 999]
    pts = np.concatenate([pos[on], probes(61)])
    eps = 0.05
    bar = (BAR_F64, BAR_F64) if kw else (BAR_F32, BAR_ACC)
    with direct(bodies_of(pos, m), eps=eps, **kw) as sim:
        got = sim.field(pts)
    want = fm.field_f64(pts, pos, m, eps)
    assert within(got, want, *bar, "points on bodies")
    for t, b in enumerate(on):                                 # the -m / eps term is there, and leaving it out would miss the bar
        term = float(m[b]) / pm.eps_of(eps)
        assert got[0][t] < -term and term > 1e3 * BAR_F32 * abs(want[0][t])


@pytest.mark.parametrize("kw", [dict(), dict(precision="fp64"), dict(dims=3)], ids=["fp32", "fp64", "fp32-3d"])
def test_without_softening_a_point_on_a_body_sees_the_other_bodies(kw):
    """eps = 0: the pair with r^2 = 0 adds nothing; the result is finite and has the bits of the field with that body massless."""
    dims = kw.get("dims", 2)
    pos, m = cloud(1000, dims)
    on = [0, 255, 256, 999]
    pts = np.concatenate([pos[on], probes(61, dims)])
    bar =(BAR_F64, BAR_F64) if "precision" in kw else (BAR_F32, BAR_ACC)
    with direct(bodies_of(pos, m), eps=0.0, **kw) as sim:
        got = sim.field(pts)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    want = fm.field_f64(pts, pos, m, 0.0)
    assert np.isfinite(want[0]).all() and within(got, want, *bar, f"eps 0 {kw}")
    for t, b in enumerate(on):                                 # one body massless at a time: the same bits at the point on it
        one = m.copy()
        one[b] = 0.0
        with direct(bodies_of(pos, one), eps=0.0, **kw) as sim:
            phi, acc = sim.field(pts[t:t + 1])
        assert same(phi, got[0][t:t + 1]) and same(acc, got[1][t:t + 1]), b


@pytest.mark.parametrize("kw", [dict(), dict(precision="fp64"), dict(dims=3)], ids=["fp32", "fp64", "fp32-3d"])
def test_sharded_handles_return_the_unsharded_bits(kw):
    dims = kw.get("dims", 2)
    pos, m = cloud(1000, dims)
    pts = probes(257, dims)
    b = bodies_of(pos, m)
    with direct(b, **kw) as one, direct(b, i_begin=300, i_count=500, **kw) as block, \
            direct(b, shard_rank=0, shard_world=1, shard_single=True, **kw) as single:
        want, got_block, got_single = one.field(pts), block.field(pts), single.field(pts)
    assert (want[0] < 0).all()
    for got in (got_block, got_single):
        assert same(got[0], want[0]) and same(got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. nothing of the handle changes; reports, refusals, destinations, profiling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda b: direct(b), lambda b: direct(b, integrator="kdk"),
                                  lambda b: tree_sim(b, 0.05, 0.5, tree_quadrupole=True)], ids=["direct", "direct-kdk", "tree-energy"])
def test_the_trajectory_does_not_notice_the_call(make):
    pos, m, vel = gold("ic_plummer_1024")
    b = bodies_of(pos, m, vel)
    pts = probes(130)
    end = []
    for call in (True, False):
        with make(b) as sim:
            sim.advance(1, 1e-3)
            before = {f: sim.sync()[f].copy() for f in ("pos", "vel", "acc")}
            assert before["acc"].any()
            if call:
                assert (sim.field(pts)[0] < 0).all()
                after = sim.sync()
                for f in ("pos", "vel", "acc"):
                    assert np.array_equal(bits(after[f]), bits(before[f])), f
                assert sim.frame == 1
            sim.advance(1, 1e-3)
            assert sim.frame == 2
            end.append({f: sim.sync()[f].copy() for f in ("pos", "vel", "acc")})
    for f in ("pos", "vel", "acc"):
        assert np.array_equal(bits(end[0][f]), bits(end[1][f])), f


def unbuildable():
    """Pairs of positions one ulp apart that no rounded child centre separates (tests/test_tree_energy_gpu.py, its failed build)."""
    n = 512
    j = np.arange(n // 2)
    pos = np.zeros((n, 2), np.float32)
    pos[0::2, 0], pos[0::2, 1] = (j % 16) - 7.25, (j // 16) - 7.25
    pos[1::2, 0], pos[1::2, 1] = np.nextafter(pos[0::2, 0], np.float32(99)), pos[0::2, 1]
    return pos, np.full(n, 1.0 / n, np.float32)


@pytest.mark.parametrize("energy", [False, True], ids=["pending-from-a-step", "this-calls-build"])
def test_a_tree_overflow_report_leaves_through_the_call_once_with_nothing_written(energy):
    pos, m = unbuildable()
    pts = probes(65)
    phi, acc = np.full(65, SENTINEL), np.full((65, 2), SENTINEL)
    with tree_sim(bodies_of(pos, m), 0.05, 1.0, tree_energy=energy) as sim:
        if not energy:
            sim.advance(1, 1e-3)                               # the failed build of a STEP; this handle's field is the direct sweep
        with pytest.raises(L.NBodyError) as e:
            sim.field(pts, out=(phi, acc))
        assert e.value.code == L.NB_ENOMEM and "not separated within 63 levels" in str(e.value)
        assert (phi == SENTINEL).all() and (acc == SENTINEL).all()
        if not energy:                                         # once: the direct sweep of the positions, which did not move
            got = sim.field(pts, out=(phi, acc))
            assert got[0] is phi and got[1] is acc and (phi < 0).all() and np.isfinite(acc).all()
        else:                                                  # reported once: the next synchronising call passes
            assert np.array_equal(sim.sync()["pos"], pos) and sim.tree_stats()["overflow_steps"] == 1


def test_refusals():
    pos, m = cloud(1000)
    lib = nb.load()
    pts = probes(65).copy()
    phi, acc = np.full(65, SENTINEL), np.full((65, 2), SENTINEL)

    def call(h, p, k, f, a):
        return lib.nb_field(h, None if p is None else p.ctypes.data, k, None if f is None else f.ctypes.data, None if a is None else a.ctypes.data)

    with direct(bodies_of(pos, m), shard_rank=0, shard_world=1, shard_single=True) as sim:
        assert call(None, pts, 65, phi, acc) == L.NB_EINVAL and b"nb_field: NULL handle" in lib.nb_last_error()
        assert call(sim._h, None, 65, phi, acc) == L.NB_EINVAL and b"nb_field: NULL points" in lib.nb_last_error()
        assert call(sim._h, pts, 65, None, None) == L.NB_EINVAL and b"phi and acc are both NULL" in lib.nb_last_error()
        assert call(sim._h, pts, 0, phi, acc) == L.NB_EINVAL and b"npoints must be 1 .. 4194304 (got 0)" in lib.nb_last_error()
        # refused by the count alone, before the array is read: one row is all there is
        assert call(sim._h, pts[:1].copy(), L.NB_FIELD_POINTS_MAX + 1, phi, acc) == L.NB_EINVAL
        assert b"npoints must be 1 .. 4194304 (got 4194305)" in lib.nb_last_error()
        with pytest.raises(L.NBodyError) as e:
            sim.field(np.zeros((0, 2), np.float32))
        assert e.value.code == L.NB_EINVAL
        for bad, where in ((np.nan, (5, 1)), (np.inf, (64, 0)), (-np.inf, (0, 0))):
            broken = pts.copy()
            broken[where] = bad
            broken[where[0] + 1:, :] = np.nan if where[0] < 64 else 0  # only the FIRST is named
            assert call(sim._h, broken, 65, phi, acc) == L.NB_EINVAL
            msg = lib.nb_last_error().decode()
            assert f"points[{2 * where[0] + where[1]}] (point {where[0]}, axis {where[1]}) is not finite" in msg, msg
        assert (phi == SENTINEL).all() and (acc == SENTINEL).all()
        # the front end names what is wrong with a shape or a dtype
        with pytest.raises(ValueError, match="points must be"):
            sim.field(np.zeros((65, 3), np.float32))
        with pytest.raises(ValueError, match="at least one of phi and acc"):
            sim.field(pts, phi=False, acc=False)
        for bad in (np.zeros(64), np.zeros(65, np.float32), np.zeros((65, 1)), np.zeros(130)[::2]):
            with pytest.raises(TypeError, match="out for phi"):
                sim.field(pts, acc=False, out=bad)
        with pytest.raises(TypeError, match="out for acc"):
            sim.field(pts, out=(np.zeros(65), np.zeros((65, 3))))
        with pytest.raises(TypeError, match="pair"):
            sim.field(pts, out=np.zeros(65))
        sim.step_begin(1e-3)
        assert call(sim._h, pts, 65, phi, acc) == L.NB_ESTATE and b"nb_field: a split step is in flight" in lib.nb_last_error()
        assert (phi == SENTINEL).all() and (acc == SENTINEL).all()
        sim.step_mid()
        sim.step_finish()
        assert call(sim._h, pts, 65, phi, acc) == L.NB_OK and (phi < 0).all() and np.isfinite(acc).all()


def test_pageable_and_page_locked_destinations_receive_the_same_bytes():
    pos, m, _ = gold("ic_plummer_4096")
    k = 1000
    pts = probes(k)
    lib = nb.load()
    ptr = lib.nb_host_alloc(k * 8 * 3)
    assert ptr
    try:
        pinned = np.frombuffer((C.c_uint8 * (k * 8 * 3)).from_address(ptr), dtype=np.float64)
        pinned[:] = SENTINEL
        pphi, pacc = pinned[:k], pinned[k:].reshape(k, 2)
        with direct(bodies_of(pos, m)) as sim:
            phi, acc = sim.field(pts)
            got = sim.field(pts, out=(pphi, pacc))
            assert got[0] is pphi and got[1] is pacc
            assert same(phi, pphi) and same(acc, pacc) and (pphi < 0).all()
            inside = np.full(k + 10, SENTINEL)                  # an unaligned pageable slice: the elements round it stay
            sim.field(pts, acc=False, out=inside[3:k + 3])
            assert same(inside[3:k + 3], phi) and (inside[:3] == SENTINEL).all() and (inside[k + 3:] == SENTINEL).all()
        del pinned, pphi, pacc, got
    finally:
        assert lib.nb_host_free(ptr) == 0


def test_a_call_counts_as_one_profiled_launch():
    pos, m, _ = gold("ic_plummer_1024")
    pts = probes(257)
    for make in (lambda b: direct(b), lambda b: direct(b, precision="fp64"), lambda b: tree_sim(b, 0.05, 0.5)):
        with make(bodies_of(pos, m)) as sim:
            sim.profile(True)
            sim.field(pts)
            ms, launches = sim.profile_read()
            assert launches == 1 and ms > 0.0
            sim.field(pts, acc=False)
            sim.field(pts, phi=False)
            assert sim.profile_read()[1] == 2
