"""GPU: nb_neighbors — the k nearest bodies within a radius, against the numpy statement of the contract (tests/neighbors_model.py).
Every comparison is exact: the indices, the bits of dist2 and the counts."""
import ctypes as C
import functools
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import neighbors_model as nm  # noqa: E402

pytestmark = pytest.mark.gpu
NO = int(nm.NO_NEIGHBOR)
SENT_I, SENT_D, SENT_C = np.uint32(0xDEADBEEF), np.float32(-77.25), np.uint32(0xFEEDF00D)


def bodies_of(x, y, z=None, mass=1.0, radius=0.0) -> np.ndarray:
    b = nb.bodies_array(len(x))
    b["pos"][:, 0], b["pos"][:, 1], b["mass"], b["radius"] = x, y, mass, radius
    if z is not None:
        b.view(L.BODY3_DTYPE)["pos"][:, 2] = z
    return b


def direct(bodies, **kw):
    kw.setdefault("eps", 0.5)
    return nb.Simulation(bodies, device=0, **kw)


def assert_rows(got, want, what=""):
    """(idx, dist2, count) of the library equal the model's, bit for bit"""
    (gi, gd, gc), (wi, wd, wc) = got, want
    assert gi.dtype == np.uint32 and gd.dtype == np.float32 and gc.dtype == np.uint32
    assert gi.shape == wi.shape and gd.shape == wd.shape and gc.shape == wc.shape, what
    bad = np.flatnonzero(gc != wc)
    assert bad.size == 0, f"{what}: {bad.size} counts differ, first rows {bad[:4].tolist()}: {gc[bad[:4]].tolist()} vs {wc[bad[:4]].tolist()}"
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} idx rows differ, first {bad[0]}: {gi[bad[0]].tolist()} vs {wi[bad[0]].tolist()}"
    bad = np.flatnonzero((gd.view(np.uint32) != wd.view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} dist2 rows differ, first {bad[0]}: {gd[bad[0]].tolist()} vs {wd[bad[0]].tolist()}"


def check(sim, x, y, radius, k, rows=None, what=""):
    got = sim.neighbors(radius, k, dist2=True, count=True)
    want = nm.neighbors(x, y, radius, k, rows=rows)
    assert_rows(got, want, f"{what} radius {radius} k {k}")
    return want


@functools.lru_cache(maxsize=None)
def cloud(n, seed=3, extent=10.0):
    """n random bodies in a square of half-width `extent`, made once and shared; the arrays are not written to."""
    xy = np.random.default_rng(seed).uniform(-extent, extent, (n, 2)).astype(np.float32)
    out = xy[:, 0].copy(), xy[:, 1].copy()
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. wave and workgroup tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
def test_wave_and_workgroup_tails(n):
    x, y = cloud(n)
    radius = 6.0 if n < 100 else 2.5                                     # a handful of neighbours at every size
    with direct(bodies_of(x, y)) as sim:
        for k in (1, 5, 8, 32):
            _, _, wc = check(sim, x, y, radius, k, what=f"n {n}")
    if n >= 63:
        assert wc.max() > 5 and wc.min() < wc.max()
    if n == 1:
        assert wc.tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties, strictness, coincident bodies
# ---------------------------------------------------------------------------------------------------------------------
def test_lattice_ties_strictness_and_coincident_bodies():
    lx, ly = nm.lattice()
    x, y = np.concatenate([lx, [0.0, 0.0]]).astype(np.float32), np.concatenate([ly, [0.0, 0.0]]).astype(np.float32)     # three bodies on (0, 0)
    site = int(np.flatnonzero((lx == 0) & (ly == 0))[0])
    with direct(bodies_of(x, y)) as sim:
        wi, wd, wc = check(sim, x, y, 5.0, 8, what="lattice")
    # the three coincident bodies see each other at d2 = 0, lowest index first, and 68 sites besides; `<=` would give 80
    assert wc[site] == wc[256] == wc[257] == 70
    assert wi[site, :2].tolist() == [256, 257] and wi[256, :2].tolist() == [site, 257] and wi[257, :2].tolist() == [site, 256]
    assert wd[site, :6].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    far = int(np.flatnonzero((lx == -4) & (ly == 3))[0])                 # (0, 0) is exactly 5 away from (-4, 3): not a neighbour
    assert wc[far] == 68 and 25.0 not in wd[far].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a dense cluster: counts far above k, every capacity of the register list
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_cluster_and_every_capacity():
    rng = np.random.default_rng(8)
    x, y = (rng.uniform(-0.3, 0.3, (2, 300)).astype(np.float32))         # diameter 0.85 < radius: everyone sees everyone
    with direct(bodies_of(x, y)) as sim:
        _, _, wc = check(sim, x, y, 1.0, 5, what="cluster")
        assert (wc == 299).all()
        for k in (1, 4, 9, 16, 17, 32):                                  # capacities 4, 4, 16, 16, 32, 32 (k = 5 above: 8)
            check(sim, x, y, 1.0, k, what="cluster")
        assert np.array_equal(sim.neighbors(1.0, 0), wc)                 # the count-only kernel


# ---------------------------------------------------------------------------------------------------------------------
# 4. everything in one cell, nothing in range
# ---------------------------------------------------------------------------------------------------------------------
def test_one_cell_and_nothing_in_range():
    x, y = cloud(500)
    with direct(bodies_of(x, y)) as sim:
        _, _, wc = check(sim, x, y, 200.0, 8, what="radius 10 x the extent")
        assert (wc == 499).all()
        spacing = 20.0 / np.sqrt(500)
        wi, wd, wc = check(sim, x, y, 1e-3 * spacing, 8, what="radius 1e-3 of the spacing")
        assert (wc == 0).all() and (wi == NO).all() and np.isposinf(wd).all()


def test_cells_larger_than_a_staged_chunk_and_a_stretch_nobody_needs():
    """The cooperative search stages 1024 candidates at a time.  2500 bodies in one cell: every range spans three chunks.  Then two
    clumps of 1500 in cell rows 0 and 10 with 3000 bodies far to the right in the rows between them, which sort between the clumps:
    the workgroup whose queries straddle the two clumps has a union that contains chunks no lane of it needs."""
    rng = np.random.default_rng(21)
    x, y = rng.uniform(-0.3, 0.3, (2, 2500)).astype(np.float32)
    with direct(bodies_of(x, y)) as sim:
        _, _, wc = check(sim, x, y, 1.0, 5, what="2500 in one cell")
        assert (wc == 2499).all()
    ax, ay = rng.uniform(0.1, 0.9, (2, 1500))
    bx, by = rng.uniform(0.1, 0.9, (2, 1500))
    fx, fy = rng.uniform(100.0, 130.0, 3000), rng.uniform(2.0, 9.0, 3000)
    x = np.concatenate([ax, bx, fx]).astype(np.float32)
    y = np.concatenate([ay, by + 10.0, fy]).astype(np.float32)
    perm = rng.permutation(x.size)
    x, y = x[perm], y[perm]
    with direct(bodies_of(x, y)) as sim:
        for k in (5, 32):
            _, _, wc = check(sim, x, y, 1.0, k, what="two clumps and a stretch between")
    assert wc.max() > 1000 and wc.min() < 32


# ---------------------------------------------------------------------------------------------------------------------
# 5. cell borders
# ---------------------------------------------------------------------------------------------------------------------
def test_cell_borders_both_signs_and_pairs_across_zero():
    r = 0.75                                                             # exact in float, and so are its multiples
    g = np.arange(-4, 5) * np.float32(r)
    gx, gy = np.meshgrid(g, g)
    eps = np.float32(2.0 ** -20)
    # the multiples of the radius themselves, each once more a hair below and a hair above, and pairs that straddle 0
    x = np.concatenate([gx.ravel(), gx.ravel() - eps, gx.ravel() + eps, [-0.5, 0.5, -0.25, 0.25, -0.0, 0.0]]).astype(np.float32)
    y = np.concatenate([gy.ravel(), gy.ravel() + eps, gy.ravel() - eps, [0.5, -0.5, 0.25, 0.25, 0.0, -0.0]]).astype(np.float32)
    with direct(bodies_of(x, y)) as sim:
        for radius in (r, 2 * r, 1.0):
            for k in (5, 32):
                _, _, wc = check(sim, x, y, radius, k, what="borders")
        assert wc.min() > 0
    # the reference's truncating keys put (-0.5, 0.5) and (0.5, -0.5) into one cell; here they are neighbours by distance alone
    a, b = 3 * 81, 3 * 81 + 1
    assert nm.neighbors(x[[a, b]], y[[a, b]], 1.5, 1)[0].tolist() == [[1], [0]]


def test_coordinates_where_the_cell_clamp_applies():
    # near 10^9 the floats are 64 apart: with radius 1 only bodies on ONE position are neighbours.  1.0e9 is below the clamp at
    # 2^30 cells, 1.2e9 and 3e9 are beyond it (every such body shares the last cell of its axis); both signs.
    base = np.array([1.0e9, 1.0e9 + 64, 1.0e9 + 128, 1.2e9, 1.2e9 + 128, 3.0e9, -1.0e9, -1.2e9, -1.2e9 - 128, -3.0e9], np.float32)
    gx, gy = np.meshgrid(base, base)
    x, y = np.tile(gx.ravel(), 3), np.tile(gy.ravel(), 3)                # three bodies on each of the 100 positions
    with direct(bodies_of(x, y)) as sim:
        wi, wd, wc = check(sim, x, y, 1.0, 5, what="clamp")
        assert (wc == 2).all() and (wd[:, :2] == 0).all() and np.isposinf(wd[:, 2:]).all()
        _, _, wc = check(sim, x, y, 100.0, 5, what="clamp, radius 100")   # now the positions 64 apart see each other
        assert wc.max() > 2


# ---------------------------------------------------------------------------------------------------------------------
# 6. non-finite bodies
# ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_bodies_have_no_neighbours_and_are_nobodys():
    x, y = (a.copy() for a in cloud(257))
    x[[3, 64, 200]] = [np.nan, np.inf, -np.inf]
    y[[5, 64, 256]] = [np.inf, np.nan, np.nan]
    with direct(bodies_of(x, y)) as sim:
        wi, wd, wc = check(sim, x, y, 2.5, 8, what="non-finite")
    bad = [3, 5, 64, 200, 256]
    assert (wc[bad] == 0).all() and (wi[bad] == NO).all() and np.isposinf(wd[bad]).all()
    assert not np.isin(wi, bad).any() and wc.max() > 5


# ---------------------------------------------------------------------------------------------------------------------
# 7. handle kinds
# ---------------------------------------------------------------------------------------------------------------------
def test_block_handle_returns_its_slice_of_the_rows():
    x, y = cloud(1000)
    b = bodies_of(x, y)
    want = nm.neighbors(x, y, 2.5, 8)
    with direct(b) as whole, direct(b, i_begin=0, i_count=300) as lo, direct(b, i_begin=300, i_count=700) as hi:
        assert_rows(whole.neighbors(2.5, 8, dist2=True, count=True), want, "whole")
        assert_rows(lo.neighbors(2.5, 8, dist2=True, count=True), tuple(a[:300] for a in want), "block [0, 300)")
        assert_rows(hi.neighbors(2.5, 8, dist2=True, count=True), tuple(a[300:] for a in want), "block [300, 1000)")
    assert (want[0][:300] >= 300).any() and (want[0][300:] < 300).any()  # the candidates are the whole replica, global indices


def synced(sim):
    b = sim.sync()
    return b["pos"][:, 0].copy(), b["pos"][:, 1].copy()


def test_fp64_handle_equals_the_fp32_handle_of_the_rounded_bodies():
    x, y = cloud(333)
    with direct(bodies_of(x, y), precision="fp64") as sim:
        check(sim, x, y, 2.5, 8, what="fp64 before a step")
        sim.advance(3, 1e-2)
        got = sim.neighbors(2.5, 8, dist2=True, count=True)
        sx, sy = synced(sim)                                             # the fp64 state rounded to float
        assert not np.array_equal(sx, x)
        assert_rows(got, nm.neighbors(sx, sy, 2.5, 8), "fp64 after three steps")
        with direct(bodies_of(sx, sy)) as rounded:
            assert_rows(got, rounded.neighbors(2.5, 8, dist2=True, count=True), "fp64 against the fp32 handle of the rounded bodies")


def test_dims3_handle_is_projected_on_xy():
    ic = nb.plummer_3d(1000, 7)
    b3 = ic.view(L.BODY3_DTYPE)
    x, y, z = (np.ascontiguousarray(a) for a in (b3["pos"][:, 0], b3["pos"][:, 1], b3["pos"][:, 2]))
    assert np.abs(z).max() > 0.5
    with direct(ic, dims=3, eps=0.05) as sim:
        _, _, wc = check(sim, x, y, 0.2, 8, what="dims = 3")
    assert wc.max() > 8


def test_tree_handle_before_any_step_and_after_three():
    x, y = cloud(333)
    with nb.Simulation(bodies_of(x, y, mass=1.0 / 333), eps=0.5, force="tree", theta=0.5, tree_leaves=True, device=0) as sim:
        check(sim, x, y, 2.5, 8, what="tree handle before any step")
        assert sim.tree_stats()["nodes"] == 0
        sim.advance(3, 1e-2)
        got = sim.neighbors(2.5, 8, dist2=True, count=True)
        stats = sim.tree_stats()
        sx, sy = synced(sim)
        assert not np.array_equal(sx, x)
        assert_rows(got, nm.neighbors(sx, sy, 2.5, 8), "tree handle after three steps")
        assert sim.tree_stats() == stats and sim.frame == 3


# ---------------------------------------------------------------------------------------------------------------------
# 8. touches nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["direct", "tree", "collide"])
def test_neighbors_leaves_the_trajectory_alone(kind):
    x, y = cloud(333)
    kw = {"tree": dict(force="tree", theta=0.5, tree_leaves=True), "collide": dict(collide=True), "direct": {}}[kind]
    b = bodies_of(x, y, mass=1.0 / 333, radius=0.2)
    b["vel"][:, 0], b["vel"][:, 1] = -0.5 * y, 0.5 * x
    with direct(b, **kw) as plain, direct(b, **kw) as looked:
        plain.advance(4, 1e-2)
        want = plain.sync().copy()
        looked.advance(2, 1e-2)
        looked.neighbors(2.5, 8, dist2=True, count=True)
        assert looked.frame == 2
        looked.advance(1, 1e-2)
        got = looked.neighbors(2.5, 5, dist2=True, count=True)           # no wait in between: the positions of the work enqueued so far
        assert looked.frame == 3
        sx, sy = synced(looked)
        assert_rows(got, nm.neighbors(sx, sy, 2.5, 5), f"{kind}: rows taken behind an unfinished step")
        looked.advance(1, 1e-2)
        have = looked.sync()
        assert looked.frame == plain.frame == 4
        for f in ("pos", "vel", "acc", "mass", "radius"):
            assert np.array_equal(have[f].view(np.uint32), want[f].view(np.uint32)), f"{kind}: {f} differs after nb_neighbors"
        if kind == "collide":
            assert looked.collision_stats()["pairs_total"] == plain.collision_stats()["pairs_total"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 9. regrow
# ---------------------------------------------------------------------------------------------------------------------
def test_k_grows_and_shrinks_on_one_handle():
    x, y = cloud(1000)
    with direct(bodies_of(x, y)) as sim:
        for k, radius in ((32, 2.5), (4, 2.5), (32, 1.0), (4, 4.0)):
            check(sim, x, y, radius, k, what="regrow")


# ---------------------------------------------------------------------------------------------------------------------
# 10. destinations
# ---------------------------------------------------------------------------------------------------------------------
class Pinned:
    """`count` 4-byte elements of `dtype` over an nb_host_alloc block."""

    def __init__(self, count, dtype):
        self.lib = nb.load()
        self.ptr = self.lib.nb_host_alloc(count * 4)
        assert self.ptr
        self.array = np.frombuffer((C.c_uint8 * (count * 4)).from_address(self.ptr), dtype=dtype)

    def __enter__(self):
        return self.array

    def __exit__(self, *exc):
        self.array = None
        assert self.lib.nb_host_free(self.ptr) == 0


def test_every_subset_of_the_destinations_pageable_and_page_locked():
    x, y = cloud(257)
    n, k = 257, 5
    wi, wd, wc = nm.neighbors(x, y, 2.5, k)
    lib = nb.load()
    with direct(bodies_of(x, y)) as sim, Pinned(n * k, np.uint32) as pi, Pinned(n * k, np.float32) as pd, Pinned(n, np.uint32) as pc:
        hi, hd, hc = np.empty(n * k, np.uint32), np.empty(n * k, np.float32), np.empty(n, np.uint32)
        for (i_, d_, c_), mask in itertools.product(((hi, hd, hc), (pi, pd, pc), (pi, hd, pc)), range(1, 8)):
            i_[:], d_[:], c_[:] = SENT_I, SENT_D, SENT_C
            args = [a.ctypes.data if mask >> bit & 1 else None for bit, a in enumerate((i_, d_, c_))]
            assert lib.nb_neighbors(sim._h, 2.5, k, *args) == L.NB_OK, (mask, lib.nb_last_error())
            assert np.array_equal(i_.reshape(n, k), wi) if mask & 1 else (i_ == SENT_I).all(), mask
            assert np.array_equal(d_.view(np.uint32).reshape(n, k), wd.view(np.uint32)) if mask & 2 else (d_ == SENT_D).all(), mask
            assert np.array_equal(c_, wc) if mask & 4 else (c_ == SENT_C).all(), mask
        # count only: k is ignored
        hc[:] = SENT_C
        assert lib.nb_neighbors(sim._h, 2.5, 0, None, None, hc.ctypes.data) == L.NB_OK and np.array_equal(hc, wc)
        hc[:] = SENT_C
        assert lib.nb_neighbors(sim._h, 2.5, 1000, None, None, hc.ctypes.data) == L.NB_OK and np.array_equal(hc, wc)


# ---------------------------------------------------------------------------------------------------------------------
# 11. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x, y = cloud(64)
    lib = nb.load()
    idx, d2, cnt = np.full(64 * 32, SENT_I, np.uint32), np.full(64 * 32, SENT_D, np.float32), np.full(64, SENT_C, np.uint32)
    pi, pd, pc = idx.ctypes.data, d2.ctypes.data, cnt.ctypes.data
    with direct(bodies_of(x, y)) as sim:
        for radius in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert lib.nb_neighbors(sim._h, radius, 5, pi, pd, pc) == L.NB_EINVAL, radius
            text = lib.nb_last_error().decode()
            assert text.startswith("nb_neighbors: radius must be finite and > 0"), text
        for radius in (1e-30, 1e30):                                     # radius * radius is 0 / infinite in float
            assert lib.nb_neighbors(sim._h, radius, 5, pi, pd, pc) == L.NB_EINVAL, radius
            assert lib.nb_last_error().decode().startswith("nb_neighbors: radius * radius must be finite and > 0 in float")
        for k in (0, 33, 0xFFFFFFFF):
            for args in ((pi, pd, pc), (pi, None, None), (None, pd, None)):
                assert lib.nb_neighbors(sim._h, 1.0, k, *args) == L.NB_EINVAL, k
                assert lib.nb_last_error().decode().startswith("nb_neighbors: k must be 1 .. 32"), k
        assert lib.nb_neighbors(sim._h, 1.0, 5, None, None, None) == L.NB_EINVAL and b"idx, dist2 and count are all NULL" in lib.nb_last_error()
        assert lib.nb_neighbors(None, 1.0, 5, pi, pd, pc) == L.NB_EINVAL and b"NULL handle" in lib.nb_last_error()
        with pytest.raises(ValueError, match="neighbors: k must be"):
            sim.neighbors(1.0, 33)
        # NB_ESTATE between nb_step_begin and nb_step_finish
        sim.step_begin(1e-2)
        assert lib.nb_neighbors(sim._h, 1.0, 5, pi, pd, pc) == L.NB_ESTATE and b"a split step is in flight" in lib.nb_last_error()
        sim.step_finish()
        assert (idx == SENT_I).all() and (d2 == SENT_D).all() and (cnt == SENT_C).all()      # none of the refusals wrote anything
        assert lib.nb_neighbors(sim._h, 1.0, 5, pi, pd, pc) == L.NB_OK


# ---------------------------------------------------------------------------------------------------------------------
# 12. pending report
# ---------------------------------------------------------------------------------------------------------------------
def test_pending_report_leaves_through_nb_neighbors_once():
    import test_tree_gpu as ttg                     # the input that makes a build fail through the public interface, reused as it is
    flat = ttg.close_pairs()
    x, y = flat[:, 0].copy(), flat[:, 1].copy()
    n, k = flat.shape[0], 5
    lib = nb.load()
    idx, d2, cnt = np.full(n * k, SENT_I, np.uint32), np.full(n * k, SENT_D, np.float32), np.full(n, SENT_C, np.uint32)
    with ttg.tree_sim(ttg.bodies_of(flat), eps=0.05) as sim:
        sim.advance(1, 1e-3)
        assert lib.nb_neighbors(sim._h, 1.5, k, idx.ctypes.data, d2.ctypes.data, cnt.ctypes.data) == L.NB_ENOMEM
        text = lib.nb_last_error().decode()
        assert "frame 0" in text and "nodes" in text
        assert (idx == SENT_I).all() and (d2 == SENT_D).all() and (cnt == SENT_C).all()       # nothing was written
        check(sim, x, y, 1.5, k, what="after the report")                # reported once: the next call succeeds (nothing was integrated)


# ---------------------------------------------------------------------------------------------------------------------
# 13. permutation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_permuting_the_bodies_permutes_the_rows_and_relabels_the_indices(seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-500, 500, (4096, 2)).astype(np.float32)
    x, y = xy[:, 0].copy(), xy[:, 1].copy()
    n, k, radius = 4096, 8, 40.0
    perm = np.random.default_rng(100 + seed).permutation(n)             # body perm[q] of the first handle is body q of the second
    with direct(bodies_of(x, y)) as a, direct(bodies_of(x[perm], y[perm])) as b:
        ia, da, ca = a.neighbors(radius, k, dist2=True, count=True)
        ib, db, cb = b.neighbors(radius, k, dist2=True, count=True)
    assert_rows((ia, da, ca), nm.neighbors(x, y, radius, k), "first handle")
    # rows where a kept entry or the first one left out ties in d2 with its neighbour in the order may differ: from the k + 1 nearest
    _, d9, _ = nm.neighbors(x, y, radius, k + 1)
    tied = ((d9[:, 1:] == d9[:, :-1]) & np.isfinite(d9[:, 1:])).any(axis=1)
    assert tied.mean() <= 0.01, f"{int(tied.sum())} rows with ties: the cap is a condition of the test"
    back = np.where(ib == NO, ib, perm[np.minimum(ib, n - 1)].astype(np.uint32))         # second handle's indices as the first one's
    rows_b = np.empty(n, np.int64)
    rows_b[perm] = np.arange(n)                                          # body i of the first handle is row rows_b[i] of the second
    keep = ~tied
    assert np.array_equal(cb[rows_b], ca)                                # the counts do not depend on ties
    assert np.array_equal(back[rows_b][keep], ia[keep])
    assert np.array_equal(db[rows_b][keep].view(np.uint32), da[keep].view(np.uint32))
    assert 15 < ca.mean() < 25 and (ca > k).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------------
# 14. one larger case: the reference's own MAX_DISTANCE and MAX_CONNECTIONS on its own initial conditions
# ---------------------------------------------------------------------------------------------------------------------
def test_default_ics_with_the_references_distance_and_connections():
    ic = nb.default_ics(12000)
    x, y = ic["pos"][:, 0].copy(), ic["pos"][:, 1].copy()
    with direct(ic, eps=1.0) as sim:
        _, _, wc = check(sim, x, y, 1000.0, 5, what="default_ics")
    assert wc.max() > 5
