"""GPU: nb_pair_counts — the pair-separation histogram, against the numpy statement of the contract (tests/pair_counts_model.py) and
closed forms.  Every comparison is exact equality of all nbins counters."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import groups_model as gm  # noqa: E402
import neighbors_model as nm  # noqa: E402
import pair_counts_model as pm  # noqa: E402
from test_neighbors_gpu import bodies_of, cloud, direct, synced  # noqa: E402  (helpers only)
from test_pair_counts_cpu import lattice_closed_form, sparse_lattice  # noqa: E402  (helpers only)

pytestmark = pytest.mark.gpu
SENT = 0xABABABABABABABAB
TAIL_EDGES = np.geomspace(0.05, 1.5, 13).astype(np.float32)


def assert_counts(got, want, what=""):
    assert isinstance(got, np.ndarray) and got.dtype == np.uint64 and got.shape == np.shape(want), what
    assert got.tolist() == [int(v) for v in want], f"{what}: {got.tolist()} vs {[int(v) for v in want]}"


def check(sim, x, y, edges, rows=None, what=""):
    want = pm.pair_counts(x, y, edges, rows=rows)
    assert_counts(sim.pair_counts(edges), want, f"{what} edges {np.asarray(edges, np.float32).tolist()}")
    return want


@functools.lru_cache(maxsize=None)
def cloud_counts(n):
    """The model's answer for cloud(n) at the edges of the tails test, computed once."""
    want = pm.pair_counts(*cloud(n), TAIL_EDGES)
    want.setflags(write=False)
    return want


# ---------------------------------------------------------------------------------------------------------------------
# 1. wave and workgroup tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 4097])
def test_tails_and_the_model(n):
    x, y = cloud(n)
    want = cloud_counts(n)
    if n >= 1000:
        assert want.min() >= (6 if n == 1000 else 120)                    # no bin of the model is empty
    if n == 1:
        assert not want.any()
    with direct(bodies_of(x, y)) as sim:
        assert_counts(sim.pair_counts(TAIL_EDGES), want, f"n {n}")
        if n == 2:                                                       # and the one pair in a bin
            assert_counts(sim.pair_counts([0, 100]), [1], "n 2")


# ---------------------------------------------------------------------------------------------------------------------
# 2. every bin capacity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [1, 7, 8, 9, 16, 17, 32, 33, 64])
def test_every_capacity(nbins):
    x, y = cloud(1500)
    edges = np.geomspace(0.1, 2.0, nbins + 1).astype(np.float32)
    want = pm.pair_counts(x, y, edges)
    assert want.min() >= 5 and want.sum() == 32074
    with direct(bodies_of(x, y)) as sim:
        assert_counts(sim.pair_counts(edges), want, f"nbins {nbins}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the lattices: half-open bins, coincident bodies
# ---------------------------------------------------------------------------------------------------------------------
def test_lattices_against_the_closed_forms_and_coincident_bodies():
    lx, ly = nm.lattice()
    closed = [lattice_closed_form(16, lo * lo, hi * hi) for lo, hi in ((0, 1), (1, 2), (2, 3), (3, 5))]
    assert closed == [0, 930, 1680, 4038]
    with direct(bodies_of(lx, ly)) as sim:
        assert_counts(sim.pair_counts([0, 1, 2, 3, 5]), closed, "lattice")            # d2 = 1 in [1, 4), d2 = 25 outside
        assert_counts(sim.pair_counts([1, 2, 3, 5]), closed[1:], "lattice from 1")
    sx, sy = sparse_lattice()
    with direct(bodies_of(sx, sy)) as sim:
        assert_counts(sim.pair_counts([0, 0.8, 1.0]), [3120, 3042], "sparse lattice")
    # three bodies on one site: 3 pairs at d2 = 0, and each of the two extra bodies pairs with the site's neighbours like the first
    x, y = np.concatenate([lx, [0.0, 0.0]]).astype(np.float32), np.concatenate([ly, [0.0, 0.0]]).astype(np.float32)
    extra = [2 * sum(1 for a in range(-8, 8) for b in range(-8, 8) if (a or b) and lo * lo <= a * a + b * b < hi * hi)
             for lo, hi in ((0, 1), (1, 2), (2, 3), (3, 5))]
    assert extra == [0, 16, 32, 88]
    with direct(bodies_of(x, y)) as sim:
        want = [closed[0] + 3] + [c + e for c, e in zip(closed[1:], extra[1:])]
        assert_counts(sim.pair_counts([0, 1, 2, 3, 5]), want, "coincident, edges[0] = 0")
        assert pm.pair_counts(x, y, [0, 1, 2, 3, 5]).tolist() == want
        want = [closed[0], closed[1] + extra[1]]                         # [0.5, 1): nothing; the d2 = 0 pairs are in no bin
        assert_counts(sim.pair_counts([0.5, 1, 2]), want, "coincident, edges[0] = 0.5")


# ---------------------------------------------------------------------------------------------------------------------
# 4. cells (the placements of tests/test_neighbors_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_cells_larger_than_a_staged_chunk_and_a_stretch_nobody_needs():
    rng = np.random.default_rng(21)
    x, y = rng.uniform(-0.3, 0.3, (2, 2500)).astype(np.float32)
    edges = [0, 0.1, 0.3, 0.6, 1.0]
    with direct(bodies_of(x, y)) as sim:
        want = check(sim, x, y, edges, what="2500 in one cell")
        assert want.sum() == 2500 * 2499 // 2
    ax, ay = rng.uniform(0.1, 0.9, (2, 1500))
    bx, by = rng.uniform(0.1, 0.9, (2, 1500))
    fx, fy = rng.uniform(100.0, 130.0, 3000), rng.uniform(2.0, 9.0, 3000)
    x = np.concatenate([ax, bx, fx]).astype(np.float32)
    y = np.concatenate([ay, by + 10.0, fy]).astype(np.float32)
    perm = rng.permutation(x.size)
    x, y = x[perm], y[perm]
    with direct(bodies_of(x, y)) as sim:
        want = check(sim, x, y, [0.01, 0.1, 0.5, 1.0], what="two clumps and a stretch between")
    assert want.min() > 100


def test_cell_borders_both_signs_and_pairs_across_zero():
    r = 0.75
    g = np.arange(-4, 5) * np.float32(r)
    gx, gy = np.meshgrid(g, g)
    eps = np.float32(2.0 ** -20)
    x = np.concatenate([gx.ravel(), gx.ravel() - eps, gx.ravel() + eps, [-0.5, 0.5, -0.25, 0.25, -0.0, 0.0]]).astype(np.float32)
    y = np.concatenate([gy.ravel(), gy.ravel() + eps, gy.ravel() - eps, [0.5, -0.5, 0.25, 0.25, 0.0, -0.0]]).astype(np.float32)
    with direct(bodies_of(x, y)) as sim:
        for last in (r, float(np.nextafter(np.float32(r), np.float32(1))), 1.0, 2 * r):
            want = check(sim, x, y, [0, 2.0 ** -21, 2.0 ** -19, 0.5, last], what="borders")
            assert want[0] == 3 and want[1:].min() > 0                   # (-0, 0), (0, -0) and the lattice's (0, 0) are one position


def test_coordinates_where_the_cell_clamp_applies():
    base = np.array([1.0e9, 1.0e9 + 64, 1.0e9 + 128, 1.2e9, 1.2e9 + 128, 3.0e9, -1.0e9, -1.2e9, -1.2e9 - 128, -3.0e9], np.float32)
    gx, gy = np.meshgrid(base, base)
    x, y = np.tile(gx.ravel(), 3), np.tile(gy.ravel(), 3)                # three bodies on each of the 100 positions
    with direct(bodies_of(x, y)) as sim:
        want = check(sim, x, y, [0, 1.0], what="clamp")
        assert want.tolist() == [300]
        want = check(sim, x, y, [0, 1.0, 100.0, 200.0], what="clamp, last edge 200")
        assert want[0] == 300 and want[1] > 0 and want[2] > 0


def test_one_cell_holds_everything():
    rng = np.random.default_rng(8)
    x, y = rng.uniform(-0.3, 0.3, (2, 2048)).astype(np.float32)          # diameter 0.85 below the last edge
    with direct(bodies_of(x, y)) as sim:
        want = check(sim, x, y, [0, 0.05, 0.2, 0.5, 1.0], what="one cell")
    assert want.sum() == 2048 * 2047 // 2 and want.min() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. one counter past 2^32
# ---------------------------------------------------------------------------------------------------------------------
def test_a_counter_past_two_to_the_32():
    n = 92700
    xy = np.random.default_rng(55).uniform(0.0, 1.0, (n, 2)).astype(np.float32)
    assert xy.max() < 1.0
    with direct(bodies_of(xy[:, 0], xy[:, 1])) as sim:
        got = sim.pair_counts([0, 2])
    assert n * (n - 1) // 2 == 4296598650 > 2 ** 32
    assert_counts(got, [4296598650], "92 700 bodies in one bin")


# ---------------------------------------------------------------------------------------------------------------------
# 6. non-finite and massless bodies
# ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_bodies_are_in_no_pair_and_massless_bodies_are():
    x, y = (a.copy() for a in cloud(257))
    x[[3, 64, 200]] = [np.nan, np.inf, -np.inf]
    y[[5, 64, 256]] = [np.inf, np.nan, np.nan]
    mass = np.ones(257, np.float32)
    mass[::2] = 0.0
    with direct(bodies_of(x, y, mass=mass)) as sim:
        want = check(sim, x, y, TAIL_EDGES * 2, what="non-finite")
        assert want.sum() > 500
        assert_counts(sim.pair_counts([0, 100]), [252 * 251 // 2], "non-finite, one bin over everything")
    keep = np.isfinite(x) & np.isfinite(y)
    assert keep.sum() == 252 and np.array_equal(pm.pair_counts(x[keep], y[keep], TAIL_EDGES * 2), want)


# ---------------------------------------------------------------------------------------------------------------------
# 7. block handles
# ---------------------------------------------------------------------------------------------------------------------
def test_block_handles_count_the_pairs_of_their_lower_index_and_add_up():
    x, y = cloud(1000)
    b = bodies_of(x, y)
    whole_want = cloud_counts(1000)
    blocks = ((0, 130), (130, 333), (463, 537))
    total = np.zeros(TAIL_EDGES.size - 1, np.uint64)
    with direct(b) as whole:
        got_whole = whole.pair_counts(TAIL_EDGES)
    assert_counts(got_whole, whole_want, "whole")
    for begin, count in blocks:
        with direct(b, i_begin=begin, i_count=count) as part:
            got = part.pair_counts(TAIL_EDGES)
        assert_counts(got, pm.pair_counts(x, y, TAIL_EDGES, rows=np.arange(begin, begin + count)), f"block [{begin}, +{count})")
        assert got.sum() > 0
        total += got
    assert_counts(total, got_whole, "the blocks' sum")


# ---------------------------------------------------------------------------------------------------------------------
# 8. other kinds of handle
# ---------------------------------------------------------------------------------------------------------------------
def test_fp64_handle_equals_the_fp32_handle_of_the_rounded_bodies():
    x, y = cloud(333)
    edges = TAIL_EDGES * 2
    with direct(bodies_of(x, y), precision="fp64") as sim:
        check(sim, x, y, edges, what="fp64 before a step")
        sim.advance(3, 1e-2)
        got = sim.pair_counts(edges)
        sx, sy = synced(sim)                                             # the fp64 state rounded to float
        assert not np.array_equal(sx, x)
        assert_counts(got, pm.pair_counts(sx, sy, edges), "fp64 after three steps")
        with direct(bodies_of(sx, sy)) as rounded:
            assert_counts(rounded.pair_counts(edges), got, "fp64 against the fp32 handle of the rounded bodies")


def test_dims3_handle_is_projected_on_xy():
    ic = nb.plummer_3d(1000, 7)
    b3 = ic.view(L.BODY3_DTYPE)
    x, y, z = (np.ascontiguousarray(a) for a in (b3["pos"][:, 0], b3["pos"][:, 1], b3["pos"][:, 2]))
    assert np.abs(z).max() > 0.5
    with direct(ic, dims=3, eps=0.05) as sim:
        want = check(sim, x, y, [0, 0.02, 0.05, 0.1, 0.2], what="dims = 3")
    assert want.min() > 10


def test_tree_handle_before_any_step_and_after_three():
    x, y = cloud(333)
    edges = TAIL_EDGES * 2
    with nb.Simulation(bodies_of(x, y, mass=1.0 / 333), eps=0.5, force="tree", theta=0.5, tree_leaves=True, device=0) as sim:
        check(sim, x, y, edges, what="tree handle before any step")
        assert sim.tree_stats()["nodes"] == 0
        sim.advance(3, 1e-2)
        got = sim.pair_counts(edges)
        stats = sim.tree_stats()
        sx, sy = synced(sim)
        assert not np.array_equal(sx, x)
        assert_counts(got, pm.pair_counts(sx, sy, edges), "tree handle after three steps")
        assert sim.tree_stats() == stats and sim.frame == 3


# ---------------------------------------------------------------------------------------------------------------------
# 9. touches nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["direct", "tree", "collide"])
def test_pair_counts_leaves_the_trajectory_alone(kind):
    x, y = cloud(333)
    kw = {"tree": dict(force="tree", theta=0.5, tree_leaves=True), "collide": dict(collide=True), "direct": {}}[kind]
    b = bodies_of(x, y, mass=1.0 / 333, radius=0.2)
    b["vel"][:, 0], b["vel"][:, 1] = -0.5 * y, 0.5 * x
    edges = TAIL_EDGES * 2
    with direct(b, **kw) as plain, direct(b, **kw) as looked:
        plain.advance(4, 1e-2)
        want = plain.sync().copy()
        looked.advance(2, 1e-2)
        looked.pair_counts(edges)
        assert looked.frame == 2
        looked.advance(1, 1e-2)
        got = looked.pair_counts([0, 0.5, 2.5])                          # no wait in between: the positions of the work enqueued so far
        assert looked.frame == 3
        sx, sy = synced(looked)
        assert_counts(got, pm.pair_counts(sx, sy, [0, 0.5, 2.5]), f"{kind}: counts taken behind an unfinished step")
        looked.advance(1, 1e-2)
        have = looked.sync()
        assert looked.frame == plain.frame == 4
        for f in ("pos", "vel", "acc", "mass", "radius"):
            assert np.array_equal(have[f].view(np.uint32), want[f].view(np.uint32)), f"{kind}: {f} differs after nb_pair_counts"
        if kind == "collide":
            assert looked.collision_stats()["pairs_total"] == plain.collision_stats()["pairs_total"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 10. shared scratch
# ---------------------------------------------------------------------------------------------------------------------
def test_alternating_with_the_other_grid_queries_at_other_radii():
    x, y = cloud(1000)
    b = bodies_of(x, y)
    b["vel"][:, 0] = 0.25 * y
    edges = {0: TAIL_EDGES, 1: np.array([0.2, 0.7, 3.0], np.float32)}
    with direct(b) as fresh:
        want_p = {k: fresh.pair_counts(e) for k, e in edges.items()}
    assert_counts(want_p[0], cloud_counts(1000), "fresh handle")
    with direct(b) as fresh:
        want_c = fresh.group_catalog(0.3, 2)
    want_g = gm.groups(x, y, 0.3)
    want_n = nm.neighbors(x, y, 0.5, 5)
    with direct(b) as sim:
        for k in (0, 1, 0):
            gi, gd, gc = sim.neighbors(0.5, 5, dist2=True, count=True)
            assert np.array_equal(gi, want_n[0]) and np.array_equal(gd.view(np.uint32), want_n[1].view(np.uint32)) and np.array_equal(gc, want_n[2])
            assert_counts(sim.pair_counts(edges[k]), want_p[k], f"after neighbors, edges {k}")
            gl, gs, gn = sim.groups(0.3, size=True, ngroups=True)
            assert np.array_equal(gl, want_g[0]) and np.array_equal(gs, want_g[1]) and gn == want_g[2]
            assert_counts(sim.pair_counts(edges[1 - k]), want_p[1 - k], f"after groups, edges {1 - k}")
            assert sim.group_catalog(0.3, 2).tobytes() == want_c.tobytes()
            assert_counts(sim.pair_counts(edges[k]), want_p[k], f"after group_catalog, edges {k}")
    assert want_c.shape[0] > 10 and want_g[2] < 1000


# ---------------------------------------------------------------------------------------------------------------------
# 11. permutation, repetition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_permuting_the_bodies_leaves_the_counts(seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-500, 500, (4096, 2)).astype(np.float32)
    x, y = xy[:, 0].copy(), xy[:, 1].copy()
    edges = np.geomspace(2.0, 60.0, 11).astype(np.float32)
    perm = np.random.default_rng(100 + seed).permutation(4096)
    with direct(bodies_of(x, y)) as a, direct(bodies_of(x[perm], y[perm])) as b:
        ca, cb = a.pair_counts(edges), b.pair_counts(edges)
        again = a.pair_counts(edges)
    assert_counts(ca, pm.pair_counts(x, y, edges), "first handle")
    assert_counts(cb, ca, "permuted handle")
    assert_counts(again, ca, "second call")
    assert ca.min() > 20


# ---------------------------------------------------------------------------------------------------------------------
# 12. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x, y = cloud(64)
    lib = nb.load()
    counts = np.full(64, SENT, np.uint64)

    def call(handle, edges, nbins=None, out=counts):
        e = None if edges is None else np.asarray(edges, np.float32)
        return lib.nb_pair_counts(handle, None if e is None else e.ctypes.data, (e.size - 1) if nbins is None else nbins,
                                  None if out is None else out.ctypes.data)

    def refused(edges, needle, **kw):
        assert call(kw.pop("handle", sim._h), edges, **kw) == L.NB_EINVAL, edges
        text = lib.nb_last_error().decode()
        assert text.startswith("nb_pair_counts: ") and needle in text, text

    with direct(bodies_of(x, y)) as sim:
        refused([0, 1], "NULL handle", handle=None)
        refused(None, "NULL edges", nbins=1)
        refused([0, 1], "NULL counts", out=None)
        for nbins in (0, 65, 0xFFFFFFFF):
            refused(np.arange(66), f"nbins must be 1 .. 64 (got {nbins})", nbins=nbins)
        for bad in (np.nan, np.inf, -np.inf):
            refused([0, 1, bad, 3], "edges[2] is not finite")
        refused([np.nan, 1], "edges[0] is not finite")
        refused([-0.5, 1], "edges[0] must be >= 0")
        refused([0, 1, 1, 2], "strictly ascending (edges[1]")
        refused([0, 2, 1, 3], "strictly ascending (edges[1]")
        refused([3, 2], "strictly ascending (edges[0]")
        refused([1e-30, 2e-30], "squares of edges[0]")
        refused([0, 1e-30], "squares of edges[0]")
        refused([0, 1, 1e30], "radius * radius must be finite and > 0 in float")
        # NB_ESTATE between nb_step_begin and nb_step_finish
        sim.step_begin(1e-2)
        assert call(sim._h, [0, 1]) == L.NB_ESTATE and b"a split step is in flight" in lib.nb_last_error()
        sim.step_finish()
        assert (counts == SENT).all()                                    # none of the refusals wrote anything
        assert call(sim._h, [-0.0, 1, 30]) == L.NB_OK                    # -0 is 0
        assert counts[:2].sum() == 64 * 63 // 2 and (counts[2:] == SENT).all()      # only the nbins entries are written


def test_pending_report_leaves_through_nb_pair_counts_once():
    import test_tree_gpu as ttg                     # the input that makes a build fail through the public interface, reused as it is
    flat = ttg.close_pairs()
    x, y = flat[:, 0].copy(), flat[:, 1].copy()
    lib = nb.load()
    counts = np.full(4, SENT, np.uint64)
    edges = np.array([0, 0.5, 1.5], np.float32)
    with ttg.tree_sim(ttg.bodies_of(flat), eps=0.05) as sim:
        sim.advance(1, 1e-3)
        assert lib.nb_pair_counts(sim._h, edges.ctypes.data, 2, counts.ctypes.data) == L.NB_ENOMEM
        text = lib.nb_last_error().decode()
        assert "frame 0" in text and "nodes" in text
        assert (counts == SENT).all()                                    # nothing was written
        want = check(sim, x, y, edges, what="after the report")          # reported once: the next call succeeds (nothing was integrated)
        assert want[0] >= flat.shape[0] // 2


# ---------------------------------------------------------------------------------------------------------------------
# 13. profiling
# ---------------------------------------------------------------------------------------------------------------------
def test_profiling_counts_the_count_kernel_as_one_launch():
    x, y = cloud(1000)
    with direct(bodies_of(x, y)) as sim:
        sim.pair_counts(TAIL_EDGES)                                      # not profiled
        sim.profile(True)
        ms, launches = sim.profile_read(reset=True)
        assert launches == 0
        assert_counts(sim.pair_counts(TAIL_EDGES), cloud_counts(1000), "profiled call")
        ms, launches = sim.profile_read(reset=False)
        assert launches == 1 and ms > 0
        sim.pair_counts([0, 1])
        assert sim.profile_read(reset=True)[1] == 2
