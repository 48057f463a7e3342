"""GPU: nb_groups — the friends-of-friends groups of the bodies, against the numpy statement of the contract (tests/groups_model.py).
Every comparison is exact integer equality: the labels, the sizes and the number of groups."""
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
import groups_model as gm  # noqa: E402
import neighbors_model as nm  # noqa: E402
from test_neighbors_gpu import Pinned, bodies_of, cloud, direct, synced  # noqa: E402  (helpers only)

pytestmark = pytest.mark.gpu
SENT_L, SENT_S, SENT_N = np.uint32(0xDEADBEEF), np.uint32(0xFEEDF00D), 0x0123456789ABCDEF


def assert_groups(got, want, what=""):
    """(label, size, ngroups) of the library equal the model's"""
    (gl, gs, gn), (wl, ws, wn) = got, want
    assert gl.dtype == np.uint32 and gs.dtype == np.uint32 and isinstance(gn, int)
    assert gl.shape == wl.shape and gs.shape == ws.shape, what
    bad = np.flatnonzero(gl != wl)
    assert bad.size == 0, f"{what}: {bad.size} labels differ, first bodies {bad[:4].tolist()}: {gl[bad[:4]].tolist()} vs {wl[bad[:4]].tolist()}"
    bad = np.flatnonzero(gs != ws)
    assert bad.size == 0, f"{what}: {bad.size} sizes differ, first bodies {bad[:4].tolist()}: {gs[bad[:4]].tolist()} vs {ws[bad[:4]].tolist()}"
    assert gn == wn, f"{what}: ngroups {gn} vs {wn}"


def check(sim, x, y, radius, rows=None, what=""):
    want = gm.groups(x, y, radius, rows=rows)
    assert_groups(sim.groups(radius, size=True, ngroups=True), want, f"{what} radius {radius}")
    return want


def mix_of(label, size):
    """(groups of two or more, singletons, largest group) of a whole partition"""
    roots = label == np.arange(label.size)
    return int((size[roots] >= 2).sum()), int((size[roots] == 1).sum()), int(size.max())


@functools.lru_cache(maxsize=None)
def cloud_groups(n):
    """The model's answer for cloud(n) at the radius of the tails test (a mean of 1.2 neighbours), computed once."""
    x, y = cloud(n)
    radius = float(np.float32(np.sqrt(1.2 * 400.0 / (n * np.pi))))
    label, size, ng = gm.groups(x, y, radius)
    for a in (label, size):
        a.setflags(write=False)
    return radius, label, size, ng


# ---------------------------------------------------------------------------------------------------------------------
# 1. wave and workgroup tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_wave_and_workgroup_tails(n):
    x, y = cloud(n)
    radius, wl, ws, wn = cloud_groups(n)
    multi, single, largest = mix_of(wl, ws)
    if n >= 255:                                                         # no trivial partition
        assert multi >= 20 and single >= 20 and largest <= n // 2, (multi, single, largest)
    elif n >= 63:                                                        # 65 bodies cannot hold 20 + 20 of them at any radius of this cloud
        assert multi >= 15 and single >= 20 and largest <= n // 2, (multi, single, largest)
    with direct(bodies_of(x, y)) as sim:
        assert_groups(sim.groups(radius, size=True, ngroups=True), (wl, ws, wn), f"n {n}")
        if n == 2:                                                       # and both bodies in one group
            assert_groups(sim.groups(100.0, size=True, ngroups=True), (np.zeros(2, np.uint32), np.full(2, 2, np.uint32), 1), "n 2, linked")


# ---------------------------------------------------------------------------------------------------------------------
# 2. strictness on the integer lattice
# ---------------------------------------------------------------------------------------------------------------------
def test_lattice_strictness_and_coincident_bodies():
    lx, ly = nm.lattice()
    with direct(bodies_of(lx, ly)) as sim:
        wl, ws, wn = check(sim, lx, ly, 1.0, what="lattice")
        assert wn == 256 and (ws == 1).all() and np.array_equal(wl, np.arange(256))     # d2 = 1 is not < 1
        wl, ws, wn = check(sim, lx, ly, float(np.nextafter(np.float32(1), np.float32(2))), what="lattice")
        assert wn == 1 and (wl == 0).all() and (ws == 256).all()
        wl, ws, wn = check(sim, lx, ly, 1.5, what="lattice")
        assert wn == 1 and (wl == 0).all()
    colour = (lx + ly) % 2 == 0                                           # one colour of the checkerboard: the diagonals alone
    cx, cy = lx[colour], ly[colour]
    with direct(bodies_of(cx, cy)) as sim:
        wl, ws, wn = check(sim, cx, cy, 1.5, what="checkerboard")
        assert wn == 1 and (ws == 128).all()
        assert check(sim, cx, cy, 1.25, what="checkerboard")[2] == 128
    # three bodies on one site: linked at d2 = 0 whatever the radius
    x, y = np.concatenate([lx, [0.0, 0.0]]).astype(np.float32), np.concatenate([ly, [0.0, 0.0]]).astype(np.float32)
    site = int(np.flatnonzero((lx == 0) & (ly == 0))[0])
    with direct(bodies_of(x, y)) as sim:
        wl, ws, wn = check(sim, x, y, 1.0, what="coincident")
        assert wn == 256 and wl[[site, 256, 257]].tolist() == [site] * 3 and ws[[site, 256, 257]].tolist() == [3] * 3 and (ws == 1).sum() == 255
        check(sim, x, y, 1e-3, what="coincident, tiny radius")


# ---------------------------------------------------------------------------------------------------------------------
# 3. long chains: a propagation that needs k - 1 rounds, or a union-find that can cycle, shows here
# ---------------------------------------------------------------------------------------------------------------------
def test_long_chains_along_an_axis_and_along_the_diagonal():
    n, radius = 3000, 1.0
    perm = np.random.default_rng(17).permutation(n)                      # body perm[t] sits at place t of the chain
    t = np.empty(n, np.float32)
    t[perm] = np.arange(n) - 1500.0                                      # both sides of zero
    x, y = t * np.float32(0.75), np.full(n, 0.3, np.float32)
    with direct(bodies_of(x, y)) as sim:
        wl, ws, wn = check(sim, x, y, radius, what="chain")
        assert wn == 1 and (wl == 0).all() and (ws == n).all()
    x2 = x.copy()
    x2[perm[1500]], y2 = 5000.0, y.copy()                                # the middle body moved away: two pieces and itself
    with direct(bodies_of(x2, y2)) as sim:
        wl, ws, wn = check(sim, x2, y2, radius, what="broken chain")
        assert wn == 3 and sorted(set(ws.tolist())) == [1, 1499, 1500]
        assert wl[perm[0]] == perm[:1500].min() and wl[perm[2999]] == perm[1501:].min()
    dx = t * np.float32(0.7)                                             # 0.99 radius per link, across cell corners
    for sx, sy in ((dx, dx), (dx, -dx), (dx - 3000.0, dx - 3000.0)):
        with direct(bodies_of(sx, sy)) as sim:
            wl, ws, wn = check(sim, sx, sy, radius, what="diagonal chain")
            assert wn == 1 and (wl == 0).all() and (ws == n).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. contention
# ---------------------------------------------------------------------------------------------------------------------
def test_everyone_in_one_cell_races_for_one_root():
    rng = np.random.default_rng(8)
    x, y = rng.uniform(-0.3, 0.3, (2, 2048)).astype(np.float32)          # diameter 0.85 < radius: everyone is linked to everyone
    with direct(bodies_of(x, y)) as sim:
        label, size, ng = sim.groups(1.0, size=True, ngroups=True)
    assert (label == 0).all() and (size == 2048).all() and ng == 1


def test_many_tight_clumps_far_apart():
    rng = np.random.default_rng(9)
    cx, cy = np.meshgrid(np.arange(32) * 10.0 - 155.0, np.arange(16) * 10.0 - 75.0)
    x = (np.repeat(cx.ravel(), 4) + rng.uniform(-0.1, 0.1, 2048)).astype(np.float32)
    y = (np.repeat(cy.ravel(), 4) + rng.uniform(-0.1, 0.1, 2048)).astype(np.float32)
    perm = rng.permutation(2048)
    x, y = x[perm], y[perm]
    with direct(bodies_of(x, y)) as sim:
        wl, ws, wn = check(sim, x, y, 1.0, what="clumps")
    assert wn == 512 and (ws == 4).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. cell borders and the clamp (the placements of tests/test_neighbors_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_cell_borders_both_signs_and_pairs_across_zero():
    r = 0.75
    g = np.arange(-4, 5) * np.float32(r)
    gx, gy = np.meshgrid(g, g)
    eps = np.float32(2.0 ** -20)
    x = np.concatenate([gx.ravel(), gx.ravel() - eps, gx.ravel() + eps, [-0.5, 0.5, -0.25, 0.25, -0.0, 0.0]]).astype(np.float32)
    y = np.concatenate([gy.ravel(), gy.ravel() + eps, gy.ravel() - eps, [0.5, -0.5, 0.25, 0.25, 0.0, -0.0]]).astype(np.float32)
    seen = set()
    with direct(bodies_of(x, y)) as sim:
        for radius in (2.0 ** -21, 2.0 ** -19, 0.5, r, float(np.nextafter(np.float32(r), np.float32(1))), 1.0, 2 * r):
            seen.add(check(sim, x, y, radius, what="borders")[2])
    assert len(seen) >= 3 and 1 in seen                                   # the partition really changes across these radii


def test_coordinates_where_the_cell_clamp_applies():
    base = np.array([1.0e9, 1.0e9 + 64, 1.0e9 + 128, 1.2e9, 1.2e9 + 128, 3.0e9, -1.0e9, -1.2e9, -1.2e9 - 128, -3.0e9], np.float32)
    gx, gy = np.meshgrid(base, base)
    x, y = np.tile(gx.ravel(), 3), np.tile(gy.ravel(), 3)                # three bodies on each of the 100 positions
    with direct(bodies_of(x, y)) as sim:
        wl, ws, wn = check(sim, x, y, 1.0, what="clamp")
        assert wn == 100 and (ws == 3).all()
        wl, ws, wn = check(sim, x, y, 100.0, what="clamp, radius 100")   # now the positions 64 apart are linked
        assert wn < 100 and ws.max() > 3


# ---------------------------------------------------------------------------------------------------------------------
# 6. non-finite bodies
# ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_bodies_are_singletons_labelled_with_themselves():
    x, y = (a.copy() for a in cloud(257))
    x[[3, 64, 200]] = [np.nan, np.inf, -np.inf]
    y[[5, 64, 256]] = [np.inf, np.nan, np.nan]
    bad = [3, 5, 64, 200, 256]
    with direct(bodies_of(x, y)) as sim:
        wl, ws, wn = check(sim, x, y, 1.5, what="non-finite")
        assert wl[bad].tolist() == bad and (ws[bad] == 1).all() and ws.max() > 5
        wl, ws, wn = check(sim, x, y, 100.0, what="non-finite, radius over everything")
        assert wn == 6 and wl[bad].tolist() == bad and (np.delete(ws, bad) == 252).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. handle kinds
# ---------------------------------------------------------------------------------------------------------------------
def test_block_handle_returns_its_slice_with_ngroups_of_all():
    x, y = cloud(1000)
    radius, wl, ws, wn = cloud_groups(1000)
    b = bodies_of(x, y)
    with direct(b) as whole, direct(b, i_begin=0, i_count=300) as lo, direct(b, i_begin=300, i_count=700) as hi:
        assert_groups(whole.groups(radius, size=True, ngroups=True), (wl, ws, wn), "whole")
        assert_groups(lo.groups(radius, size=True, ngroups=True), (wl[:300], ws[:300], wn), "block [0, 300)")
        assert_groups(hi.groups(radius, size=True, ngroups=True), (wl[300:], ws[300:], wn), "block [300, 1000)")
    assert (wl[300:] < 300).any()                                         # labels are global indices: groups reach across the blocks


def test_fp64_handle_equals_the_fp32_handle_of_the_rounded_bodies():
    x, y = cloud(333)
    with direct(bodies_of(x, y), precision="fp64") as sim:
        check(sim, x, y, 0.8, what="fp64 before a step")
        sim.advance(3, 1e-2)
        got = sim.groups(0.8, size=True, ngroups=True)
        sx, sy = synced(sim)                                             # the fp64 state rounded to float
        assert not np.array_equal(sx, x)
        assert_groups(got, gm.groups(sx, sy, 0.8), "fp64 after three steps")
        with direct(bodies_of(sx, sy)) as rounded:
            assert_groups(got, rounded.groups(0.8, size=True, ngroups=True), "fp64 against the fp32 handle of the rounded bodies")


def test_dims3_handle_is_projected_on_xy():
    ic = nb.plummer_3d(1000, 7)
    b3 = ic.view(L.BODY3_DTYPE)
    x, y, z = (np.ascontiguousarray(a) for a in (b3["pos"][:, 0], b3["pos"][:, 1], b3["pos"][:, 2]))
    assert np.abs(z).max() > 0.5
    with direct(ic, dims=3, eps=0.05) as sim:
        wl, ws, wn = check(sim, x, y, 0.06, what="dims = 3")
    assert 20 < wn < 980 and ws.max() > 8


def test_tree_handle_before_any_step_and_after_three():
    x, y = cloud(333)
    with nb.Simulation(bodies_of(x, y, mass=1.0 / 333), eps=0.5, force="tree", theta=0.5, tree_leaves=True, device=0) as sim:
        check(sim, x, y, 0.8, what="tree handle before any step")
        assert sim.tree_stats()["nodes"] == 0
        sim.advance(3, 1e-2)
        got = sim.groups(0.8, size=True, ngroups=True)
        stats = sim.tree_stats()
        sx, sy = synced(sim)
        assert not np.array_equal(sx, x)
        assert_groups(got, gm.groups(sx, sy, 0.8), "tree handle after three steps")
        assert sim.tree_stats() == stats and sim.frame == 3


# ---------------------------------------------------------------------------------------------------------------------
# 8. against nb_neighbors on the same handle
# ---------------------------------------------------------------------------------------------------------------------
def test_cross_check_against_nb_neighbors():
    x, y = cloud(4097)
    radius = cloud_groups(4097)[0]
    with direct(bodies_of(x, y)) as sim:
        label, size = sim.groups(radius, size=True)
        idx, count = sim.neighbors(radius, 4, count=True)
    assert np.array_equal(count == 0, size == 1)
    linked = np.flatnonzero(count > 0)
    assert linked.size > 1000 and np.array_equal(label[idx[linked, 0]], label[linked])


# ---------------------------------------------------------------------------------------------------------------------
# 9. touches nothing; shares its scratch with nb_neighbors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["direct", "tree"])
def test_groups_leaves_the_trajectory_alone(kind):
    x, y = cloud(333)
    kw = {"tree": dict(force="tree", theta=0.5, tree_leaves=True), "direct": {}}[kind]
    b = bodies_of(x, y, mass=1.0 / 333, radius=0.2)
    b["vel"][:, 0], b["vel"][:, 1] = -0.5 * y, 0.5 * x
    with direct(b, **kw) as plain, direct(b, **kw) as looked:
        plain.advance(4, 1e-2)
        want = plain.sync().copy()
        looked.advance(2, 1e-2)
        looked.groups(0.8, size=True, ngroups=True)
        assert looked.frame == 2
        looked.advance(1, 1e-2)
        got = looked.groups(0.9, size=True, ngroups=True)                # no wait in between: the positions of the work enqueued so far
        assert looked.frame == 3
        sx, sy = synced(looked)
        assert_groups(got, gm.groups(sx, sy, 0.9), f"{kind}: groups taken behind an unfinished step")
        looked.advance(1, 1e-2)
        have = looked.sync()
        assert looked.frame == plain.frame == 4
        for f in ("pos", "vel", "acc", "mass", "radius"):
            assert np.array_equal(have[f].view(np.uint32), want[f].view(np.uint32)), f"{kind}: {f} differs after nb_groups"


def test_alternating_with_nb_neighbors_at_other_radii():
    x, y = cloud(1000)
    want_g = {r: gm.groups(x, y, r) for r in (0.3, 0.9)}
    want_n = {r: nm.neighbors(x, y, r, 5) for r in (0.5, 1.5)}
    with direct(bodies_of(x, y)) as sim:
        for rg, rn in ((0.3, 1.5), (0.9, 0.5), (0.3, 0.5)):
            assert_groups(sim.groups(rg, size=True, ngroups=True), want_g[rg], f"groups at {rg}")
            gi, gd, gc = sim.neighbors(rn, 5, dist2=True, count=True)
            wi, wd, wc = want_n[rn]
            assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gc, wc), rn
    assert want_g[0.3][2] != want_g[0.9][2]


# ---------------------------------------------------------------------------------------------------------------------
# 10. destinations
# ---------------------------------------------------------------------------------------------------------------------
def test_every_subset_of_the_destinations_pageable_and_page_locked():
    n = 257
    x, y = cloud(n)
    radius, wl, ws, wn = cloud_groups(n)
    lib = nb.load()
    with direct(bodies_of(x, y)) as sim, Pinned(n, np.uint32) as pl, Pinned(n, np.uint32) as ps:
        hl, hs = np.empty(n, np.uint32), np.empty(n, np.uint32)
        for (l_, s_), mask in itertools.product(((hl, hs), (pl, ps), (pl, hs)), range(1, 8)):
            l_[:], s_[:] = SENT_L, SENT_S
            count = C.c_uint64(SENT_N)
            args = [l_.ctypes.data if mask & 1 else None, s_.ctypes.data if mask & 2 else None, C.byref(count) if mask & 4 else None]
            assert lib.nb_groups(sim._h, radius, *args) == L.NB_OK, (mask, lib.nb_last_error())
            assert np.array_equal(l_, wl) if mask & 1 else (l_ == SENT_L).all(), mask
            assert np.array_equal(s_, ws) if mask & 2 else (s_ == SENT_S).all(), mask
            assert count.value == (wn if mask & 4 else SENT_N), mask


# ---------------------------------------------------------------------------------------------------------------------
# 11. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x, y = cloud(64)
    lib = nb.load()
    label, size, count = np.full(64, SENT_L, np.uint32), np.full(64, SENT_S, np.uint32), C.c_uint64(SENT_N)
    pl, ps, pn = label.ctypes.data, size.ctypes.data, C.byref(count)
    with direct(bodies_of(x, y)) as sim:
        for radius in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert lib.nb_groups(sim._h, radius, pl, ps, pn) == L.NB_EINVAL, radius
            text = lib.nb_last_error().decode()
            assert text.startswith("nb_groups: radius must be finite and > 0"), text
        for radius in (1e-30, 1e30):                                     # radius * radius is 0 / infinite in float
            assert lib.nb_groups(sim._h, radius, pl, ps, pn) == L.NB_EINVAL, radius
            assert lib.nb_last_error().decode().startswith("nb_groups: radius * radius must be finite and > 0 in float")
        assert lib.nb_groups(sim._h, 1.0, None, None, None) == L.NB_EINVAL and b"label, size and ngroups are all NULL" in lib.nb_last_error()
        assert lib.nb_groups(None, 1.0, pl, ps, pn) == L.NB_EINVAL and b"NULL handle" in lib.nb_last_error()
        # NB_ESTATE between nb_step_begin and nb_step_finish
        sim.step_begin(1e-2)
        assert lib.nb_groups(sim._h, 1.0, pl, ps, pn) == L.NB_ESTATE and b"a split step is in flight" in lib.nb_last_error()
        sim.step_finish()
        assert (label == SENT_L).all() and (size == SENT_S).all() and count.value == SENT_N      # none of the refusals wrote anything
        assert lib.nb_groups(sim._h, 1.0, pl, ps, pn) == L.NB_OK and count.value <= 64


def test_pending_report_leaves_through_nb_groups_once():
    import test_tree_gpu as ttg                     # the input that makes a build fail through the public interface, reused as it is
    flat = ttg.close_pairs()
    x, y = flat[:, 0].copy(), flat[:, 1].copy()
    n = flat.shape[0]
    lib = nb.load()
    label, size, count = np.full(n, SENT_L, np.uint32), np.full(n, SENT_S, np.uint32), C.c_uint64(SENT_N)
    with ttg.tree_sim(ttg.bodies_of(flat), eps=0.05) as sim:
        sim.advance(1, 1e-3)
        assert lib.nb_groups(sim._h, 0.5, label.ctypes.data, size.ctypes.data, C.byref(count)) == L.NB_ENOMEM
        text = lib.nb_last_error().decode()
        assert "frame 0" in text and "nodes" in text
        assert (label == SENT_L).all() and (size == SENT_S).all() and count.value == SENT_N     # nothing was written
        wl, ws, wn = check(sim, x, y, 0.5, what="after the report")      # reported once: the next call succeeds (nothing was integrated)
        assert wn == n // 2 and (ws == 2).all()


# ---------------------------------------------------------------------------------------------------------------------
# 12. permutation
# ---------------------------------------------------------------------------------------------------------------------
def test_permuting_the_bodies_permutes_the_partition():
    n = 4097
    x, y = cloud(n)
    radius, wl, ws, wn = cloud_groups(n)
    perm = np.random.default_rng(101).permutation(n)                     # body perm[q] of the first handle is body q of the second
    with direct(bodies_of(x, y)) as a, direct(bodies_of(x[perm], y[perm])) as b:
        la, sa, na = a.groups(radius, size=True, ngroups=True)
        lb, sb, nb_ = b.groups(radius, size=True, ngroups=True)
    assert_groups((la, sa, na), (wl, ws, wn), "first handle")
    new = np.empty(n, np.int64)
    new[perm] = np.arange(n)                                             # body i of the first handle is body new[i] of the second
    assert na == nb_ and np.array_equal(sb[new], sa)
    # the same partition: bodies share a label in one handle exactly where they do in the other ...
    assert len(set(zip(la.tolist(), lb[new].tolist()))) == na == len(set(la.tolist())) == len(set(lb.tolist()))
    # ... and each label is the smallest NEW index of its group
    smallest = np.full(n, n, np.int64)
    np.minimum.at(smallest, la, new)
    assert np.array_equal(lb[new], smallest[la])


# ---------------------------------------------------------------------------------------------------------------------
# 13. the reference's own start at the reference's MAX_DISTANCE
# ---------------------------------------------------------------------------------------------------------------------
def test_default_ics_at_the_references_max_distance():
    ic = nb.default_ics(25000)
    x, y = ic["pos"][:, 0].copy(), ic["pos"][:, 1].copy()
    with direct(ic, eps=1.0) as sim:
        wl, ws, wn = check(sim, x, y, 1000.0, what="default_ics")
    assert 1000 < wn < 24000 and ws.max() > 1000
