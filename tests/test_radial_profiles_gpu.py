"""GPU: nb_radial_profiles — shell sums about many centres, against the numpy statement of the contract
(tests/radial_profiles_model.py) and closed forms.  Counts are compared for equality; every double is held to the model's bar,
(count + 8) 2^-52 times the sum of the terms' magnitudes, which is derived there and not measured."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import radial_profiles_model as rm  # noqa: E402
from test_neighbors_gpu import Pinned, bodies_of, cloud, direct  # noqa: E402  (helpers only)
from test_radial_profiles_cpu import LATTICE_SHELLS, OMEGA, assert_lattice_row, rigid_lattice  # noqa: E402  (helpers only)

pytestmark = pytest.mark.gpu
SENT = 0xAB
TAIL_EDGES = np.geomspace(0.05, 1.5, 13).astype(np.float32)              # the twelve geometric shells of tests/test_pair_counts_gpu.py
WIDE_EDGES = np.geomspace(0.25, 6.0, 13).astype(np.float32)              # twelve that hold bodies of a cloud of a few hundred
P = rm.PIECE


def moving(x, y, z=None, seed=0, mass=None):
    """bodies at (x, y[, z]) with random velocities and masses"""
    rng = np.random.default_rng(1000 + seed)
    n = len(x)
    b = bodies_of(x, y, z=z, mass=rng.uniform(0.2, 3.0, n).astype(np.float32) if mass is None else mass)
    v = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
    b["vel"][:, 0], b["vel"][:, 1] = v[:, 0], v[:, 1]
    if z is not None:
        b.view(L.BODY3_DTYPE)["vel"][:, 2] = v[:, 2]
    return b


def model_of(b, cen, edges, vc=None, dims=2):
    v = b.view(L.BODY3_DTYPE) if dims == 3 else b
    return rm.profiles(v["pos"], v["vel"], b["mass"], cen, edges, vc)


def check(sim, b, cen, edges, vc=None, dims=2, what=""):
    got = sim.radial_profiles(cen, edges, vc)
    model = model_of(b, cen, edges, vc, dims)
    assert got.dtype == L.SHELL_DTYPE and got.shape == model[0].shape, what
    print(f"{what}: worst |got - want| / bar = {rm.worst(got, model):.3g}, bodies in shells {int(model[0].sum())}")
    bad = rm.mismatches(got, model, what)
    assert not bad, "; ".join(bad)
    return got, model


def three_centres(b, dims=2):
    """on body 0, off any body, 1e6 away"""
    p = b.view(L.BODY3_DTYPE)["pos"] if dims == 3 else b["pos"]
    return np.array([p[0], [0.123, -0.321, 0.05][:dims], [1e6] * dims], np.float32)


@functools.lru_cache(maxsize=None)
def cloud_bodies(n):
    b = moving(*cloud(n), seed=n)
    b.setflags(write=False)
    return b


# ---------------------------------------------------------------------------------------------------------------------
# 1. wave and workgroup tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 4097])
def test_tails_and_the_model(n):
    b = cloud_bodies(n)
    cen = three_centres(b)
    vc = np.array([[0.3, -0.2], [0.0, 1.5], [2.0, 2.0]])
    with direct(b) as sim:
        for edges in (TAIL_EDGES, WIDE_EDGES, np.concatenate([[0], WIDE_EDGES[1:]]).astype(np.float32)):
            for v in (vc, None):
                got, model = check(sim, b, cen, edges, v, what=f"n {n}")
                assert not got[2].tobytes().strip(b"\0")                 # the far centre: every byte zero
        assert model[0][0, 0] >= 1                                       # edges[0] == 0: body 0 lies on its centre
    if n >= 1000:
        assert model[0][:2].sum(axis=1).min() > 50 and (model[0][:2].sum(axis=0) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. every shell capacity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [1, 7, 8, 9, 16, 17, 32, 33, 64])
def test_every_capacity(nbins):
    b = cloud_bodies(1500)
    cen = np.random.default_rng(nbins).uniform(-6, 6, (40, 2)).astype(np.float32)
    edges = np.geomspace(0.5, 5.0, nbins + 1).astype(np.float32)
    with direct(b) as sim:
        _, model = check(sim, b, cen, edges, what=f"nbins {nbins}")
    assert model[0].sum() > 1200 and (model[0].sum(axis=0) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the lattice: closed forms with ==, half-open shells, bodies on the centre
# ---------------------------------------------------------------------------------------------------------------------
def as_sums(rec):
    return np.stack([rec[f] for f in rm.FIELDS], axis=-1)


def test_lattice_closed_forms_half_open_shells_and_bodies_on_the_centre():
    pos, vel, mass = rigid_lattice()
    b = bodies_of(pos[:, 0], pos[:, 1], mass=mass)
    b["vel"][:, :2] = vel
    edges = [s[0] for s in LATTICE_SHELLS] + [LATTICE_SHELLS[-1][1]]
    cen = np.array([[0, 0], [3, -2]], np.float32)
    vc = np.array([[0, 0], [-OMEGA * -2, OMEGA * 3]], np.float64)        # the second centre moves with the rotation at its site
    with direct(b) as sim:
        got = sim.radial_profiles(cen, edges, vc)
        assert_lattice_row(got["count"][0], as_sums(got)[0], 0, 0, "origin")
        assert_lattice_row(got["count"][1], as_sums(got)[1], 3, -2, "site (3, -2)")
        whole = sim.radial_profiles(cen[:1], [0, 100])
        assert whole["count"][0, 0] == 256 and whole["mlz"][0, 0] == 1376.0 and whole["mass"][0, 0] == 64.0
        # d2 = 1 is in [1, 2), not in [0, 1): the four nearest sites
        assert sim.radial_profiles(cen[:1], [0, 1, 2])["count"][0].tolist() == [1, 8]
        assert sim.radial_profiles(cen[:1], [1, 2, 3])["count"][0].tolist() == [8, 16]
    # three bodies on the centre's site: in shell 0 when edges[0] == 0 (count, mass and mv2 only), in no shell otherwise
    b3 = nb.bodies_array(b.shape[0] + 2)
    b3[:-2], b3[-2:] = b, b[:2]
    b3["pos"][-2:] = 0.0
    b3["vel"][-2:, :2] = [[3.0, 4.0], [0.0, -2.0]]
    with direct(b3) as sim:
        got = sim.radial_profiles(cen[:1], [0, 1, 2])
        assert got["count"][0].tolist() == [3, 8] and got["mass"][0, 0] == 0.75 and got["mv2"][0, 0] == 0.25 * (25.0 + 4.0)
        assert [got[f][0, 0] for f in ("mr", "mr2", "mvr", "mvr2", "mlz")] == [0.0] * 5
        got = sim.radial_profiles(cen[:1], [0.5, 1, 2])
        assert got["count"][0].tolist() == [0, 8] and not got[0, 0].tobytes().strip(b"\0")


# ---------------------------------------------------------------------------------------------------------------------
# 4. a centre at a cell corner: every cell round it that can hold a body of a shell contributes
# ---------------------------------------------------------------------------------------------------------------------
def test_a_centre_at_a_cell_corner_reads_every_cell_round_it():
    """A centre 5e-4 inside a corner of its cell, last edge 1: the four cells at that corner hold most of the disc, and the four
    cells beyond the two far sides hold slivers 5e-4 wide, where bodies are put by hand.  The ninth cell, diagonally opposite, is
    more than the last edge away in both axes and can hold no body of any shell; it is read and contributes nothing."""
    rng = np.random.default_rng(4)
    h = 1.0 * (1.0 + 2.0 ** -16)
    far = h - 5e-4
    slivers = [(1.0002, 5e-4), (1.0002, -0.01), (5e-4, 1.0002), (-0.01, 1.0002),          # round the centre at the low corner
               (-0.0002, far), (-0.0002, h + 0.01), (far, -0.0002), (h + 0.01, -0.0002)]  # round the one at the high corner
    xy = np.concatenate([rng.uniform(-3, 3, (4000, 2)), slivers]).astype(np.float32)
    b = moving(xy[:, 0], xy[:, 1], seed=4)
    edges = [0, 0.3, 0.7, 0.9, 0.999, 1.0]
    with direct(b) as sim:
        for corner in ((5e-4, 5e-4), (far, far)):
            cen = np.array([corner], np.float32)
            d = xy - cen[0]
            inside = xy[d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < 1.0].astype(np.float64)
            cells = {(int(np.floor(x / h)), int(np.floor(y / h))) for x, y in inside}
            assert len(cells) == 8 and {c[0] for c in cells} == {-1, 0, 1} == {c[1] for c in cells}, (corner, cells)
            _, model = check(sim, b, cen, edges, what=f"corner {corner}")
            assert model[0].min() >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. split and unsplit centres
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded_cell():
    """5 P + 37 bodies in the cell [0, 1) x [0, 1) of a grid of last edge 0.9999, and 3000 spread over [5, 25) x [5, 25)"""
    rng = np.random.default_rng(5)
    inside = rng.uniform(0.05, 0.95, (5 * P + 37, 2))
    spread = rng.uniform(5.0, 25.0, (3000, 2))
    xy = np.concatenate([inside, spread]).astype(np.float32)
    xy = xy[rng.permutation(xy.shape[0])]
    b = moving(xy[:, 0], xy[:, 1], seed=5)
    b.setflags(write=False)
    return b


def test_one_split_centre_and_many_centres_in_its_cell():
    b = crowded_cell()
    edges = np.array([0, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9999], np.float32)
    rng = np.random.default_rng(55)
    with direct(b) as sim:
        _, model = check(sim, b, np.array([[0.5, 0.5]], np.float32), edges, what="one centre, six pieces")
        assert model[0].sum() > 4 * P
        cen = rng.uniform(0.1, 0.9, (300, 2)).astype(np.float32)
        check(sim, b, cen, edges, rng.normal(0, 1, (300, 2)), what="300 centres in the crowded cell")


def test_one_giant_centre_among_two_hundred_small_ones():
    b = crowded_cell()
    edges = np.array([0.02, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9999], np.float32)
    rng = np.random.default_rng(56)
    cen = rng.uniform(6.0, 24.0, (201, 2)).astype(np.float32)
    cen[77] = [0.4, 0.6]
    with direct(b) as sim:
        got, model = check(sim, b, cen, edges, rng.normal(0, 1, (201, 2)), what="giant among small")
        alone = sim.radial_profiles(cen[77:78], edges, None)
        again = sim.radial_profiles(cen, edges, None)
    assert model[0][77].sum() > 4 * P and 0 < np.delete(model[0], 77, axis=0).sum(axis=1).max() < P
    assert again[77].tobytes() == alone[0].tobytes()                     # a centre's row does not depend on the other centres


# ---------------------------------------------------------------------------------------------------------------------
# 6. every body a centre: nb_neighbors' counts and nb_pair_counts' histogram
# ---------------------------------------------------------------------------------------------------------------------
def test_every_body_a_centre_against_neighbors_and_pair_counts():
    b = cloud_bodies(1500)
    n = 1500
    cen = np.ascontiguousarray(b["pos"])
    with direct(b) as sim:
        for r in (0.7, 1.2):
            got = sim.radial_profiles(cen, [0, r])
            assert np.array_equal(got["count"][:, 0], sim.neighbors(r, 1, count=True)[1].astype(np.uint64) + 1), r
        for edges in (TAIL_EDGES, np.concatenate([[0], TAIL_EDGES[1:]]).astype(np.float32)):
            got = sim.radial_profiles(cen, edges)
            pairs = sim.pair_counts(edges)
            want = 2 * pairs
            if edges[0] == 0:
                want[0] += n
            assert got["count"].sum(axis=0).tolist() == want.tolist() and pairs.min() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. every kind of handle
# ---------------------------------------------------------------------------------------------------------------------
def test_fp64_handle_after_three_steps():
    b = cloud_bodies(333).copy()
    b["mass"] *= np.float32(1.0 / 333)
    cen = three_centres(b)
    with direct(b, precision="fp64") as sim:
        check(sim, b, cen, WIDE_EDGES, what="fp64 before a step")
        sim.advance(3, 1e-2)
        got = sim.radial_profiles(cen, WIDE_EDGES)
        now = sim.sync().copy()                                          # the fp64 state rounded to float
        assert not np.array_equal(now["pos"], b["pos"])
        bad = rm.mismatches(got, model_of(now, cen, WIDE_EDGES), "fp64 after three steps")
        assert not bad, "; ".join(bad)


def test_dims3_handle_with_flat_z_and_with_real_z():
    b2 = cloud_bodies(1000)
    cen2 = three_centres(b2)
    with direct(b2) as flat2:
        want = flat2.radial_profiles(cen2, WIDE_EDGES)
    b3 = b2.copy()
    b3.view(L.BODY3_DTYPE)["pos"][:, 2] = 0.0
    b3.view(L.BODY3_DTYPE)["vel"][:, 2] = 0.0
    cen3 = np.concatenate([cen2, np.zeros((3, 1), np.float32)], axis=1)
    with direct(b3, dims=3, eps=0.05) as sim:
        got, _ = check(sim, b3, cen3, WIDE_EDGES, dims=3, what="dims = 3, z = 0")
    assert got["count"].tobytes() == want["count"].tobytes()
    assert not rm.mismatches(got, model_of(b2, cen2, WIDE_EDGES), "dims = 3, z = 0, against the planar model")
    ic = nb.plummer_3d(1000, 7).copy()
    v3 = ic.view(L.BODY3_DTYPE)
    v3["vel"][:] = np.random.default_rng(7).normal(0, 0.5, (1000, 3)).astype(np.float32)
    assert np.abs(v3["pos"][:, 2]).max() > 0.5
    cen = np.concatenate([v3["pos"][:1], [[0.01, -0.02, 0.03]], [[1e6, 0, 0]]]).astype(np.float32)
    edges = np.geomspace(0.02, 1.0, 13).astype(np.float32)
    with direct(ic, dims=3, eps=0.05) as sim:
        _, model = check(sim, ic, cen, edges, np.array([[0.1, 0.2, -0.3], [0, 0, 0.5], [1, 1, 1]]), dims=3, what="dims = 3, real z")
    planar = rm.profiles(v3["pos"][:, :2], v3["vel"][:, :2], ic["mass"], cen[:, :2], edges)
    assert model[0][1].sum() > 300 and not np.array_equal(planar[0], model[0])   # the projection is another answer


def test_tree_allreduce_and_single_rank_sharded_handles():
    b = cloud_bodies(1000).copy()
    b["mass"] *= np.float32(1.0 / 1000)
    cen = three_centres(b)
    with direct(b) as plain:
        want = plain.radial_profiles(cen, WIDE_EDGES).tobytes()
    with nb.Simulation(b, eps=0.5, force="tree", theta=0.5, tree_leaves=True, device=0) as sim:
        assert sim.radial_profiles(cen, WIDE_EDGES).tobytes() == want and sim.tree_stats()["nodes"] == 0
        sim.advance(2, 1e-2)
        stats = sim.tree_stats()
        got = sim.radial_profiles(cen, WIDE_EDGES)
        assert sim.tree_stats() == stats and sim.frame == 2
        bad = rm.mismatches(got, model_of(sim.sync().copy(), cen, WIDE_EDGES), "tree handle after two steps")
        assert not bad, "; ".join(bad)
    for allreduce in (False, True):
        with nb.Simulation(b, eps=0.5, shard_rank=0, shard_world=1, shard_single=True, shard_allreduce=allreduce, device=0) as sim:
            assert sim.radial_profiles(cen, WIDE_EDGES).tobytes() == want, f"single-rank sharded handle, allreduce {allreduce}"


def test_block_handle_is_refused_with_the_reason():
    b = cloud_bodies(1000)
    lib = nb.load()
    cen = np.zeros((1, 2), np.float32)
    edges = np.array([0, 1], np.float32)
    out = np.full(64, SENT, np.uint8)
    with direct(b, i_begin=0, i_count=300) as lo, direct(b, i_begin=300, i_count=700) as hi:
        for sim, owned in ((lo, 300), (hi, 700)):
            assert lib.nb_radial_profiles(sim._h, cen.ctypes.data, None, 1, edges.ctypes.data, 1, out.ctypes.data) == L.NB_ESTATE
            text = lib.nb_last_error().decode()
            assert text.startswith("nb_radial_profiles:") and f"owns {owned} of the 1000 bodies" in text and "all n" in text, text
    assert (out == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. unusual bodies
# ---------------------------------------------------------------------------------------------------------------------
def test_massless_negative_and_nan_masses_count_and_weigh_nothing_and_a_nan_coordinate_is_in_no_shell():
    b = cloud_bodies(257).copy()
    b["mass"][::3] = 0.0
    b["mass"][1::9] = -2.0
    b["mass"][2::9] = np.nan
    cen = np.array([[0.5, 0.5]], np.float32)
    with direct(b) as sim:
        got, model = check(sim, b, cen, [0, 100], what="odd masses")
        keep = b["mass"] > 0
        assert got["count"][0, 0] == 257 and np.isfinite(as_sums(got)).all()
    heavy = b[keep]
    with direct(heavy) as sim:
        only = sim.radial_profiles(cen, [0, 100])
    assert only["count"][0, 0] == keep.sum() < 200
    assert not rm.mismatches(only, (np.array([[keep.sum()]], np.uint64),) + model[1:], "the bodies that weigh something, alone")
    c = cloud_bodies(257).copy()
    c["pos"][[3, 64, 200], 0] = [np.nan, np.inf, -np.inf]
    c["pos"][[5, 64], 1] = [np.inf, np.nan]
    with direct(c) as sim:
        got, _ = check(sim, c, cen, [0, 100], what="non-finite coordinates")
        assert got["count"][0, 0] == 253
        check(sim, c, three_centres(cloud_bodies(257)), WIDE_EDGES, what="non-finite coordinates, twelve shells")


# ---------------------------------------------------------------------------------------------------------------------
# 9. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_handles_two_calls_permuted_bodies_and_permuted_centres():
    b = crowded_cell()
    edges = np.array([0, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9999], np.float32)
    rng = np.random.default_rng(9)
    cen = np.concatenate([rng.uniform(0.1, 0.9, (3, 2)), rng.uniform(6.0, 24.0, (60, 2))]).astype(np.float32)
    vc = rng.normal(0, 1, cen.shape)
    perm, cperm = rng.permutation(b.shape[0]), rng.permutation(cen.shape[0])
    with direct(b) as one, direct(b) as two, direct(b[perm]) as shuffled:
        first = one.radial_profiles(cen, edges, vc)
        assert one.radial_profiles(cen, edges, vc).tobytes() == first.tobytes() == two.radial_profiles(cen, edges, vc).tobytes()
        other = shuffled.radial_profiles(cen, edges, vc)
        rows = one.radial_profiles(cen[cperm], edges, vc[cperm])
    model = model_of(b, cen, edges, vc)
    assert not rm.mismatches(first, model, "first handle") and not rm.mismatches(other, model, "permuted bodies")
    assert other["count"].tobytes() == first["count"].tobytes()
    assert rows.tobytes() == first[cperm].tobytes()                      # permuted centres: the rows permuted, byte for byte
    assert model[0][:3].sum(axis=1).min() > P                            # split centres among them


# ---------------------------------------------------------------------------------------------------------------------
# 10. destinations and untouched memory
# ---------------------------------------------------------------------------------------------------------------------
def test_pageable_and_page_locked_destinations_and_sentinels():
    b = cloud_bodies(1000)
    cen = three_centres(b)
    nbins = WIDE_EDGES.size - 1
    lib = nb.load()
    records = 3 * nbins
    with direct(b) as sim, Pinned((records + 2) * 16, np.uint8) as pinned:
        want = sim.radial_profiles(cen, WIDE_EDGES).tobytes()
        assert want.strip(b"\0")
        for buf in (np.empty((records + 2) * 64, np.uint8), pinned):
            buf[:] = SENT
            dst = buf[64: 64 + records * 64]
            assert lib.nb_radial_profiles(sim._h, cen.ctypes.data, None, 3, WIDE_EDGES.ctypes.data, nbins, dst.ctypes.data) == L.NB_OK
            assert dst.tobytes() == want and (buf[:64] == SENT).all() and (buf[64 + records * 64:] == SENT).all()
        out = np.zeros((3, nbins), L.SHELL_DTYPE)
        assert sim.radial_profiles(cen, WIDE_EDGES, out=out) is out and out.tobytes() == want
        with pytest.raises(TypeError):
            sim.radial_profiles(cen, WIDE_EDGES, out=np.zeros((2, nbins), L.SHELL_DTYPE))
        with pytest.raises(ValueError):
            sim.radial_profiles(cen[:, :1], WIDE_EDGES)


# ---------------------------------------------------------------------------------------------------------------------
# 11. isolation
# ---------------------------------------------------------------------------------------------------------------------
def test_the_next_step_is_the_step_of_a_handle_that_never_called():
    b = cloud_bodies(333).copy()
    b["mass"] *= np.float32(1.0 / 333)
    cen = three_centres(b)
    with direct(b) as plain, direct(b) as looked:
        plain.advance(4, 1e-2)
        want = plain.sync().copy()
        looked.advance(2, 1e-2)
        looked.radial_profiles(cen, WIDE_EDGES)
        looked.advance(1, 1e-2)
        got = looked.radial_profiles(cen, TAIL_EDGES * 3)                # no wait in between: the positions of the work enqueued so far
        assert looked.frame == 3
        bad = rm.mismatches(got, model_of(looked.sync().copy(), cen, TAIL_EDGES * 3), "behind an unfinished step")
        assert not bad, "; ".join(bad)
        looked.advance(1, 1e-2)
        have = looked.sync()
        for f in ("pos", "vel", "acc", "mass", "radius"):
            assert np.array_equal(have[f].view(np.uint32), want[f].view(np.uint32)), f"{f} differs after nb_radial_profiles"


def test_alternating_with_groups_and_pair_counts_at_other_radii():
    b = cloud_bodies(1000)
    cen = three_centres(b)
    edges = {0: WIDE_EDGES, 1: np.array([0.2, 0.7, 3.0], np.float32)}
    with direct(b) as fresh:
        want_r = {k: fresh.radial_profiles(cen, e).tobytes() for k, e in edges.items()}
    with direct(b) as fresh:
        want_p = fresh.pair_counts(TAIL_EDGES).tobytes()
        want_g = fresh.groups(0.3).tobytes()
    with direct(b) as sim:
        for k in (0, 1, 0):
            assert sim.groups(0.3).tobytes() == want_g
            assert sim.radial_profiles(cen, edges[k]).tobytes() == want_r[k], f"after groups, edges {k}"
            assert sim.pair_counts(TAIL_EDGES).tobytes() == want_p
            assert sim.radial_profiles(cen, edges[1 - k]).tobytes() == want_r[1 - k], f"after pair counts, edges {1 - k}"


# ---------------------------------------------------------------------------------------------------------------------
# 12. errors and profiling
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    b = cloud_bodies(64)
    lib = nb.load()
    out = np.full(64 * 64 * 2, SENT, np.uint8)
    big = np.zeros((1 << 20) + 1, np.float32)                            # never read past the argument checks

    def call(handle, cen, edges, vc=None, ncenters=None, nbins=None, dst=out):
        c = None if cen is None else np.ascontiguousarray(cen, np.float32)
        e = None if edges is None else np.asarray(edges, np.float32)
        v = None if vc is None else np.ascontiguousarray(vc, np.float64)
        return lib.nb_radial_profiles(handle, None if c is None else c.ctypes.data, None if v is None else v.ctypes.data,
                                      (c.size // 2 if c is not None else 1) if ncenters is None else ncenters,
                                      None if e is None else e.ctypes.data, (e.size - 1) if nbins is None else nbins,
                                      None if dst is None else dst.ctypes.data)

    def refused(needle, *args, **kw):
        assert call(kw.pop("handle", sim._h), *args, **kw) == L.NB_EINVAL, needle
        text = lib.nb_last_error().decode()
        assert text.startswith("nb_radial_profiles: ") and needle in text, text

    one = [[0.0, 0.0]]
    with direct(b) as sim:
        refused("NULL handle", one, [0, 1], handle=None)
        refused("NULL centers", None, [0, 1])
        refused("NULL edges", one, None, nbins=1)
        refused("NULL out", one, [0, 1], dst=None)
        for bad in (0, (1 << 20) + 1):
            refused(f"ncenters must be 1 .. 1048576 (got {bad})", big, [0, 1], ncenters=bad)
        for bad in (0, 65, 0xFFFFFFFF):
            refused(f"nbins must be 1 .. 64 (got {bad})", one, np.arange(66), nbins=bad)
        refused("ncenters * nbins must be at most 1048576 records (16385 * 64", big, np.arange(65), ncenters=16385)
        refused("ncenters * nbins must be at most 1048576 records (1048576 * 2", big, [0, 1, 2], ncenters=1 << 20)
        for bad in (np.nan, np.inf, -np.inf):
            refused("edges[2] is not finite", one, [0, 1, bad, 3])
        refused("edges[0] must be >= 0", one, [-0.5, 1])
        refused("strictly ascending (edges[1]", one, [0, 1, 1, 2])
        refused("strictly ascending (edges[0]", one, [3, 2])
        refused("squares of edges[0]", one, [1e-30, 2e-30])
        refused("radius * radius must be finite and > 0 in float", one, [0, 1, 1e30])
        for bad in (np.nan, np.inf, -np.inf):
            refused("centers[3] (centre 1, axis 1) is not finite", [[0, 0], [1, bad], [bad, 2]], [0, 1])
            refused("vcenters[4] (centre 2, axis 0) is not finite", [[0, 0], [1, 1], [2, 2]], [0, 1], vc=[[0, 0], [1, 1], [bad, bad]])
        refused("ncenters must be", [[np.nan, 0]], [0, np.nan], ncenters=0)    # the order of the list: the count before the edges
        refused("edges[1] is not finite", [[np.nan, 0]], [0, np.nan])           # ... and the edges before the centres
        sim.step_begin(1e-2)                                             # NB_ESTATE between nb_step_begin and nb_step_finish
        assert call(sim._h, one, [0, 1]) == L.NB_ESTATE and b"a split step is in flight" in lib.nb_last_error()
        sim.step_finish()
        assert (out == SENT).all()                                       # none of the refusals wrote anything
        assert call(sim._h, one, [-0.0, 1, 30]) == L.NB_OK               # -0 is 0
        rec = out[:128].view(L.SHELL_DTYPE)
        assert rec["count"].sum() == 64 and (out[128:] == SENT).all()    # only the ncenters x nbins records are written


def test_pending_report_leaves_through_nb_radial_profiles_once():
    import test_tree_gpu as ttg                     # the input that makes a build fail through the public interface, reused as it is
    flat = ttg.close_pairs()
    lib = nb.load()
    out = np.full(2 * 64, SENT, np.uint8)
    edges, cen = np.array([0, 0.5, 1.5], np.float32), np.zeros((1, 2), np.float32)
    with ttg.tree_sim(ttg.bodies_of(flat), eps=0.05) as sim:
        sim.advance(1, 1e-3)
        assert lib.nb_radial_profiles(sim._h, cen.ctypes.data, None, 1, edges.ctypes.data, 2, out.ctypes.data) == L.NB_ENOMEM
        text = lib.nb_last_error().decode()
        assert "frame 0" in text and "nodes" in text
        assert (out == SENT).all()                                       # nothing was written
        assert lib.nb_radial_profiles(sim._h, cen.ctypes.data, None, 1, edges.ctypes.data, 2, out.ctypes.data) == L.NB_OK   # reported once


def test_profiling_counts_the_sweep_as_one_launch():
    b = cloud_bodies(1000)
    cen = three_centres(b)
    with direct(b) as sim:
        want = sim.radial_profiles(cen, WIDE_EDGES).tobytes()            # not profiled
        sim.profile(True)
        assert sim.profile_read(reset=True)[1] == 0
        assert sim.radial_profiles(cen, WIDE_EDGES).tobytes() == want
        ms, launches = sim.profile_read(reset=False)
        assert launches == 1 and ms > 0
        sim.radial_profiles(cen[:1], [0, 1])
        assert sim.profile_read(reset=True)[1] == 2
