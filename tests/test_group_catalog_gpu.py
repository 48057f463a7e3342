"""GPU: nb_group_catalog — mass, centre, motion, dispersion and radius of every friends-of-friends group, against the numpy statement
of the contract (tests/group_catalog_model.py).  In every test label and members are compared by exact equality with the model and with
sim.groups(radius, size=True) on the same handle; the doubles are compared within the model's bounds, none of which is measured."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import group_catalog_model as cm  # noqa: E402
import groups_model as gm  # noqa: E402
import neighbors_model as nm  # noqa: E402
from test_groups_gpu import cloud_groups  # noqa: E402  (helper only: the model's groups of cloud(n), computed once)
from test_neighbors_gpu import Pinned, bodies_of, cloud, direct  # noqa: E402  (helpers only)

pytestmark = pytest.mark.gpu
SENT = 0xA5


def dressed(x, y, seed=1):
    """Bodies at (x, y) with individual masses from uniform(0.5, 2) and velocities (-0.5 y, 0.5 x) plus noise."""
    rng = np.random.default_rng(seed)
    b = bodies_of(x, y)
    n = len(x)
    b["mass"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
    b["vel"][:, 0] = (-0.5 * np.asarray(y) + rng.normal(0, 0.1, n)).astype(np.float32)
    b["vel"][:, 1] = (0.5 * np.asarray(x) + rng.normal(0, 0.1, n)).astype(np.float32)
    return b


def check(sim, b, radius, min_members, dims=2, label=None, what=""):
    """The catalogue of the handle against the model of the bodies ``b`` and against nb_groups on the same handle."""
    got = sim.group_catalog(radius, min_members)
    assert got.dtype == L.GROUP_DTYPE
    cat, bound = cm.catalog(b, radius, min_members, dims, label)
    bad = cm.mismatches(got, cat, bound)
    assert not bad, f"{what} radius {radius} min_members {min_members}: " + "; ".join(bad)
    gl, gs = sim.groups(radius, size=True)
    roots = np.flatnonzero((gl == np.arange(gl.size)) & (gs >= min_members))
    assert np.array_equal(got["label"], roots) and np.array_equal(got["members"], gs[roots]), f"{what}: not nb_groups' groups"
    if dims == 2:
        assert (got["pos"][:, 2] == 0).all() and (got["vel"][:, 2] == 0).all()
    return got, cat, bound


def sentinel_records(count):
    out = np.full(count * L.GROUP_DTYPE.itemsize, SENT, np.uint8).view(L.GROUP_DTYPE)
    return out, out.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 1. wave, tile and run tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_tails(n):
    x, y = cloud(n)
    radius, wl, ws, _ = cloud_groups(n)
    b = dressed(x, y, seed=n)
    with direct(b) as sim:
        for min_members in (1, 2, 5):
            got, cat, _ = check(sim, b, radius, min_members, label=wl, what=f"n {n}")
            assert got.shape[0] == int(((wl == np.arange(n)) & (ws >= min_members)).sum())
    if n >= 255:                                                         # groups of five and more exist, and they have an extent
        assert cat.shape[0] >= 2 and got["sigma2"].min() > 0 and got["r_max"].min() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. segments against run boundaries.  The run length R is the implementation's choice: the shapes are repeated for every candidate
# ---------------------------------------------------------------------------------------------------------------------
def singletons(count):
    """`count` bodies 10 apart on a line far from everything else"""
    return 1000.0 + 10.0 * np.arange(count), np.full(count, 500.0)


def clump(size, seed):
    """`size` bodies inside one cell at the origin: diameter 0.85 < radius 1"""
    return np.random.default_rng(seed).uniform(-0.3, 0.3, (2, size))


@pytest.mark.parametrize("R", [256, 512, 1024, 2048])
def test_one_group_against_the_run_boundaries(R):
    for prefix in (1, 63, R - 1):
        px, py = singletons(prefix)
        for size in (R - 1, R, R + 1, 2 * R, 2 * R + 1):
            cx, cy = clump(size, size)
            x, y = np.concatenate([px, cx]).astype(np.float32), np.concatenate([py, cy]).astype(np.float32)
            b = dressed(x, y, seed=prefix)
            # the model's groups, known without its n^2 pass: the clump's box has a diagonal of 0.85 < radius, so every pair of it is
            # linked (16.8 million links at R = 2048), and the singletons are 10 apart and hundreds away from it
            label = np.concatenate([np.arange(prefix), np.full(size, prefix)])
            if R == 256 and prefix == 63:
                assert np.array_equal(label, gm.groups(x, y, 1.0)[0])
            with direct(b) as sim:
                for min_members in (1, 2):
                    got, _, _ = check(sim, b, 1.0, min_members, label=label, what=f"R {R} prefix {prefix} size {size}")
                assert got.shape[0] == 1 and got["label"][0] == prefix and got["members"][0] == size


def test_chain_of_3000_in_permuted_index_order():
    n = 3000
    perm = np.random.default_rng(17).permutation(n)                      # body perm[t] sits at place t of the chain
    t = np.empty(n, np.float32)
    t[perm] = np.arange(n) - 1500.0
    x, y = t * np.float32(0.75), np.full(n, 0.3, np.float32)
    b = dressed(x, y, seed=5)
    with direct(b) as sim:
        got, _, _ = check(sim, b, 1.0, 2, what="chain")
    assert got.shape[0] == 1 and got["members"][0] == n and got["r_max"][0] > 1000


@functools.lru_cache(maxsize=None)
def giant():
    """One group of 20 000 bodies (a jittered lattice, links of 0.75 radius) with 300 singletons of smaller index before it and 300
    of larger index after it; the model's catalogue at min_members 1, computed once."""
    rng = np.random.default_rng(31)
    gx, gy = np.meshgrid(np.arange(200) * 0.75, np.arange(100) * 0.75)
    order = rng.permutation(20000)                                       # the members far from contiguous in space
    gx, gy = gx.ravel()[order] + rng.uniform(-0.05, 0.05, 20000), gy.ravel()[order] + rng.uniform(-0.05, 0.05, 20000)
    sx, sy = singletons(600)
    x = np.concatenate([sx[:300], gx, sx[300:]]).astype(np.float32)
    y = np.concatenate([sy[:300], gy, sy[300:]]).astype(np.float32)
    b = dressed(x, y, seed=32)
    label = gm.groups(x, y, 1.0)[0]
    assert (label[300:20300] == 300).all() and np.array_equal(np.delete(label, np.s_[300:20300]), np.delete(np.arange(20600), np.s_[300:20300]))
    cat, bound = cm.catalog(b, 1.0, 1, label=label)
    for a in (b, label, cat, bound):
        a.setflags(write=False)
    return b, label, cat, bound


def test_giant_group_with_singletons_on_both_sides():
    b, label, cat, bound = giant()
    with direct(b) as sim:
        got = sim.group_catalog(1.0, 1)
        bad = cm.mismatches(got, cat, bound)
        assert not bad, "; ".join(bad)
        assert got.shape[0] == 601 and got["members"][300] == 20000 and (np.delete(got["members"], 300) == 1).all()
        got2, _, _ = check(sim, b, 1.0, 2, label=label, what="giant")
        assert got2.shape[0] == 1 and got2["label"][0] == 300 and got2["members"][0] == 20000


# ---------------------------------------------------------------------------------------------------------------------
# 3. many small groups
# ---------------------------------------------------------------------------------------------------------------------
def test_512_clumps_of_4():
    rng = np.random.default_rng(9)                                       # the bodies of test_groups_gpu.test_many_tight_clumps_far_apart
    cx, cy = np.meshgrid(np.arange(32) * 10.0 - 155.0, np.arange(16) * 10.0 - 75.0)
    x = (np.repeat(cx.ravel(), 4) + rng.uniform(-0.1, 0.1, 2048)).astype(np.float32)
    y = (np.repeat(cy.ravel(), 4) + rng.uniform(-0.1, 0.1, 2048)).astype(np.float32)
    perm = rng.permutation(2048)
    x, y = x[perm], y[perm]
    b = dressed(x, y, seed=10)
    lib = nb.load()
    with direct(b) as sim:
        got, _, _ = check(sim, b, 1.0, 2, what="clumps")
        assert got.shape[0] == 512 and (got["members"] == 4).all()
        assert np.array_equal(check(sim, b, 1.0, 4, what="clumps")[0], got)
        out, before = sentinel_records(8)
        count = C.c_size_t(77)
        assert lib.nb_group_catalog(sim._h, 1.0, 5, out.ctypes.data, 8, C.byref(count)) == L.NB_OK
        assert count.value == 0 and out.tobytes() == before
        assert sim.group_catalog(1.0, 5).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# 4. massless and mixed groups, exact zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_massless_and_mixed_groups_and_exact_zeros():
    rng = np.random.default_rng(4)
    jit = lambda k: rng.uniform(-0.2, 0.2, k)
    x = np.concatenate([jit(5), 10 + jit(5), np.full(3, 20.125), 30 + jit(4)]).astype(np.float32)
    y = np.concatenate([jit(5), jit(5), np.full(3, -3.5), jit(4)]).astype(np.float32)
    b = dressed(x, y, seed=6)
    b["mass"][0:5] = 0.0                                                 # a group without mass
    b["mass"][5:10] = [1.0, 0.0, -2.0, 0.5, 1.5]                         # w = 0 for the massless and for the negative one
    b["mass"][10:13] = [0.75, 1.5, 1.25]                                 # three coincident bodies
    b["vel"][13:17] = [np.float32(0.3), np.float32(-1.7)]                # equal velocities
    with direct(b) as sim:
        got, cat, _ = check(sim, b, 1.0, 1, what="mixed")
    assert got["label"].tolist() == [0, 5, 10, 13] and got["members"].tolist() == [5, 5, 3, 4]
    assert got["mass"][0] == 0.0 and got["mass"][1] == 3.0 and got["mass"][2] == 3.5
    xs, vs = b["pos"][0:5].astype(np.float64), b["vel"][0:5].astype(np.float64)
    assert np.allclose(got["pos"][0][:2], xs.mean(axis=0), rtol=1e-14, atol=1e-16) and np.allclose(got["vel"][0][:2], vs.mean(axis=0), rtol=1e-14)
    w = np.array([1.0, 0.0, 0.0, 0.5, 1.5])
    assert np.allclose(got["pos"][1][:2], (w[:, None] * b["pos"][5:10].astype(np.float64)).sum(axis=0) / 3.0, rtol=1e-14, atol=1e-16)
    assert got["r_max"][1] >= np.linalg.norm(b["pos"][7].astype(np.float64) - got["pos"][1][:2]) * (1 - 1e-14)    # w = 0 members count for r_max
    assert got["r_max"][2] == 0.0 and got["pos"][2].tolist() == [20.125, -3.5, 0.0]
    assert got["sigma2"][3] == 0.0 and got["vel"][3].tolist() == [float(np.float32(0.3)), float(np.float32(-1.7)), 0.0]
    assert cat["r_max"][2] == 0.0 and cat["sigma2"][3] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. handle kinds
# ---------------------------------------------------------------------------------------------------------------------
def test_fp64_handle_against_the_model_on_syncs_floats():
    x, y = cloud(333)
    b = dressed(x, y, seed=7)
    b["mass"] *= np.float32(1.0 / 333)
    with direct(b, precision="fp64") as sim:
        check(sim, b, 0.8, 2, what="fp64 before a step")
        sim.advance(3, 1e-2)
        got = sim.group_catalog(0.8, 2)
        now = sim.sync().copy()                                          # the fp64 state rounded to float
        assert not np.array_equal(now["pos"], b["pos"]) and not np.array_equal(now["vel"], b["vel"])
        cat, bound = cm.catalog(now, 0.8, 2)
        bad = cm.mismatches(got, cat, bound)
        assert not bad, "; ".join(bad)
        check(sim, now, 0.8, 1, what="fp64 after three steps")


def test_dims3_handle_z_takes_part():
    ic = nb.plummer_3d(1000, 7)
    b3 = ic.view(L.BODY3_DTYPE)
    assert np.abs(b3["pos"][:, 2]).max() > 0.5 and np.abs(b3["vel"][:, 2]).max() > 0
    with direct(ic, dims=3, eps=0.05) as sim:
        got, cat, _ = check(sim, b3, 0.06, 2, dims=3, what="dims = 3")
        check(sim, b3, 0.06, 1, dims=3, what="dims = 3")
    assert got.shape[0] > 20 and got["members"].max() > 8
    assert np.abs(got["pos"][:, 2]).max() > 0.01 and np.abs(got["vel"][:, 2]).max() > 0
    flat, _ = cm.catalog(b3, 0.06, 2, dims=2)                            # and the planar model is another answer
    assert (flat["r_max"] < cat["r_max"]).any()


def test_tree_handle_before_any_step_and_after_three():
    x, y = cloud(333)
    b = dressed(x, y, seed=8)
    b["mass"] *= np.float32(1.0 / 333)
    with nb.Simulation(b, eps=0.5, force="tree", theta=0.5, tree_leaves=True, device=0) as sim:
        check(sim, b, 0.8, 2, what="tree handle before any step")
        assert sim.tree_stats()["nodes"] == 0
        sim.advance(3, 1e-2)
        stats = sim.tree_stats()
        got = sim.group_catalog(0.8, 2)
        assert sim.tree_stats() == stats and sim.frame == 3
        now = sim.sync().copy()
        assert not np.array_equal(now["pos"], b["pos"])
        cat, bound = cm.catalog(now, 0.8, 2)
        bad = cm.mismatches(got, cat, bound)
        assert not bad, "; ".join(bad)


def test_block_handle_is_refused_with_the_reason():
    x, y = cloud(1000)
    b = dressed(x, y, seed=9)
    lib = nb.load()
    out, before = sentinel_records(1000)
    count = C.c_size_t(77)
    with direct(b, i_begin=0, i_count=300) as lo, direct(b, i_begin=300, i_count=700) as hi:
        for sim, owned in ((lo, 300), (hi, 700)):
            assert lib.nb_group_catalog(sim._h, 1.0, 2, out.ctypes.data, 1000, C.byref(count)) == L.NB_ESTATE
            text = lib.nb_last_error().decode()
            assert text.startswith("nb_group_catalog:") and f"owns {owned} of the 1000 bodies" in text and "all n" in text, text
            assert lib.nb_group_catalog(sim._h, 1.0, 2, None, 0, C.byref(count)) == L.NB_ESTATE
        assert out.tobytes() == before and count.value == 77
        assert lo.groups(1.0).shape == (300,)                            # nb_groups still serves it


# ---------------------------------------------------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_handles_and_two_calls_agree_byte_for_byte():
    x, y = cloud(4097)
    radius = cloud_groups(4097)[0]
    for b, r, m in ((giant()[0], 1.0, 1), (dressed(x, y, seed=11), radius, 2)):
        with direct(b) as one, direct(b) as two:
            first = one.group_catalog(r, m).tobytes()
            one.groups(r * 0.5, size=True)                               # other work on the shared scratch in between
            assert one.group_catalog(r, m).tobytes() == first
            assert two.group_catalog(r, m).tobytes() == first and len(first) >= 80 * 300


def test_permuting_the_bodies_relabels_the_groups():
    n = 4097
    x, y = cloud(n)
    radius, wl, _, _ = cloud_groups(n)
    b = dressed(x, y, seed=11)
    perm = np.random.default_rng(101).permutation(n)                     # body perm[q] of the first handle is body q of the second
    new = np.empty(n, np.int64)
    new[perm] = np.arange(n)                                             # body i of the first handle is body new[i] of the second
    smallest = np.full(n, n, np.int64)
    np.minimum.at(smallest, wl, new)                                     # by old label: the smallest NEW index of the group
    with direct(b) as sa, direct(b[perm]) as sb:
        ga, ca, ba = check(sa, b, radius, 2, label=wl, what="first handle")
        gb, cb, bb = check(sb, b[perm], radius, 2, label=smallest[wl][perm], what="permuted handle")
    assert sorted(ga["members"].tolist()) == sorted(gb["members"].tolist()) and ga.shape[0] > 300
    row_b = {int(l): r for r, l in enumerate(gb["label"])}
    rows = np.array([row_b[int(smallest[l])] for l in ga["label"]])     # KeyError: a label that is not the smallest new index
    assert sorted(rows.tolist()) == list(range(gb.shape[0]))
    assert np.array_equal(gb["members"][rows], ga["members"])
    for f in cm.FIELDS:                                                  # equal up to the order of summation: within the summed bounds
        d = np.abs(gb[f][rows] - ga[f])
        assert (d <= ba[f] + bb[f][rows]).all(), f
    assert any((gb[f][rows] != ga[f]).any() for f in ("pos", "vel", "sigma2"))     # and the order did change


# ---------------------------------------------------------------------------------------------------------------------
# 7. count query, capacity, destinations
# ---------------------------------------------------------------------------------------------------------------------
def test_count_query_capacity_and_destinations():
    n = 257
    x, y = cloud(n)
    radius, wl, _, _ = cloud_groups(n)
    b = dressed(x, y, seed=12)
    cat, bound = cm.catalog(b, radius, 2, label=wl)
    want = cat.shape[0]
    assert want >= 20
    lib = nb.load()
    with direct(b) as sim, Pinned((want + 3) * 20, np.uint8) as pinned:
        count = C.c_size_t(77)
        assert lib.nb_group_catalog(sim._h, radius, 2, None, 0, C.byref(count)) == L.NB_OK and count.value == want
        assert lib.nb_group_catalog(sim._h, radius, 2, None, 12345, C.byref(count)) == L.NB_OK and count.value == want
        out, before = sentinel_records(want + 3)
        count = C.c_size_t(77)
        assert lib.nb_group_catalog(sim._h, radius, 2, out.ctypes.data, want - 1, C.byref(count)) == L.NB_EINVAL
        text = lib.nb_last_error().decode()
        assert text.startswith("nb_group_catalog:") and f"{want} groups" in text and f"holds {want - 1}" in text, text
        assert count.value == want and out.tobytes() == before
        page_locked = pinned.view(L.GROUP_DTYPE)
        page_locked.view(np.uint8)[:] = SENT
        for dst, capacity in ((out, want), (out, want + 3), (page_locked, want), (page_locked, want + 3)):
            dst.view(np.uint8)[:] = SENT
            count = C.c_size_t(77)
            assert lib.nb_group_catalog(sim._h, radius, 2, dst.ctypes.data, capacity, C.byref(count)) == L.NB_OK, lib.nb_last_error()
            assert count.value == want
            assert not cm.mismatches(dst[:want], cat, bound)
            assert (dst[want:].view(np.uint8) == SENT).all()             # bytes past count records are untouched
        assert page_locked[:want].tobytes() == out[:want].tobytes()
        # the binding: out given, too small, of another dtype
        assert sim.group_catalog(radius, 2, out=out).tobytes() == out[:want].tobytes()
        with pytest.raises(nb.NBodyError):
            sim.group_catalog(radius, 2, out=out[: want - 1])
        with pytest.raises(TypeError):
            sim.group_catalog(radius, 2, out=np.zeros(want * 10, np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals and reports
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x, y = cloud(64)
    lib = nb.load()
    out, before = sentinel_records(64)
    count = C.c_size_t(77)
    po, pc = out.ctypes.data, C.byref(count)
    with direct(dressed(x, y)) as sim:
        for radius in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert lib.nb_group_catalog(sim._h, radius, 2, po, 64, pc) == L.NB_EINVAL, radius
            text = lib.nb_last_error().decode()
            assert text.startswith("nb_group_catalog: radius must be finite and > 0"), text
        for radius in (1e-30, 1e30):                                     # radius * radius is 0 / infinite in float
            assert lib.nb_group_catalog(sim._h, radius, 2, po, 64, pc) == L.NB_EINVAL, radius
            assert lib.nb_last_error().decode().startswith("nb_group_catalog: radius * radius must be finite and > 0 in float")
        assert lib.nb_group_catalog(sim._h, 1.0, 0, po, 64, pc) == L.NB_EINVAL and b"min_members" in lib.nb_last_error()
        assert lib.nb_group_catalog(sim._h, 1.0, 2, po, 64, None) == L.NB_EINVAL and b"NULL count" in lib.nb_last_error()
        assert lib.nb_group_catalog(None, 1.0, 2, po, 64, pc) == L.NB_EINVAL and b"NULL handle" in lib.nb_last_error()
        with pytest.raises(ValueError):
            sim.group_catalog(1.0, 0)
        # NB_ESTATE between nb_step_begin and nb_step_finish
        sim.step_begin(1e-2)
        assert lib.nb_group_catalog(sim._h, 1.0, 2, po, 64, pc) == L.NB_ESTATE and b"a split step is in flight" in lib.nb_last_error()
        sim.step_finish()
        assert out.tobytes() == before and count.value == 77             # none of the refusals wrote anything
        assert lib.nb_group_catalog(sim._h, 1.0, 1, po, 64, pc) == L.NB_OK and 1 <= count.value <= 64


def test_pending_report_leaves_through_the_call_once():
    import test_tree_gpu as ttg                     # the input that makes a build fail through the public interface, reused as it is
    flat = ttg.close_pairs()
    n = flat.shape[0]
    b = ttg.bodies_of(flat)
    lib = nb.load()
    out, before = sentinel_records(n)
    count = C.c_size_t(77)
    with ttg.tree_sim(b, eps=0.05) as sim:
        sim.advance(1, 1e-3)
        assert lib.nb_group_catalog(sim._h, 0.5, 2, out.ctypes.data, n, C.byref(count)) == L.NB_ENOMEM
        text = lib.nb_last_error().decode()
        assert "frame 0" in text and "nodes" in text
        assert out.tobytes() == before and count.value == 77             # nothing was written
        got, _, _ = check(sim, b, 0.5, 2, what="after the report")       # reported once: the next call succeeds (nothing was integrated)
        assert got.shape[0] == n // 2 and (got["members"] == 2).all()


# ---------------------------------------------------------------------------------------------------------------------
# 9. touches nothing; shares its scratch with nb_groups and nb_neighbors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["direct", "tree"])
def test_catalog_leaves_the_trajectory_alone(kind):
    x, y = cloud(333)
    kw = {"tree": dict(force="tree", theta=0.5, tree_leaves=True), "direct": {}}[kind]
    b = bodies_of(x, y, mass=1.0 / 333, radius=0.2)
    b["vel"][:, 0], b["vel"][:, 1] = -0.5 * y, 0.5 * x
    with direct(b, **kw) as plain, direct(b, **kw) as looked:
        plain.advance(4, 1e-2)
        want = plain.sync().copy()
        looked.advance(2, 1e-2)
        looked.group_catalog(0.8, 1)
        assert looked.frame == 2
        looked.advance(1, 1e-2)
        got = looked.group_catalog(0.9, 2)                               # no wait in between: the state of the work enqueued so far
        assert looked.frame == 3
        now = looked.sync().copy()
        cat, bound = cm.catalog(now, 0.9, 2)
        bad = cm.mismatches(got, cat, bound)
        assert not bad, f"{kind}: catalogue taken behind an unfinished step: " + "; ".join(bad)
        looked.advance(1, 1e-2)
        have = looked.sync()
        assert looked.frame == plain.frame == 4
        for f in ("pos", "vel", "acc", "mass", "radius"):
            assert np.array_equal(have[f].view(np.uint32), want[f].view(np.uint32)), f"{kind}: {f} differs after nb_group_catalog"


def test_alternating_with_groups_and_neighbors_at_other_radii():
    x, y = cloud(1000)
    b = dressed(x, y, seed=13)
    want_c = {r: cm.catalog(b, r, 2) for r in (0.4, 0.8)}
    want_g = {r: gm.groups(x, y, r) for r in (0.3, 0.9)}
    want_n = {r: nm.neighbors(x, y, r, 5) for r in (0.5, 1.5)}
    with direct(b) as sim:
        for rc, rg, rn in ((0.4, 0.9, 1.5), (0.8, 0.3, 0.5), (0.4, 0.3, 1.5)):
            bad = cm.mismatches(sim.group_catalog(rc, 2), *want_c[rc])
            assert not bad, f"catalogue at {rc}: " + "; ".join(bad)
            gl, gs, gn = sim.groups(rg, size=True, ngroups=True)
            wl, ws, wn = want_g[rg]
            assert np.array_equal(gl, wl) and np.array_equal(gs, ws) and gn == wn, rg
            gi, gd, gc = sim.neighbors(rn, 5, dist2=True, count=True)
            wi, wd, wc = want_n[rn]
            assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gc, wc), rn
    assert want_c[0.4][0].shape[0] != want_c[0.8][0].shape[0]


# ---------------------------------------------------------------------------------------------------------------------
# 10. the reference's own start: a 1e9 central mass beside light bodies, the weighted sums span nine orders of magnitude
# ---------------------------------------------------------------------------------------------------------------------
def test_default_ics_at_the_references_max_distance():
    ic = nb.default_ics(25000)
    with direct(ic, eps=1.0) as sim:
        got, cat, _ = check(sim, ic, 1000.0, 2, what="default_ics")
    assert got.shape[0] >= 2 and got["members"].max() > 1000 and got["mass"].max() >= 1e9 > 1e3 * got["mass"].min()
