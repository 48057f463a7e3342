"""CPU: the numpy statement of the convergent Barnes-Hut force (tests/tree_leaves_model.py, NB_FLAG_TREE_LEAVES) — theta = 0 is
the direct sum, every inserted body is counted exactly once at any theta, the wave-uniform walk never opens less than a body's own
walk — and the interface additions."""
import ctypes as C
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

GOLD = Path(__file__).resolve().parent / "golden"
CASES = {"plummer_1024": ("ic_plummer_1024.npy", 0.05), "random_333": ("ic_random_333.npy", 0.5)}
_cache = {}


def case(name):
    """(x, y, m, eps, tree) of a fixture, built once and shared (nothing below writes into it)."""
    if name not in _cache:
        file, eps = CASES[name]
        flat = np.load(GOLD / file).astype(np.float32)
        x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
        _cache[name] = (x, y, m, eps, tm.build_canonical(x, y, m))
    return _cache[name]


def terms_of(name, theta, group):
    key = (name, theta, group)
    if key not in _cache:
        x, y, m, eps, tree = case(name)
        _cache[key] = tlm.walk(tree, x, y, m, eps, theta, quake=False, group=group, visited=True)[2]
    return _cache[key]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("group", [None, 64])
def test_theta_zero_is_the_direct_sum(name, group):
    """Every body's terms are the other distinct positions, each once, and their float64 sum is the float64 direct sum."""
    import nbo
    x, y, m, eps, tree = case(name)
    n = x.shape[0]
    pairs = terms_of(name, 0.0, group)
    leaves = np.nonzero((tree["child"] == 0) & (tree["mass"] != 0))[0]
    own = np.full(n, -1, np.int64)                            # the leaf at a body's own position
    for leaf in leaves:
        own[(x == tree["px"][leaf]) & (y == tree["py"][leaf])] = leaf
    # every body's term set: the other distinct positions, each once
    seen = np.zeros((n, tree["px"].shape[0]), np.int64)
    np.add.at(seen, (pairs[:, 0], pairs[:, 1]), 1)
    want = np.zeros_like(seen)
    want[:, leaves] = 1
    has = own >= 0
    want[np.nonzero(has)[0], own[has]] = 0
    assert np.array_equal(seen, want)
    # re-summed in float64 throughout: a leaf that several bodies share carries their masses added in float32 (the build's
    # rounding, the same with and without the flag), so the masses of a leaf's bodies are added in float64 here
    # (ic_random_333 has one such pair: 332 positions).  First the tree's own leaf masses: the float32 sum in body order.
    for leaf in leaves:
        f32 = np.float32(0)
        for b in np.nonzero(own == leaf)[0]:
            f32 = np.float32(f32 + m[b])
        assert tree["mass"][leaf] == f32
    exact = dict(tree, mass=np.bincount(own[has], m[has].astype(np.float64), tree["px"].shape[0]))
    ax, ay = tm.resum_f64(exact, x, y, pairs, eps)
    st = {"x": x.astype(np.float64), "y": y.astype(np.float64), "m": m.astype(np.float64)}
    dx, dy = nbo.accel_f64(st, eps)
    scale = np.hypot(dx, dy).max()
    assert np.hypot(ax - dx, ay - dy).max() <= 1e-12 * scale


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("theta", [1.0, 0.5, 0.3])
@pytest.mark.parametrize("group", [None, 64])
def test_every_inserted_body_is_counted_exactly_once(name, theta, group):
    """Per body the masses (leaf masses added in float64) and the numbers of positions of its accepted cells and leaves add
    up to all inserted ones less those at its own position."""
    x, y, m, eps, tree = case(name)
    n = x.shape[0]
    pairs = terms_of(name, theta, group)
    m64, cnt = tlm.subtree_mass_f64(tree)
    leaf = (tree["child"] == 0) & (tree["mass"] != 0)
    own_m, own_c = np.zeros(n), np.zeros(n, np.int64)
    for l in np.nonzero(leaf)[0]:
        at = (x == tree["px"][l]) & (y == tree["py"][l])
        own_m[at], own_c[at] = tree["mass"][l], 1
    got_m = np.bincount(pairs[:, 0], m64[pairs[:, 1]], n)
    got_c = np.bincount(pairs[:, 0], cnt[pairs[:, 1]], n)
    assert np.array_equal(got_c, cnt[0] - own_c)
    assert np.abs(got_m - (m64[0] - own_m)).max() <= 1e-12 * m64[0]
    # no term inside another: a node and one of its descendants are never both taken
    end = tlm.subtree_end(tree)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    b, nd = pairs[order, 0], pairs[order, 1]
    same = b[1:] == b[:-1]
    assert (nd[1:][same] >= end[nd[:-1]][same]).all()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("theta", [1.0, 0.5, 0.3])
def test_the_group_walk_opens_every_node_the_bodys_own_walk_opens(name, theta):
    """Every term of the group=64 walk lies inside (or is) a term of the body's own walk: the group's partition of the bodies
    refines the per-body one, so it is never the coarser approximation."""
    x, y, m, eps, tree = case(name)
    total = tree["px"].shape[0]
    end = tlm.subtree_end(tree)
    lane, grp = terms_of(name, theta, None), terms_of(name, theta, 64)
    lkey = np.sort(lane[:, 0] * total + lane[:, 1])
    gkey = grp[:, 0] * total + grp[:, 1]
    at = np.searchsorted(lkey, gkey, side="right") - 1
    assert (at >= 0).all()
    lb, ln = lkey[at] // total, lkey[at] % total
    assert (lb == grp[:, 0]).all() and (grp[:, 1] < end[ln]).all()
    assert grp.shape[0] >= lane.shape[0]


def test_the_per_body_walk_visits_the_nodes_of_the_walk_without_leaves():
    """Same tree, same acceptance test: the accepted cells are those of tree_model.walk, the rest of the terms are leaves."""
    x, y, m, eps, tree = case("plummer_1024")
    _, _, base = tm.walk(tree, x, y, eps, 0.5, visited=True)
    with_leaves = terms_of("plummer_1024", 0.5, None)
    total = tree["px"].shape[0]
    a, b = set((base[:, 0] * total + base[:, 1]).tolist()), set((with_leaves[:, 0] * total + with_leaves[:, 1]).tolist())
    assert a <= b and all(tree["child"][k % total] == 0 for k in b - a) and len(b) > len(a)


def test_interface_additions():
    lib = nb.load()
    assert lib.nb_abi_version() == 8 == L.NB_ABI_VERSION
    assert L.NB_FLAG_TREE_LEAVES == 4096
    header = (Path(__file__).resolve().parents[1] / "include" / "nbody.h").read_text()
    assert "NB_FLAG_TREE_LEAVES     = 4096" in header and "#define NB_ABI_VERSION 8" in header
    b = nb.bodies_array(16)
    b["mass"] = 1.0
    p = L.default_params()
    p.flags = L.NB_FLAG_TREE_LEAVES
    assert p.force == L.NB_FORCE_DIRECT
    assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))                 # refused before a device is looked for
    assert lib.nb_last_error_code() == L.NB_EINVAL
    assert b"NB_FLAG_TREE_LEAVES" in lib.nb_last_error() and b"NB_FORCE_DIRECT" in lib.nb_last_error()
    p.flags = 2048                                                            # stays an unknown bit
    assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
    assert lib.nb_last_error_code() == L.NB_EINVAL and b"unknown bits" in lib.nb_last_error()
    # every refusal of NB_FORCE_TREE holds with the flag
    for field, value, text in (("precision", L.NB_FP64, b"NB_FP64"), ("dims", 3, b"dims = 3"), ("integrator", L.NB_INTEGRATOR_KDK, b"KDK"),
                               ("shard_world", 2, b"shard_world"), ("i_count", 8, b"i_count < n"), ("sum_order", L.NB_SUM_SEQUENTIAL, b"NB_SUM_SEQUENTIAL")):
        p = L.default_params()
        p.force, p.flags = L.NB_FORCE_TREE, L.NB_FLAG_TREE_LEAVES
        setattr(p, field, value)
        assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
        assert lib.nb_last_error_code() == L.NB_EINVAL and text in lib.nb_last_error() and b"NB_FORCE_TREE" in lib.nb_last_error(), field
    with pytest.raises(ValueError):
        nb.Simulation(b, force="direct", tree_leaves=True)
