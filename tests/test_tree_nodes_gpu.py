"""GPU: nb_tree_nodes — the tree of the last build exported as the reference's `Node` records, byte for byte against the numpy
statement of the reference form (tests/tree_nodes_model.py over tests/tree_model.py)."""
import ctypes as C
import functools
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tree_model as tm  # noqa: E402
import tree_nodes_model as nm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"


def bodies_of(flat: np.ndarray) -> np.ndarray:
    b = nb.bodies_array(flat.shape[0])
    b["pos"], b["vel"], b["acc"] = flat[:, 0:2], flat[:, 2:4], flat[:, 4:6]
    b["mass"], b["radius"] = flat[:, 6], flat[:, 7]
    return b


def flat_xym(x, y, m) -> np.ndarray:
    flat = np.zeros((len(x), 8), np.float32)
    flat[:, 0], flat[:, 1], flat[:, 6] = x, y, m
    return flat


def tree_sim(bodies, **kw):
    kw.setdefault("rsqrt", "quake")
    return nb.Simulation(bodies, force="tree", device=0, **kw)


def model_nodes(x, y, m):
    """(reference form, pre-order tree) of the model for these bodies."""
    x, y, m = (np.ascontiguousarray(a, np.float32) for a in (x, y, m))
    pre = tm.build_canonical(x, y, m)
    return nm.reference_form(pre, tm.root_cell(x, y)), pre


@functools.lru_cache(maxsize=None)
def fixture_model(name: str):
    """Computed once per fixture and shared; the arrays are not written to."""
    flat = np.load(GOLD / name).astype(np.float32)
    nodes, pre = model_nodes(flat[:, 0], flat[:, 1], flat[:, 6])
    for a in (flat, nodes):
        a.setflags(write=False)
    return flat, nodes, pre


def assert_same_bytes(got: np.ndarray, want: np.ndarray, what: str):
    assert got.dtype == L.NODE_DTYPE and got.shape == want.shape, f"{what}: {got.shape[0]} nodes, the model has {want.shape[0]}"
    g, w = got.view(np.uint8).reshape(-1, 128), want.view(np.uint8).reshape(-1, 128)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} records differ, first {bad[:5]}: {got[bad[:2]]} vs {want[bad[:2]]}"


# ---------------------------------------------------------------------------------------------------------------------
# small shapes
# ---------------------------------------------------------------------------------------------------------------------
SMALL = {
    "one body": (flat_xym([1.5], [-2.0], [3.0]), 1),
    "two distinct bodies": (flat_xym([0.0, 1.0], [0.0, 2.0], [1.0, 2.0]), 5),
    "two coincident bodies": (flat_xym([0.25, 0.25], [4.0, 4.0], [1.0, 2.5]), 1),
    "three massless bodies": (flat_xym([0.0, 1.0, 3.0], [0.0, 1.0, -1.0], [0.0, 0.0, 0.0]), 1),
}


@pytest.mark.parametrize("case", list(SMALL))
def test_small_shapes(case):
    flat, count = SMALL[case]
    want, _ = model_nodes(flat[:, 0], flat[:, 1], flat[:, 6])
    assert want.shape[0] == count
    with tree_sim(bodies_of(flat), eps=0.5) as sim:
        sim.accelerations()
        got = sim.tree_nodes()
        assert sim.tree_stats()["nodes"] == count
    assert got.shape[0] == count
    assert_same_bytes(got, want, case)
    root = got[0]
    assert root["next"] == 0 and root["depth"] == 0
    if case == "one body":
        assert root["children"] == 0 and tuple(root["pos"]) == (1.5, -2.0) and root["mass"] == 3.0     # the root is the leaf
    elif case == "two distinct bodies":
        assert root["children"] == 1 and root["mass"] == 3.0 and sorted(got["mass"][1:].tolist()) == [0.0, 0.0, 1.0, 2.0]
    elif case == "two coincident bodies":
        assert root["children"] == 0 and root["mass"] == 3.5 and tuple(root["pos"]) == (0.25, 4.0)     # the masses summed
    else:
        assert root["children"] == 0 and root["mass"] == 0.0 and tuple(root["pos"]) == (0.0, 0.0)      # the empty root


# ---------------------------------------------------------------------------------------------------------------------
# against the model, byte for byte
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,eps", [("ic_random_333.npy", 0.5), ("ic_plummer_4096.npy", 0.05)])
def test_fixture_trees_equal_the_model_byte_for_byte(name, eps):
    flat, want, _ = fixture_model(name)
    with tree_sim(bodies_of(flat), eps=eps) as sim:
        acc = sim.accelerations()
        got = sim.tree_nodes()
        stats = sim.tree_stats()
    assert got.shape[0] == stats["nodes"] == want.shape[0] and int(got["depth"].max()) == stats["max_depth"]
    assert_same_bytes(got, want, name)                      # all 128 bytes of every record: the padding is zero
    # Quadtree::acc over the exported array reproduces the handle's accelerations bit for bit
    ax, ay = tm.walk(nm.to_walk_dict(got), flat[:, 0].copy(), flat[:, 1].copy(), eps)
    assert tm.same_bits(ax, np.ascontiguousarray(acc[:, 0])) and tm.same_bits(ay, np.ascontiguousarray(acc[:, 1]))
    assert np.abs(ax).max() > 0


def chain_bodies() -> np.ndarray:
    """A long single-child chain: a pair 2^-20 apart inside the unit square spanned by two corner bodies, and 60 random bodies."""
    rng = np.random.default_rng(5)
    rest = rng.random((60, 2), dtype=np.float32)
    x = np.concatenate([np.array([0.0, 1.0, 0.3, np.float32(0.3) + np.float32(2.0 ** -20)], np.float32), rest[:, 0]])
    y = np.concatenate([np.array([0.0, 1.0, 0.3, 0.3], np.float32), rest[:, 1]])
    return flat_xym(x, y, np.full(64, 1.0 / 64, np.float32))


def test_long_single_child_chain():
    flat = chain_bodies()
    want, pre = model_nodes(flat[:, 0], flat[:, 1], flat[:, 6])
    depth = int(pre["depth"].max())
    print(f"chain: model depth {depth}, {want.shape[0]} nodes")
    assert depth >= 18
    with tree_sim(bodies_of(flat), eps=0.01) as sim:
        sim.accelerations()
        got = sim.tree_nodes()
        assert sim.tree_stats()["max_depth"] == depth
    assert_same_bytes(got, want, "chain")


def test_default_bodies_keep_the_invariants_of_the_form():
    """The overlay's own workload: the reference's 25 000 default bodies.  Vectorised invariants, no Python tree build."""
    ic = nb.default_ics(25000)
    with tree_sim(ic, eps=1.0) as sim:
        sim.accelerations()
        got = sim.tree_nodes()
        stats = sim.tree_stats()
    print(f"default bodies: {got.shape[0]} nodes, depth {int(got['depth'].max())}")
    assert got.shape[0] == stats["nodes"] and int(got["depth"].max()) == stats["max_depth"]
    assert 50000 < got.shape[0] < 100000 and 12 <= stats["max_depth"] <= 20
    parent, quad = nm.check_rules(got)                      # next, children, depth, empty leaf ranges
    nm.check_geometry(got, parent, quad)                    # every child's centre and size from its parent's
    nm.check_records(got)                                   # every branch's record from its children, fp32, quadrant order
    x, y = ic["pos"][:, 0], ic["pos"][:, 1]
    cx, cy, size = tm.root_cell(x, y)
    assert tuple(got["center"][0]) == (cx, cy) and got["size"][0] == size
    massive = ic["mass"] != 0
    points = np.unique(np.ascontiguousarray(ic["pos"][massive]).view(np.uint64)).shape[0]   # different positions (none is -0.0 here)
    assert not (np.signbit(ic["pos"]) & (ic["pos"] == 0)).any()
    leaves = (got["children"] == 0) & (got["mass"] > 0)
    assert int(leaves.sum()) == points
    tail = got.view(np.uint8).reshape(-1, 128)
    for lo, hi in ((8, 16), (20, 32), (40, 48), (52, 64), (104, 128)):
        assert not tail[:, lo:hi].any(), "padding bytes are zero"
    # every leaf with bodies holds one of the positions
    lp = np.ascontiguousarray(got["pos"][leaves]).view(np.uint64).ravel()
    assert np.isin(lp, np.ascontiguousarray(ic["pos"][massive]).view(np.uint64).ravel()).all()


# ---------------------------------------------------------------------------------------------------------------------
# which build, which handle
# ---------------------------------------------------------------------------------------------------------------------
def test_the_tree_of_the_last_build_is_exported():
    flat, _, _ = fixture_model("ic_random_333.npy")
    with tree_sim(bodies_of(flat), eps=0.5) as sim:
        sim.advance(2, 1e-3)
        b = sim.sync().copy()                               # the positions of frame 2 ...
        sim.advance(1, 1e-3)                                # ... are the ones the force evaluation of step 3 builds its tree from
        got = sim.tree_nodes()
        assert sim.frame == 3
    want, _ = model_nodes(b["pos"][:, 0], b["pos"][:, 1], b["mass"])
    assert_same_bytes(got, want, "after step 3: the tree of the positions before the drift")
    with tree_sim(bodies_of(flat), eps=0.5, rsqrt="exact", tree_leaves=True, tree_energy=True) as sim:
        sim.advance(1, 1e-3)
        before = sim.tree_nodes()
        sim.energy()                                        # rebuilds the tree at the current positions
        got = sim.tree_nodes()
        b = sim.sync()
    want, _ = model_nodes(b["pos"][:, 0], b["pos"][:, 1], b["mass"])
    assert_same_bytes(got, want, "after energy(): the tree of the current positions")
    assert not np.array_equal(before.view(np.uint8), got.view(np.uint8))


def test_every_tree_handle_exports_the_same_bytes():
    flat, want, _ = fixture_model("ic_random_333.npy")
    ic = bodies_of(flat)
    for kw in (dict(), dict(tree_leaves=True, rsqrt="exact"), dict(tree_leaves=True, tree_quadrupole=True, rsqrt="exact"),
               dict(tree_leaves=True, tree_alpha=0.005), dict(theta=0.3)):
        with tree_sim(ic, eps=0.5, **kw) as sim:
            sim.accelerations()
            assert_same_bytes(sim.tree_nodes(), want, str(kw))


def test_permuting_the_bodies_leaves_the_bytes_unchanged():
    flat = np.load(GOLD / "ic_plummer_1024.npy").astype(np.float32)
    assert np.unique(flat[:, 0:2], axis=0).shape[0] == flat.shape[0]           # distinct positions
    perm = np.random.default_rng(11).permutation(flat.shape[0])
    out = []
    for f in (flat, flat[perm]):
        with tree_sim(bodies_of(f), eps=0.05) as sim:
            sim.accelerations()
            out.append(sim.tree_nodes())              # (a new array per call; .copy() of a record array leaves its padding unset)
    assert out[0].shape[0] > 1024
    assert_same_bytes(out[1], out[0], "permuted bodies")


def test_page_locked_and_pageable_destinations_receive_the_same_bytes():
    flat, want, _ = fixture_model("ic_plummer_4096.npy")
    lib = nb.load()
    count = want.shape[0]
    ptr = lib.nb_host_alloc(count * 128 + 4096)
    assert ptr
    try:
        pinned = np.frombuffer((C.c_uint8 * (count * 128)).from_address(ptr), dtype=L.NODE_DTYPE)
        pinned.view(np.uint8)[:] = 0xEE
        guard = np.frombuffer((C.c_uint8 * 4096).from_address(ptr + count * 128), dtype=np.uint8)
        guard[:] = 0x5A
        pageable = np.full((count + 3) * 128, 0xEE, np.uint8).view(L.NODE_DTYPE)
        with tree_sim(bodies_of(flat), eps=0.05) as sim:
            sim.accelerations()
            a = sim.tree_nodes(out=pinned)
            b = sim.tree_nodes(out=pageable)
            c = sim.tree_nodes()
        assert a.shape[0] == b.shape[0] == c.shape[0] == count
        for got, what in ((a, "nb_host_alloc"), (b, "numpy, larger than needed"), (c, "numpy")):
            assert_same_bytes(got, want, what)
        assert (guard == 0x5A).all() and (pageable[count:].view(np.uint8) == 0xEE).all()        # nothing past count records
        del pinned, guard, a
    finally:
        assert lib.nb_host_free(ptr) == L.NB_OK


def test_exporting_does_not_touch_the_trajectory():
    flat, _, _ = fixture_model("ic_random_333.npy")
    ic = bodies_of(flat)
    with tree_sim(ic, eps=0.5) as plain, tree_sim(ic, eps=0.5) as watched:
        for _ in range(10):
            plain.advance(1, 1e-3)
            watched.advance(1, 1e-3)
            assert watched.tree_nodes().shape[0] > 333
        a, b = plain.sync(), watched.sync()
        assert plain.frame == watched.frame == 10
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert plain.tree_stats() == watched.tree_stats()


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_count_query():
    flat, want, _ = fixture_model("ic_random_333.npy")
    lib = nb.load()
    ic = bodies_of(flat)
    cnt = C.c_size_t(77)
    with nb.Simulation(ic, eps=0.5, device=0) as direct:
        assert lib.nb_tree_nodes(direct._h, None, 0, C.byref(cnt)) == L.NB_ESTATE and b"NB_FORCE_DIRECT" in lib.nb_last_error()
        assert cnt.value == 77
        with pytest.raises(L.NBodyError) as e:
            direct.tree_nodes()
        assert e.value.code == L.NB_ESTATE
    with tree_sim(ic, eps=0.5) as sim:
        assert lib.nb_tree_nodes(sim._h, None, 0, C.byref(cnt)) == L.NB_OK and cnt.value == 0          # a fresh handle: no build yet
        assert sim.tree_nodes().shape[0] == 0
        sim.accelerations()
        n = want.shape[0]
        assert lib.nb_tree_nodes(sim._h, None, 0, C.byref(cnt)) == L.NB_OK and cnt.value == n           # out = NULL: the count only
        assert lib.nb_tree_nodes(sim._h, None, 10 ** 9, C.byref(cnt)) == L.NB_OK and cnt.value == n
        small = np.full((n - 1) * 128, 0xEE, np.uint8).view(L.NODE_DTYPE)
        cnt.value = 0
        assert lib.nb_tree_nodes(sim._h, small.ctypes.data, n - 1, C.byref(cnt)) == L.NB_EINVAL
        assert cnt.value == n and str(n).encode() in lib.nb_last_error() and str(n - 1).encode() in lib.nb_last_error()
        assert (small.view(np.uint8) == 0xEE).all()                                                      # out untouched
        assert lib.nb_tree_nodes(sim._h, small.ctypes.data, 0, C.byref(cnt)) == L.NB_EINVAL
        assert lib.nb_tree_nodes(sim._h, small.ctypes.data, n, None) == L.NB_EINVAL
        with pytest.raises(TypeError):
            sim.tree_nodes(out=np.zeros(n * 128, np.uint8))
        assert_same_bytes(sim.tree_nodes(), want, "after the refused calls")


def test_a_failed_build_is_reported_once_and_never_exported():
    from test_tree_gpu import close_pairs                   # the input of the depth-cap test
    bad = close_pairs(one_ulp=True)
    lib = nb.load()
    cnt = C.c_size_t(77)
    with tree_sim(bodies_of(bad), eps=0.05) as sim:
        sim.advance(1, 1e-3)
        buf = np.full(64 * 128, 0xEE, np.uint8).view(L.NODE_DTYPE)
        assert lib.nb_tree_nodes(sim._h, buf.ctypes.data, 64, C.byref(cnt)) == L.NB_ENOMEM              # the first synchronising call
        assert b"not separated within 63 levels" in lib.nb_last_error()
        sim.wait()                                                                                       # ... once
        for _ in range(2):
            assert lib.nb_tree_nodes(sim._h, buf.ctypes.data, 64, C.byref(cnt)) == L.NB_ESTATE
            assert b"no tree to export" in lib.nb_last_error()
            assert lib.nb_tree_nodes(sim._h, None, 0, C.byref(cnt)) == L.NB_ESTATE
        assert cnt.value == 77 and (buf.view(np.uint8) == 0xEE).all()
        good = np.load(GOLD / "ic_plummer_1024.npy").astype(np.float32)[: bad.shape[0]]
        sim.upload(bodies_of(good))
        sim.accelerations()
        want, _ = model_nodes(good[:, 0], good[:, 1], good[:, 6])
        assert_same_bytes(sim.tree_nodes(), want, "after a good build")
        assert sim.tree_stats()["overflow_steps"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# the C++ adaptor
# ---------------------------------------------------------------------------------------------------------------------
def test_adaptor_fills_quadtree_nodes_for_the_overlay(tmp_path):
    """-DNBODY_TREE=1 -DNBODY_TREE_NODES=1 without the reference's headers: Simulation() steps once, the program walks
    quadtree.nodes like drawQuadtreeNode and meets what the Python-side export holds."""
    exe = tmp_path / "tree_nodes_host"
    libdir = ROOT / "nbodysim_amd"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DNBODY_TREE=1", "-DNBODY_TREE_NODES=1",
                        "-I", str(ROOT / "include"), "-I", str(libdir / "host"), "-o", str(exe), str(ROOT / "tests" / "tree_nodes_host.cpp"),
                        f"-L{libdir}", "-lnbody_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"frame=1 nodes=(\d+) visited=(\d+) leaves=(\d+) branches=(\d+) deepest=(\d+)", r.stdout)
    assert m, r.stdout
    nodes, visited, leaves, branches, deepest = map(int, m.groups())
    with tree_sim(nb.default_ics(25000), eps=1.0, extras=L.NB_EXTRA_VCLAMP | L.NB_EXTRA_BOUNDARY) as sim:
        sim.advance(1, 0.01)
        got = sim.tree_nodes()
    assert nodes == visited == got.shape[0] and branches == int((got["children"] != 0).sum())
    assert leaves == int(((got["children"] == 0) & (got["mass"] != 0)).sum()) and deepest == int(got["depth"].max())
