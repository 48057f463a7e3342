"""numpy restatement of nb_tree_nodes (include/nbody.h): the Barnes-Hut tree as the reference's ``Node`` records, in reference form.

``reference_form``   renumbers a pre-order tree of ``tree_model.build_canonical`` the way the export does: node 0 is the root, the
                     branches are ranked r = 0, 1, ... in pre-order and the children of branch r are nodes 1 + 4 r ... 1 + 4 r + 3 in
                     quadrant order; cell centres are carried down from the root with ``tree_model.child_cell``.
``same_tree``        equality of two ``NODE_DTYPE`` arrays as TREES: from the roots, following ``children``; node indices do not
                     matter, every other field is compared bit for bit.
``to_walk_dict``     a ``NODE_DTYPE`` array as the dict ``tree_model.walk`` takes.
``check_rules`` / ``check_geometry`` / ``check_records``   the invariants of the form, vectorised (no Python tree build): usable on
                     an array of any size and, ``check_rules`` and ``check_geometry``, on the compiled reference's own array.
"""
from __future__ import annotations

import numpy as np

import tree_model as tm

F = np.float32

#: the reference's 128-byte Node (Node.hpp:31-53); restated here so that the model does not depend on the package under test
NODE_DTYPE = np.dtype(
    {
        "names": ["pos", "mass", "center", "size", "children", "next", "bodies_start", "bodies_end", "depth"],
        "formats": [(np.float32, 2), np.float32, (np.float32, 2), np.float32, np.uint64, np.uint64, np.uint64, np.uint64, np.uint64],
        "offsets": [0, 16, 32, 48, 64, 72, 80, 88, 96],
        "itemsize": 128,
    }
)


def nodes_array(n: int) -> np.ndarray:
    return np.zeros(n * NODE_DTYPE.itemsize, np.uint8).view(NODE_DTYPE)


def reference_form(tree: dict, root) -> np.ndarray:
    """``tree``: a pre-order dict of ``build_canonical``; ``root``: (cx, cy, size) of ``root_cell``."""
    child, nxt = tree["child"], tree["next"]
    total = child.shape[0]
    branch = child != 0
    rank = np.cumsum(branch) - branch
    out = nodes_array(total)
    assert total == 1 + 4 * int(branch.sum())
    idx = np.full(total, -1, np.int64)
    idx[0] = 0
    out["center"][0] = (root[0], root[1])
    out["size"][0] = root[2]
    for i in range(total):                                  # pre-order: a parent comes before its children
        e = idx[i]
        out["pos"][e] = (tree["px"][i], tree["py"][i])
        out["mass"][e] = tree["mass"][i]
        out["depth"][e] = tree["depth"][i]
        if not branch[i]:
            continue
        first = 1 + 4 * int(rank[i])
        out["children"][e] = first
        c = i + 1
        for q in range(4):
            idx[c] = first + q
            cx, cy, cs = tm.child_cell(out["center"][e][0], out["center"][e][1], out["size"][e], q)
            out["center"][first + q] = (cx, cy)
            out["size"][first + q] = cs
            out["next"][first + q] = first + q + 1 if q < 3 else out["next"][e]
            c = int(nxt[c]) if nxt[c] >= 0 else total
    return out


FIELDS = ("pos", "mass", "center", "size", "depth", "bodies_start", "bodies_end")


def same_tree(a: np.ndarray, b: np.ndarray) -> bool:
    """The two arrays hold the same tree: equal records (every field but the indices, bit for bit) at the roots and, following
    ``children``, at the four children of every branch; a leaf on one side is a leaf on the other."""
    if a.shape[0] != b.shape[0]:
        return False
    ia, ib = [0], [0]                                       # breadth-first, one level at a time, vectorised
    seen = 0
    while ia:
        ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
        seen += ia.shape[0]
        for f in FIELDS:
            if not tm.same_bits(np.ascontiguousarray(a[f][ia]), np.ascontiguousarray(b[f][ib])):
                return False
        ba, bb = a["children"][ia] != 0, b["children"][ib] != 0
        if not np.array_equal(ba, bb):
            return False
        ca, cb = a["children"][ia][ba].astype(np.int64), b["children"][ib][bb].astype(np.int64)
        if ca.size and (ca.max() + 3 >= a.shape[0] or cb.max() + 3 >= b.shape[0]):
            return False
        ia = (ca[:, None] + np.arange(4)).ravel().tolist()
        ib = (cb[:, None] + np.arange(4)).ravel().tolist()
    return seen == a.shape[0]


def to_walk_dict(nodes: np.ndarray) -> dict:
    nxt = nodes["next"].astype(np.int64)
    size = np.ascontiguousarray(nodes["size"], F)
    return {"px": np.ascontiguousarray(nodes["pos"][:, 0]), "py": np.ascontiguousarray(nodes["pos"][:, 1]),
            "mass": np.ascontiguousarray(nodes["mass"]), "s2": size * size, "child": nodes["children"].astype(np.int64),
            "next": np.where(nxt == 0, -1, nxt), "depth": nodes["depth"].astype(np.int64)}


def check_rules(nodes: np.ndarray):
    """The ``children`` / ``next`` / ``depth`` rules (Quadtree.hpp:64-75).  Returns (parent, quadrant) per node (-1 for the root)."""
    total = nodes.shape[0]
    ch = nodes["children"].astype(np.int64)
    br = np.nonzero(ch)[0]
    assert total == 1 + 4 * br.shape[0], "count = 1 + 4 x branches"
    assert np.array_equal(np.sort(ch[br]), 1 + 4 * np.arange(br.shape[0])), "the children blocks tile nodes 1 .. count - 1"
    parent = np.full(total, -1, np.int64)
    quad = np.full(total, -1, np.int64)
    if br.size:
        kids = ch[br][:, None] + np.arange(4)
        parent[kids] = br[:, None]
        quad[kids] = np.arange(4)
    assert (parent[1:] >= 0).all()
    nxt = nodes["next"].astype(np.int64)
    depth = nodes["depth"].astype(np.int64)
    assert nxt[0] == 0 and depth[0] == 0, "the root: next 0, depth 0"
    i = np.arange(1, total)
    q, p = quad[1:], parent[1:]
    assert np.array_equal(nxt[1:], np.where(q < 3, i + 1, nxt[p])), "next: own index + 1 for quadrants 0..2, the parent's for quadrant 3"
    assert np.array_equal(depth[1:], depth[p] + 1), "depth: the parent's + 1"
    assert not nodes["bodies_start"].any() and not nodes["bodies_end"].any(), "the leaf ranges are empty"
    return parent, quad


def check_geometry(nodes: np.ndarray, parent: np.ndarray, quad: np.ndarray) -> None:
    """Every child's centre and size from its parent's: Quad::into_quadrant (Quad.hpp:51-57), one rounding per operation."""
    p, q = parent[1:], quad[1:]
    size = (nodes["size"][p] * tm.HALF).astype(F)
    cx = nodes["center"][p, 0] + ((q & 1).astype(F) - tm.HALF) * size
    cy = nodes["center"][p, 1] + ((q >> 1).astype(F) - tm.HALF) * size
    assert tm.same_bits(np.ascontiguousarray(nodes["size"][1:]), size), "size: the parent's halved"
    assert tm.same_bits(np.ascontiguousarray(nodes["center"][1:, 0]), cx.astype(F)), "centre x"
    assert tm.same_bits(np.ascontiguousarray(nodes["center"][1:, 1]), cy.astype(F)), "centre y"


def check_records(nodes: np.ndarray) -> None:
    """Every branch's record from its four children, float32, quadrant order (Quadtree.hpp:236-258)."""
    br = np.nonzero(nodes["children"])[0]
    if not br.size:
        return
    first = nodes["children"][br].astype(np.int64)
    sx, sy, sm = np.zeros(br.shape, F), np.zeros(br.shape, F), np.zeros(br.shape, F)
    for q in range(4):
        c = first + q
        m = nodes["mass"][c]
        sx = sx + nodes["pos"][c, 0] * m
        sy = sy + nodes["pos"][c, 1] * m
        sm = sm + m
    pos = sm > 0
    with np.errstate(all="ignore"):
        inv = (F(1) / np.where(pos, sm, F(1))).astype(F)
    sx = np.where(pos, sx * inv, sx).astype(F)
    sy = np.where(pos, sy * inv, sy).astype(F)
    assert tm.same_bits(np.ascontiguousarray(nodes["mass"][br]), sm.astype(F)), "branch mass"
    assert tm.same_bits(np.ascontiguousarray(nodes["pos"][br, 0]), sx), "branch centre of mass x"
    assert tm.same_bits(np.ascontiguousarray(nodes["pos"][br, 1]), sy), "branch centre of mass y"
