"""numpy restatement of the convergent Barnes-Hut force (NB_FLAG_TREE_LEAVES, include/nbody.h) used by the tree-leaves tests.

The tree is ``tree_model.build_canonical``'s, unchanged.  ``walk`` is ``tree_model.walk`` with the leaves contributing: a leaf
that is not accepted adds its own term when its mass is not zero and d^2 > 0; the nodes visited are the same.

``group=None``   every body walks on its own (the per-lane kernel; with ``quake`` its bits).
``group=64``     the wave-uniform kernel: the bodies in key order (``key_order``) walk in windows of 64, and a node is accepted
                 for a body exactly when ALL bodies of its window accept it.  Two kinds of body leave their window and walk on
                 their own (``walks_alone``), so that a window does not depend on the order of the bodies: massless ones, and
                 a body on a position that first appears in an earlier window.

With ``visited`` the (body, node) terms are returned as well, in visit order per body, for ``tree_model.resum_f64``.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tree_model as tm  # noqa: E402

F = tm.F


def key_order(x, y, m) -> np.ndarray:
    """Body indices in the order the GPU sorts them: inserted bodies by (quadrant path, index), massless bodies last by index."""
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    ins = np.nonzero(m != 0)[0]
    dig = tm.path_digits(x[ins], y[ins], tm.root_cell(x, y))
    order = np.lexsort((ins,) + tuple(dig[:, l] for l in range(tm.DEPTH_CAP - 1, -1, -1)))
    return np.concatenate([ins[order], np.nonzero(m == 0)[0]])


def walks_alone(x, y, m, order, group: int) -> np.ndarray:
    """Per position of ``order``: True where the body takes no part in its window."""
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    k = order.shape[0]
    bx, by, bm = x[order], y[order], m[order]
    head = np.ones(k, bool)
    head[1:] = (bx[1:] != bx[:-1]) | (by[1:] != by[:-1])     # (inserted bodies on one position are neighbours in key order)
    first = np.maximum.accumulate(np.where(head, np.arange(k), 0))
    return (bm == 0) | (first // group != np.arange(k) // group)


def _term(tree, nd, dx, dy, d2, e2, quake):
    t = d2 + e2
    inv = tm.quake_rsqrt(t) if quake else (F(1) / np.sqrt(t)).astype(F)
    s = tree["mass"][nd] * (inv * inv * inv)
    return dx * s, dy * s


def walk(tree: dict, x, y, m, eps: float, theta: float = 1.0, quake: bool = True, group=None, visited: bool = False):
    """Accelerations (ax, ay) of every body with the leaves contributing; with ``visited`` also the (body, node) terms."""
    x, y = np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)
    n = x.shape[0]
    e2 = F(F(eps) * F(eps))
    t2 = F(F(theta) * F(theta))
    ax, ay = np.zeros(n, F), np.zeros(n, F)
    px, py, s2, mass, child, nxt = (tree[k] for k in ("px", "py", "s2", "mass", "child", "next"))
    terms = []
    if group is None:
        order = np.arange(n)
        g = 1
    else:
        order = key_order(x, y, m)
        g = int(group)
    w = -(-n // g)
    body = np.full(w * g, -1, np.int64)                      # windows of g bodies; -1 pads the last one (it does not vote)
    body[:n] = order
    alone = np.zeros(0, np.int64)
    if group is not None:
        out = walks_alone(x, y, m, order, g)
        alone = order[out]
        body[:n][out] = -1
    body = body.reshape(w, g)
    valid = body >= 0
    bx, by = x[np.maximum(body, 0)], y[np.maximum(body, 0)]
    node = np.zeros(w, np.int64)
    live = np.arange(w)
    with np.errstate(all="ignore"):
        while live.size:
            nd = node[live]
            dx, dy = px[nd][:, None] - bx[live], py[nd][:, None] - by[live]
            d2 = dx * dx + dy * dy
            far = (s2[nd][:, None] < d2 * t2) | ~valid[live]
            all_far = far.all(axis=1)
            leaf = child[nd] == 0
            add = ((all_far | (leaf & (mass[nd] != 0)))[:, None] & (d2 > 0) & valid[live])
            if add.any():
                r, c = np.nonzero(add)
                who, which = body[live[r], c], nd[r]
                tx, ty = _term(tree, which, dx[r, c], dy[r, c], d2[r, c], e2, quake)
                ax[who] = ax[who] + tx                       # (a body appears once per round: no repeated index)
                ay[who] = ay[who] + ty
                if visited:
                    terms.append(np.stack([who, which], axis=1))
            new = np.where(all_far | leaf, nxt[nd], child[nd])
            node[live] = new
            live = live[new >= 0]
    if alone.size:                                           # the bodies that left their windows: every one on its own
        lx, ly, lt = walk(tree, x, y, m, eps, theta, quake, None, True)
        ax[alone], ay[alone] = lx[alone], ly[alone]
        terms.append(lt[np.isin(lt[:, 0], alone)])
    if visited:
        return ax, ay, (np.concatenate(terms) if terms else np.zeros((0, 2), np.int64))
    return ax, ay


def accelerations(x, y, m, eps, theta=1.0, quake=True, group=None):
    return walk(tm.build_canonical(x, y, m), x, y, m, eps, theta, quake, group)


def subtree_mass_f64(tree: dict):
    """Per node: the masses of the leaves of its subtree added in float64, and their number (leaves with mass != 0).  The
    subtree of node i is [i, next) in the pre-order layout."""
    total = tree["px"].shape[0]
    leafm = np.where(tree["child"] == 0, tree["mass"].astype(np.float64), 0.0)
    cm = np.concatenate([[0.0], np.cumsum(leafm)])
    cc = np.concatenate([[0], np.cumsum((tree["child"] == 0) & (tree["mass"] != 0))])
    end = subtree_end(tree)
    i = np.arange(total)
    return cm[end] - cm[i], cc[end] - cc[i]


def subtree_end(tree: dict) -> np.ndarray:
    """Per node the index one past its subtree: for a leaf or a branch that is not the last child, its `next`; otherwise
    the next of the nearest ancestor that has one (pre-order: the first later node that is not deeper)."""
    total = tree["px"].shape[0]
    depth = tree["depth"]
    end = np.full(total, total, np.int64)
    stack = []                                               # open nodes, depths increasing
    for i in range(total):
        while stack and depth[stack[-1]] >= depth[i]:
            end[stack.pop()] = i
        stack.append(i)
    return end
