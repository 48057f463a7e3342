"""numpy restatement of the quadrupole term of the convergent Barnes-Hut force (NB_FLAG_TREE_QUADRUPOLE, include/nbody.h) used
by the tree-quadrupole tests.

The tree is ``tree_model.build_canonical``'s and the terms are those ``tree_leaves_model.walk`` visits, both unchanged.

``moments(tree)``   per node the raw second moment (xx, xy, yy) of its subtree about its stored centre of mass, in float32 with
                    one rounding per operation: bottom-up, the children in quadrant order, each child's moment moved to the
                    parent's centre by the parallel-axis term.  Leaves and empty quadrants have zeros.
``walk``            ``tree_leaves_model.walk`` (same ``group`` and ``visited`` options) where an accepted BRANCH adds, with
                    d = centre of mass - body, R^2 = d^2 + eps^2, m its mass and M its moment,
                        d * (m R^-3 + 7.5 (d^T M d) R^-7 - 1.5 tr(M) R^-5) - 3 (M d) R^-5
                    and a leaf adds the monopole term as before; one running float32 sum per body in visit order (with ``quake``
                    the bits of the per-lane kernel).
``resum_f64``       the visited (body, node) terms, the quadrupole part included, summed in float64 with an exact 1/sqrt from the
                    float32 node records and the float32 moments.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tree_leaves_model as tlm  # noqa: E402
import tree_model as tm  # noqa: E402

F = tm.F


def moments(tree: dict) -> np.ndarray:
    """(nodes, 3) float32: xx, xy, yy per node."""
    px, py, mass, child, nxt = (tree[k] for k in ("px", "py", "mass", "child", "next"))
    total = px.shape[0]
    mom = np.zeros((total, 3), F)
    for node in range(total - 1, -1, -1):                    # pre-order: the children of a node come after it
        if not child[node]:
            continue
        cx, cy = px[node], py[node]
        xx, xy, yy = F(0), F(0), F(0)
        c = child[node]
        for _ in range(4):
            sx, sy = F(px[c] - cx), F(py[c] - cy)
            xx = F(xx + F(mom[c, 0] + F(mass[c] * F(sx * sx))))
            xy = F(xy + F(mom[c, 1] + F(mass[c] * F(sx * sy))))
            yy = F(yy + F(mom[c, 2] + F(mass[c] * F(sy * sy))))
            c = nxt[c] if nxt[c] >= 0 else total
        mom[node] = xx, xy, yy
    return mom


def term(mass, mom, dx, dy, d2, e2, quake: bool):
    """The float32 term of accepted branches (arrays over terms): what is added to the running sums."""
    t = d2 + e2
    inv = tm.quake_rsqrt(t) if quake else (F(1) / np.sqrt(t)).astype(F)
    inv2 = inv * inv
    inv3 = inv2 * inv
    inv5 = inv3 * inv2
    inv7 = inv5 * inv2
    xx, xy, yy = mom[:, 0], mom[:, 1], mom[:, 2]
    ux = xx * dx + xy * dy
    uy = xy * dx + yy * dy
    rmr = dx * ux + dy * uy
    tr = xx + yy
    g = mass * inv3 + (F(7.5) * (rmr * inv7) - F(1.5) * (tr * inv5))
    return dx * g - F(3.0) * (ux * inv5), dy * g - F(3.0) * (uy * inv5)


def term_f64(mass, mom, dx, dy, eps):
    """The same term in float64 with an exact 1/sqrt (arrays over terms, float64 in and out)."""
    r2 = dx * dx + dy * dy + float(eps) ** 2
    xx, xy, yy = (mom[:, k].astype(np.float64) for k in range(3))
    ux, uy = xx * dx + xy * dy, xy * dx + yy * dy
    g = mass * r2 ** -1.5 + 7.5 * (dx * ux + dy * uy) * r2 ** -3.5 - 1.5 * (xx + yy) * r2 ** -2.5
    return dx * g - 3.0 * ux * r2 ** -2.5, dy * g - 3.0 * uy * r2 ** -2.5


def walk(tree: dict, mom: np.ndarray, x, y, m, eps: float, theta: float = 1.0, quake: bool = True, group=None, visited: bool = False):
    """Accelerations (ax, ay) of every body; with ``visited`` also the (body, node) terms, in visit order per body."""
    x, y = np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)
    n = x.shape[0]
    e2 = F(F(eps) * F(eps))
    pairs = tlm.walk(tree, x, y, m, eps, theta, quake, group, True)[2]
    order = np.argsort(pairs[:, 0], kind="stable")           # per body in visit order
    b, nd = pairs[order, 0], pairs[order, 1]
    with np.errstate(all="ignore"):
        dx, dy = tree["px"][nd] - x[b], tree["py"][nd] - y[b]
        d2 = dx * dx + dy * dy
        tx, ty = tlm._term(tree, nd, dx, dy, d2, e2, quake)  # leaves: the monopole term, unchanged
        br = tree["child"][nd] != 0                          # a branch among the terms was accepted
        qx, qy = term(tree["mass"][nd[br]], mom[nd[br]], dx[br], dy[br], d2[br], e2, quake)
    tx[br], ty[br] = qx, qy
    ax, ay = np.zeros(n, F), np.zeros(n, F)
    start = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=n))])
    rank = np.arange(b.shape[0]) - start[b]
    by_rank = np.argsort(rank, kind="stable")
    cut = np.concatenate([[0], np.cumsum(np.bincount(rank))]) if b.size else [0]
    for r in range(len(cut) - 1):                            # one running sum per body: its r-th term, all bodies at once
        k = by_rank[cut[r]:cut[r + 1]]
        ax[b[k]] = ax[b[k]] + tx[k]
        ay[b[k]] = ay[b[k]] + ty[k]
    if visited:
        return ax, ay, pairs
    return ax, ay


def resum_f64(tree: dict, mom: np.ndarray, x, y, pairs: np.ndarray, eps: float):
    """The visited terms summed in float64: the monopole part of every term (tree_model.resum_f64) and the quadrupole part of
    the branches among them."""
    n = x.shape[0]
    b, nd = pairs[:, 0], pairs[:, 1]
    dx = tree["px"][nd].astype(np.float64) - x[b].astype(np.float64)
    dy = tree["py"][nd].astype(np.float64) - y[b].astype(np.float64)
    m0 = np.where(tree["child"][nd] != 0, mom[nd].astype(np.float64).T, 0.0).T
    tx, ty = term_f64(tree["mass"][nd].astype(np.float64), m0, dx, dy, eps)
    return np.bincount(b, tx, n), np.bincount(b, ty, n)


def accelerations(x, y, m, eps, theta=1.0, quake=True, group=None):
    tree = tm.build_canonical(x, y, m)
    return walk(tree, moments(tree), x, y, m, eps, theta, quake, group)
