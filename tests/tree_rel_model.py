"""numpy restatement of the acceleration-relative opening criterion of the convergent Barnes-Hut force (NB_FLAG_TREE_RELATIVE,
include/nbody.h) used by the tree-relative tests.

The tree is ``tree_model.build_canonical``'s, the moments ``tree_quad_model.moments``', the visit loop that of
``tree_leaves_model.walk`` (same ``group`` option, same "walks alone" rule) and the terms those of ``tree_leaves_model`` /
``tree_quad_model``; only the acceptance test differs.  Per body i

    g_i = alpha * sqrt(ax ax + ay ay)         (ax, ay) = aprev[i]; float32, one rounding per operation, np.sqrt on float32

and a node {c, m, s^2} at d = c - position is far for body i when BOTH hold (float32, this order)

    s^2 < d^2 * theta^2
    g_i == 0  or  m * s^2 < (g_i * d^2) * d^2

``walk``        accelerations and the number of node visits: one per (body, node) a per-lane walk looks at; with ``group`` one
                per (window, node), plus the per-lane visits of the bodies that walk alone.  ``mom`` None: monopole terms only.
                With ``visited`` also the (body, node) terms, for ``tree_quad_model.resum_f64`` and ``tree_energy_model.phi``.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tree_leaves_model as tlm  # noqa: E402
import tree_model as tm  # noqa: E402
import tree_quad_model as tqm  # noqa: E402

F = tm.F


def g_of(aprev, alpha) -> np.ndarray:
    """alpha |a_prev| per body in float32, one rounding per operation."""
    a = np.ascontiguousarray(aprev, F)
    ax, ay = a[:, 0], a[:, 1]
    with np.errstate(all="ignore"):
        return (F(alpha) * np.sqrt(ax * ax + ay * ay)).astype(F)


def pairs_of(tree: dict, x, y, m, aprev, eps: float, theta: float, alpha: float, group=None):
    """The (body, node) terms of the relative walk, in visit order per body, and the number of node visits."""
    x, y = np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)
    n = x.shape[0]
    t2 = F(F(theta) * F(theta))
    gb = g_of(aprev, alpha)
    px, py, s2, mass, child, nxt = (tree[k] for k in ("px", "py", "s2", "mass", "child", "next"))
    with np.errstate(all="ignore"):
        ms2 = (mass * s2).astype(F)
    terms = []
    if group is None:
        order = np.arange(n)
        g = 1
    else:
        order = tlm.key_order(x, y, m)
        g = int(group)
    w = -(-n // g)
    body = np.full(w * g, -1, np.int64)                      # windows of g bodies; -1 pads the last one (it does not vote)
    body[:n] = order
    alone = np.zeros(0, np.int64)
    if group is not None:
        out = tlm.walks_alone(x, y, m, order, g)
        alone = order[out]
        body[:n][out] = -1
    body = body.reshape(w, g)
    valid = body >= 0
    at = np.maximum(body, 0)
    bx, by, bg = x[at], y[at], gb[at]
    node = np.zeros(w, np.int64)
    live = np.arange(w)
    if group is not None:
        live = live[valid.any(axis=1)]                       # (a window whose bodies all left it launches no walk)
    visits = 0
    with np.errstate(all="ignore"):
        while live.size:
            nd = node[live]
            visits += int(live.size)
            dx, dy = px[nd][:, None] - bx[live], py[nd][:, None] - by[live]
            d2 = dx * dx + dy * dy
            gl = bg[live]
            rel = (gl == 0) | (ms2[nd][:, None] < (gl * d2) * d2)
            far = ((s2[nd][:, None] < d2 * t2) & rel) | ~valid[live]
            all_far = far.all(axis=1)
            leaf = child[nd] == 0
            add = ((all_far | (leaf & (mass[nd] != 0)))[:, None] & (d2 > 0) & valid[live])
            if add.any():
                r, c = np.nonzero(add)
                terms.append(np.stack([body[live[r], c], nd[r]], axis=1))
            new = np.where(all_far | leaf, nxt[nd], child[nd])
            node[live] = new
            live = live[new >= 0]
    if alone.size:                                           # the bodies that left their windows: every one on its own
        lane, lane_visits = pairs_of(tree, x, y, m, aprev, eps, theta, alpha, None)
        keep = np.isin(lane[:, 0], alone)
        terms.append(lane[keep])
        # a per-lane walk visits, per body, the nodes it takes a term from or opens; count the alone bodies' share exactly
        visits += _lane_visits(tree, x, y, gb, t2, alone)
    return (np.concatenate(terms) if terms else np.zeros((0, 2), np.int64)), visits


def _lane_visits(tree, x, y, gb, t2, who) -> int:
    """Node visits of the per-lane walks of the bodies ``who``."""
    px, py, s2, mass, child, nxt = (tree[k] for k in ("px", "py", "s2", "mass", "child", "next"))
    with np.errstate(all="ignore"):
        ms2 = (mass * s2).astype(F)
    node = np.zeros(who.shape[0], np.int64)
    live = np.arange(who.shape[0])
    visits = 0
    with np.errstate(all="ignore"):
        while live.size:
            nd = node[live]
            visits += int(live.size)
            dx, dy = px[nd] - x[who[live]], py[nd] - y[who[live]]
            d2 = dx * dx + dy * dy
            gl = gb[who[live]]
            far = (s2[nd] < d2 * t2) & ((gl == 0) | (ms2[nd] < (gl * d2) * d2))
            new = np.where(far | (child[nd] == 0), nxt[nd], child[nd])
            node[live] = new
            live = live[new >= 0]
    return visits


def sum_terms(tree: dict, mom, x, y, pairs: np.ndarray, eps: float, quake: bool):
    """One running float32 sum per body over its terms in visit order (tree_quad_model.walk's summation): a leaf, or any node
    without ``mom``, adds the monopole term; an accepted branch with ``mom`` the quadrupole form."""
    x, y = np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)
    n = x.shape[0]
    e2 = F(F(eps) * F(eps))
    order = np.argsort(pairs[:, 0], kind="stable")           # per body in visit order
    b, nd = pairs[order, 0], pairs[order, 1]
    with np.errstate(all="ignore"):
        dx, dy = tree["px"][nd] - x[b], tree["py"][nd] - y[b]
        d2 = dx * dx + dy * dy
        tx, ty = tlm._term(tree, nd, dx, dy, d2, e2, quake)
        if mom is not None:
            br = tree["child"][nd] != 0                      # a branch among the terms was accepted
            qx, qy = tqm.term(tree["mass"][nd[br]], mom[nd[br]], dx[br], dy[br], d2[br], e2, quake)
            tx[br], ty[br] = qx, qy
    ax, ay = np.zeros(n, F), np.zeros(n, F)
    start = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=n))])
    rank = np.arange(b.shape[0]) - start[b]
    by_rank = np.argsort(rank, kind="stable")
    cut = np.concatenate([[0], np.cumsum(np.bincount(rank))]) if b.size else [0]
    with np.errstate(all="ignore"):
        for r in range(len(cut) - 1):                        # its r-th term, all bodies at once
            k = by_rank[cut[r]:cut[r + 1]]
            ax[b[k]] = ax[b[k]] + tx[k]
            ay[b[k]] = ay[b[k]] + ty[k]
    return ax, ay


def walk(tree: dict, mom, x, y, m, aprev, eps: float, theta: float = 1.0, alpha: float = 0.005, quake: bool = True, group=None,
         visited: bool = False):
    """(ax, ay, visits) of every body, and with ``visited`` the (body, node) terms as a fourth item."""
    pairs, visits = pairs_of(tree, x, y, m, aprev, eps, theta, alpha, group)
    ax, ay = sum_terms(tree, mom, x, y, pairs, eps, quake)
    if visited:
        return ax, ay, visits, pairs
    return ax, ay, visits


def resum_f64(tree: dict, mom, x, y, pairs: np.ndarray, eps: float):
    """The visited terms in float64 (tree_quad_model.resum_f64; zero moments without ``mom``)."""
    if mom is None:
        mom = np.zeros((tree["px"].shape[0], 3), F)
    return tqm.resum_f64(tree, mom, np.ascontiguousarray(x, F), np.ascontiguousarray(y, F), pairs, eps)
