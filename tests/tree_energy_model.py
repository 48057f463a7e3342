"""numpy restatement of the tree potential energy (NB_FLAG_TREE_ENERGY, include/nbody.h) used by the tree-energy tests.

The tree is ``tree_model.build_canonical``'s (float32 node records) and ``tree_quad_model.moments``' (float32 moments); the
terms are the (body, node) pairs the wave-uniform walk takes, ``tree_leaves_model.walk(..., group=64, visited=True)``:
whatever the handle's rsqrt mode, the potential has this one walk.  Everything from the term on is float64.

``term``        per (body, node), with d = node centre - body position and R^2 = d^2 + eps^2 (eps the float32 value the
                handle holds):  a leaf, or any node without ``quad``:  -m / R;
                an accepted branch with ``quad``:  -(m / R + 1.5 (d^T M d) / R^5 - 0.5 tr(M) / R^3).
``leaf_mass``   the mass a node has in a -m / R term.  A leaf that holds several bodies is the one node whose float32 mass is a
                rounded sum, and at theta = 0 every other body sees it: the kernel keeps per such leaf the float32 residual
                lo = float32(float64 sum of its masses in body order - record mass) and uses float64(record) + float64(lo),
                the float64 sum to 2^-48.  Every other node (a leaf of one body: lo = 0; a branch) has its record's mass.
``shared``      per body the bodies on its own position (its own leaf has d^2 = 0 and gives no term): each adds -m_j / eps,
                one by one (never "leaf mass - own mass": the leaf's float32 sum has lost the light ones); nothing with
                eps = 0.
``potential``   U = 1/2 sum m_i phi_i: every unordered pair once, massless bodies weigh nothing.
``direct``      -sum_{i<j} m_i m_j / sqrt(r_ij^2 + eps^2) by brute force, the convention of nb_energy without the flag
                (with ``skip_coincident`` the pairs on one position are left out, as the tree form does at eps = 0).
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
D = np.float64


def eps_of(eps) -> float:
    return float(F(eps))


def term(mass, mom, dx, dy, eps):
    """The float64 potential term (arrays over terms; ``mom`` (k, 3) with zeros where the monopole form applies)."""
    r2 = dx * dx + dy * dy + eps_of(eps) ** 2
    xx, xy, yy = (mom[:, k].astype(D) for k in range(3))
    rmr = dx * (xx * dx + xy * dy) + dy * (xy * dx + yy * dy)
    return -(mass * r2 ** -0.5 + 1.5 * rmr * r2 ** -2.5 - 0.5 * (xx + yy) * r2 ** -1.5)


def shared(x, y, m, eps) -> np.ndarray:
    """Per body: sum over the OTHER inserted bodies on its position of -m_j / eps (zeros with eps = 0 and for massless bodies)."""
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    out = np.zeros(x.shape[0], D)
    e = eps_of(eps)
    if e == 0.0:
        return out
    ins = np.nonzero(m != 0)[0]
    pos = np.stack([x[ins], y[ins]], axis=1)
    _, inv, cnt = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    for g in np.nonzero(cnt > 1)[0]:
        members = ins[inv == g]                              # ascending body index: the order of the sorted run
        for i in members:
            s = 0.0
            for j in members:
                if j != i:
                    s += -float(m[j]) / e
            out[i] = s
    return out


def leaf_mass(tree: dict, x, y, m) -> np.ndarray:
    """Per node the float64 mass of its monopole term (see above)."""
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    out = tree["mass"].astype(D)
    where = {}
    for b in np.nonzero(m != 0)[0]:                          # ascending body index: the order of the sorted run
        where.setdefault((float(x[b]), float(y[b])), []).append(b)
    for nd in np.nonzero((tree["child"] == 0) & (tree["mass"] != 0))[0]:
        members = where[float(tree["px"][nd]), float(tree["py"][nd])]
        total = 0.0
        for b in members:
            total += float(m[b])
        out[nd] = float(tree["mass"][nd]) + float(F(total - float(tree["mass"][nd])))
    return out


def phi(tree: dict, mom, x, y, m, eps, theta: float, quad: bool, pairs=None) -> np.ndarray:
    """Per body the potential the walk gives it (float64), the shared-position partners included."""
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    n = x.shape[0]
    if pairs is None:
        pairs = tlm.walk(tree, x, y, m, eps, theta, False, 64, True)[2]
    b, nd = pairs[:, 0], pairs[:, 1]
    dx = tree["px"][nd].astype(D) - x[b].astype(D)
    dy = tree["py"][nd].astype(D) - y[b].astype(D)
    m0 = np.zeros((nd.shape[0], 3), D)
    if quad:
        br = tree["child"][nd] != 0                          # a branch among the terms was accepted
        m0[br] = mom[nd[br]].astype(D)
    return np.bincount(b, term(leaf_mass(tree, x, y, m)[nd], m0, dx, dy, eps), n) + shared(x, y, m, eps)


def potential(x, y, m, eps, theta: float, quad: bool, tree=None, mom=None) -> float:
    x, y, m = (np.ascontiguousarray(a, F) for a in (x, y, m))
    if tree is None:
        tree = tm.build_canonical(x, y, m)
    if quad and mom is None:
        mom = tqm.moments(tree)
    p = phi(tree, mom, x, y, m, eps, theta, quad)
    w = m.astype(D)
    return float(0.5 * np.sum(np.where(w != 0, w * p, 0.0)))


def kinetic(vx, vy, m) -> float:
    vx, vy, m = (np.asarray(a, F).astype(D) for a in (vx, vy, m))
    return float(np.sum(0.5 * m * (vx * vx + vy * vy)))


def direct(x, y, m, eps, skip_coincident: bool = False) -> float:
    """-sum_{i<j} m_i m_j / sqrt(r^2 + eps^2) in float64 from the float32 inputs, row by row."""
    x, y, m = (np.asarray(a, F).astype(D) for a in (x, y, m))
    e2 = eps_of(eps) ** 2
    u = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(x.shape[0] - 1):
            dx, dy = x[i + 1:] - x[i], y[i + 1:] - y[i]
            d2 = dx * dx + dy * dy
            t = m[i + 1:] / np.sqrt(d2 + e2)
            if skip_coincident:
                t = np.where(d2 > 0, t, 0.0)
            u -= m[i] * float(np.sum(t))
    return u
