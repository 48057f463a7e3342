"""numpy restatement of the collision step (NB_EXTRA_COLLIDE, include/nbody.h) used by the collision tests.

State: dict of 1-D arrays x, y, vx, vy, m (float32 or float64) and r (float32).  ``pairs`` finds P, the overlapping pairs
i < j in ascending order, by a chunked brute force; ``resolve_sequential`` applies the reference's resolve(i, j)
(Simulation.hpp:293-346) to each in order, one at a time; ``resolve_rounds`` applies the same pairs the way the GPU kernel
schedules them (a pair runs once it is the lowest pending pair of both its bodies, all such pairs of a round together).
"""
from __future__ import annotations

import numpy as np


def pairs(x, y, r, chunk: int = 1024) -> np.ndarray:
    """(k, 2) int64 array of the pairs i < j with d.x*d.x + d.y*d.y <= (r_i + r_j)^2 (d = p_j - p_i, one rounding per op)."""
    n = x.shape[0]
    rr = r.astype(x.dtype)
    out = []
    with np.errstate(all="ignore"):
        for i0 in range(0, n, chunk):
            i1 = min(n, i0 + chunk)
            dx = x[None, :] - x[i0:i1, None]
            dy = y[None, :] - y[i0:i1, None]
            s = rr[i0:i1, None] + rr[None, :]
            hit = dx * dx + dy * dy <= s * s
            ii, jj = np.nonzero(hit)
            ii = ii + i0
            keep = jj > ii
            out.append(np.stack([ii[keep], jj[keep]], axis=1))
    p = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    order = np.lexsort((p[:, 1], p[:, 0]))
    return p[order].astype(np.int64)


def _resolve_arrays(st: dict, I: np.ndarray, J: np.ndarray) -> None:
    """resolve(I[k], J[k]) for DISJOINT pairs at once (no body in two of them), in place."""
    if I.size == 0:
        return
    x, y, vx, vy, m = st["x"], st["y"], st["vx"], st["vy"], st["m"]
    T = x.dtype.type
    zero, one, onehalf = T(0), T(1), T(1.5)
    with np.errstate(all="ignore"):
        p1x, p1y, p2x, p2y = x[I], y[I], x[J], y[J]
        v1x, v1y, v2x, v2y = vx[I], vy[I], vx[J], vy[J]
        dx, dy = p2x - p1x, p2y - p1y
        r = st["r"][I].astype(x.dtype) + st["r"][J].astype(x.dtype)
        d_sq = dx * dx + dy * dy
        r_sq = r * r
        hit = ~(d_sq > r_sq)
        wx, wy = v2x - v1x, v2y - v1y
        d_dot_v = dx * wx + dy * wy
        m1, m2 = m[I], m[J]
        w1, w2 = m2 / (m1 + m2), m1 / (m1 + m2)
        sep = hit & (d_dot_v >= zero) & ~((dx == zero) & (dy == zero))
        col = hit & ~sep
        # separating / resting: push apart along d
        s = r / np.sqrt(d_sq) - one
        tx, ty = dx * s, dy * s
        sx1, sy1 = p1x - tx * w1, p1y - ty * w1
        sx2, sy2 = p2x + tx * w2, p2y + ty * w2
        # approaching: back to contact, exchange along the new d, forward again
        v_sq = wx * wx + wy * wy
        disc = d_dot_v * d_dot_v - v_sq * (d_sq - r_sq)
        disc = np.where(disc < zero, zero, disc)
        t = (d_dot_v + np.sqrt(disc)) / v_sq
        q1x, q1y = p1x - v1x * t, p1y - v1y * t
        q2x, q2y = p2x - v2x * t, p2y - v2y * t
        ndx, ndy = q2x - q1x, q2y - q1y
        nd_dot_v = ndx * wx + ndy * wy
        nd_sq = ndx * ndx + ndy * ndy
        k = onehalf * nd_dot_v / nd_sq
        ux, uy = ndx * k, ndy * k
        n1x, n1y = v1x + ux * w1, v1y + uy * w1
        n2x, n2y = v2x - ux * w2, v2y - uy * w2
        c1x, c1y = q1x + n1x * t, q1y + n1y * t
        c2x, c2y = q2x + n2x * t, q2y + n2y * t
    x[I] = np.where(sep, sx1, np.where(col, c1x, p1x))
    y[I] = np.where(sep, sy1, np.where(col, c1y, p1y))
    x[J] = np.where(sep, sx2, np.where(col, c2x, p2x))
    y[J] = np.where(sep, sy2, np.where(col, c2y, p2y))
    vx[I] = np.where(col, n1x, v1x)
    vy[I] = np.where(col, n1y, v1y)
    vx[J] = np.where(col, n2x, v2x)
    vy[J] = np.where(col, n2y, v2y)


def resolve_sequential(st: dict, P: np.ndarray) -> None:
    """The ascending Gauss-Seidel pass: resolve each pair of P in order, on the current state."""
    for i, j in P:
        _resolve_arrays(st, np.array([i]), np.array([j]))


def resolve_rounds(st: dict, P: np.ndarray) -> int:
    """The GPU kernel's schedule: per-body cursors over each body's pairs in key order; a round resolves every pair that is
    under the cursors of both its bodies.  Returns the number of rounds."""
    if len(P) == 0:
        return 0
    n = st["x"].shape[0]
    ends = np.concatenate([P, P[:, ::-1]])                 # (body, partner) for both ends
    order = np.lexsort((ends[:, 1], ends[:, 0]))
    ends = ends[order]
    deg = np.bincount(ends[:, 0], minlength=n)
    off = np.concatenate([[0], np.cumsum(deg)])
    partner = ends[:, 1]
    cur = np.zeros(n, np.int64)
    bodies = np.nonzero(deg)[0]
    rounds = 0
    while True:
        live = bodies[cur[bodies] < deg[bodies]]
        if live.size == 0:
            return rounds
        p = partner[off[live] + cur[live]]
        ok = cur[p] < deg[p]
        back = np.full(live.shape, -1)
        back[ok] = partner[off[p[ok]] + cur[p[ok]]]
        ready = back == live
        lo = ready & (live < p)
        _resolve_arrays(st, live[lo], p[lo])
        cur[live[ready]] += 1
        rounds += 1


def collide(st: dict, rounds: bool = True) -> int:
    """One collision pass on st (in place); returns |P|."""
    P = pairs(st["x"], st["y"], st["r"])
    (resolve_rounds if rounds else resolve_sequential)(st, P)
    return len(P)


def drift(st: dict, dt: float) -> None:
    """x += v * dt with two roundings (Simulation.hpp:160-163), for states whose kick is below half an ulp."""
    T = st["x"].dtype.type
    st["x"] = st["x"] + st["vx"] * T(dt)
    st["y"] = st["y"] + st["vy"] * T(dt)


def state_from_bodies(b: np.ndarray, dtype=np.float32) -> dict:
    return {"x": b["pos"][:, 0].astype(dtype), "y": b["pos"][:, 1].astype(dtype), "vx": b["vel"][:, 0].astype(dtype),
            "vy": b["vel"][:, 1].astype(dtype), "m": b["mass"].astype(dtype), "r": b["radius"].astype(np.float32)}


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
