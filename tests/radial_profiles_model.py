"""The numpy statement of nb_radial_profiles' contract (include/nbody.h): fp32 d2 with one rounding per operation, shells by the
squared edges, terms in fp64, and per (centre, shell, field) the math.fsum of the terms together with the sum of their magnitudes A.
The library's sums are held to |got - want| <= (count + 8) 2^-52 A: a sum of k terms in any fixed order is within (k - 1) 2^-53 of
the sum of |terms|, and every term carries a handful of roundings whose error in v_r is relative to |u|, not to |v_r|, which is
why A is built from magnitudes and not from the terms.  The order the library fixed is NOT restated here."""
import math

import numpy as np

FIELDS = ("mass", "mr", "mr2", "mvr", "mvr2", "mv2", "mlz")
PIECE = 1024                                   # candidates per piece of the library's sweep (PROFILES_PIECE): what the split tests size by


def squared_edges(edges):
    e = np.asarray(edges, np.float32)
    return e * e


def shells_of(d2, e2):
    """shell index per body, -1 where it lies in no shell (d2 fp32; NaN and +inf are in none)"""
    with np.errstate(invalid="ignore"):
        inside = (d2 >= e2[0]) & (d2 < e2[-1])
        b = (d2[:, None] >= e2[None, 1:]).sum(axis=1)
    return np.where(inside, b, -1)


def profiles(pos, vel, mass, centers, edges, vcenters=None):
    """pos, vel: (n, dims) float32 as nb_sync returns them; mass: (n,) float32; centers: (nc, dims); vcenters: (nc, dims) float64 or None.
    Returns count (nc, nbins) uint64, want (nc, nbins, 7) float64 and mag (nc, nbins, 7) float64, the fields in FIELDS' order."""
    pos, vel, mass = np.asarray(pos, np.float32), np.asarray(vel, np.float32), np.asarray(mass, np.float32)
    cen = np.asarray(centers, np.float32)
    dims = pos.shape[1]
    assert cen.ndim == 2 and cen.shape[1] == dims and vel.shape == pos.shape
    vc = np.zeros(cen.shape, np.float64) if vcenters is None else np.asarray(vcenters, np.float64)
    e2 = squared_edges(edges)
    nbins = e2.size - 1
    with np.errstate(invalid="ignore"):
        w = np.where(mass > 0, mass, np.float32(0)).astype(np.float64)
    p64, v64 = pos.astype(np.float64), vel.astype(np.float64)
    count = np.zeros((cen.shape[0], nbins), np.uint64)
    want = np.zeros((cen.shape[0], nbins, 7))
    mag = np.zeros((cen.shape[0], nbins, 7))
    for c in range(cen.shape[0]):
        with np.errstate(invalid="ignore", over="ignore"):
            d = pos - cen[c]                                              # fp32, one rounding per operation
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            if dims == 3:
                d2 = d2 + d[:, 2] * d[:, 2]
        shell = shells_of(d2, e2)
        sel = np.flatnonzero(shell >= 0)
        if sel.size == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            X = p64[sel] - cen[c].astype(np.float64)
            u = v64[sel] - vc[c]
            r2 = (X * X).sum(axis=1)
            r = np.sqrt(r2)
            on = r == 0
            safe = np.where(on, 1.0, r)
            vr = np.where(on, 0.0, (X * u).sum(axis=1) / safe)
            u2 = (u * u).sum(axis=1)
            umag = np.sqrt(u2)
            lz = np.where(on, 0.0, X[:, 0] * u[:, 1] - X[:, 1] * u[:, 0])
            ws = w[sel]
            zero = np.zeros_like(r)
            terms = np.stack([ws, np.where(on, zero, ws * r), np.where(on, zero, ws * r2), np.where(on, zero, ws * vr),
                              np.where(on, zero, ws * vr * vr), ws * u2, np.where(on, zero, ws * lz)], axis=1)
            mags = np.stack([ws, ws * r, ws * r2, ws * umag, ws * u2, ws * u2, ws * r * umag], axis=1)
        for b in np.unique(shell[sel]):
            rows = shell[sel] == b
            count[c, b] = int(rows.sum())
            for f in range(7):
                t, a = terms[rows, f], mags[rows, f]
                want[c, b, f] = math.fsum(t) if np.isfinite(t).all() else np.nan
                mag[c, b, f] = math.fsum(a) if np.isfinite(a).all() else np.inf
    return count, want, mag


def brute(pos, vel, mass, centers, edges, vcenters=None):
    """The same contract as a double loop in Python scalars (fp32 through numpy scalars); small inputs only."""
    pos, vel, mass = np.asarray(pos, np.float32), np.asarray(vel, np.float32), np.asarray(mass, np.float32)
    cen = np.asarray(centers, np.float32)
    dims = pos.shape[1]
    e2 = squared_edges(edges)
    nbins = e2.size - 1
    count = np.zeros((cen.shape[0], nbins), np.uint64)
    terms = [[[[] for _ in range(7)] for _ in range(nbins)] for _ in range(cen.shape[0])]
    for c in range(cen.shape[0]):
        vc = [0.0] * dims if vcenters is None else [float(v) for v in np.asarray(vcenters, np.float64)[c]]
        for j in range(pos.shape[0]):
            d = [pos[j, k] - cen[c, k] for k in range(dims)]              # numpy float32 scalars: fp32 arithmetic
            d2 = d[0] * d[0] + d[1] * d[1]
            if dims == 3:
                d2 = d2 + d[2] * d[2]
            if not (d2 >= e2[0] and d2 < e2[-1]):
                continue
            b = sum(1 for t in range(1, nbins + 1) if d2 >= e2[t])
            m = float(mass[j])
            w = m if m > 0 else 0.0
            X = [float(pos[j, k]) - float(cen[c, k]) for k in range(dims)]
            u = [float(vel[j, k]) - vc[k] for k in range(dims)]
            r2 = sum(a * a for a in X)
            r = math.sqrt(r2)
            u2 = sum(a * a for a in u)
            count[c, b] += 1
            if r == 0:
                vals = [w, 0.0, 0.0, 0.0, 0.0, w * u2, 0.0]
            else:
                vr = sum(a * q for a, q in zip(X, u)) / r
                vals = [w, w * r, w * r2, w * vr, w * vr * vr, w * u2, w * (X[0] * u[1] - X[1] * u[0])]
            for f in range(7):
                terms[c][b][f].append(vals[f])
    want = np.array([[[math.fsum(terms[c][b][f]) for f in range(7)] for b in range(nbins)] for c in range(cen.shape[0])]).reshape(cen.shape[0], nbins, 7)
    return count, want


def bar(count, mag):
    """the bound on |got - want| per (centre, shell, field)"""
    return (count[..., None].astype(np.float64) + 8.0) * 2.0 ** -52 * mag


def mismatches(got, model, what=""):
    """got: a (nc, nbins) SHELL_DTYPE-like structured array; model: profiles' triple.  A list of messages, empty when the counts are equal
    and every double is inside the bar (a field whose magnitude sum is not finite is not compared: the arithmetic gives what it gives)."""
    count, want, mag = model
    out = []
    if got.shape != count.shape:
        return [f"{what}: shape {got.shape} vs {count.shape}"]
    bad = np.argwhere(got["count"] != count)
    if bad.size:
        c, b = bad[0]
        out.append(f"{what}: {bad.shape[0]} counts differ, first centre {c} shell {b}: {got['count'][c, b]} vs {count[c, b]}")
    tol = bar(count, mag)
    for f, name in enumerate(FIELDS):
        g = got[name]
        ok = ~np.isfinite(mag[..., f]) | (np.abs(g - want[..., f]) <= tol[..., f])
        bad = np.argwhere(~ok)
        if bad.size:
            c, b = bad[0]
            out.append(f"{what}: {name}: {bad.shape[0]} outside the bar, first centre {c} shell {b}: {g[c, b]!r} vs {want[c, b, f]!r} "
                       f"(bar {tol[c, b, f]:.3g}, count {count[c, b]})")
    return out


def worst(got, model):
    """the largest |got - want| / bar over all compared doubles (0 where nothing is compared): what a test prints before it asserts"""
    count, want, mag = model
    tol = bar(count, mag)
    w = 0.0
    for f, name in enumerate(FIELDS):
        use = np.isfinite(mag[..., f]) & (tol[..., f] > 0)
        if use.any():
            w = max(w, float((np.abs(got[name] - want[..., f])[use] / tol[..., f][use]).max()))
    return w
