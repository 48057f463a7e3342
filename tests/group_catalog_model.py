"""The numpy statement of nb_group_catalog's contract (include/nbody.h), on top of tests/groups_model.py: the groups are that model's;
every sum is ``math.fsum``, so the model's values are the exact ones, correctly rounded.  Beside each value stands the bound the
library is held to.  None of the bounds is measured: each follows from the fact that an fp64 sum of k terms in ANY order differs from
the exact sum by at most (k - 1) 2^-53 sum |terms| to first order.  With k = members:

    mass and every sum of w x or w v     k 2^-52 sum |terms|
    pos, vel                             that bound / W  +  2^-52 |value|           (the division)
    sigma2, d = bound on |vel|           2 sqrt(sigma2) d + d^2 + (k + 8) 2^-52 sigma2
    r_max                                the bound on |pos|  +  8 2^-52 r_max
"""
import math

import numpy as np

import groups_model as gm

U = 2.0 ** -52
FIELDS = ("mass", "pos", "vel", "sigma2", "r_max")
DTYPE = np.dtype([("label", np.uint32), ("members", np.uint32), ("mass", np.float64), ("pos", np.float64, 3), ("vel", np.float64, 3),
                  ("sigma2", np.float64), ("r_max", np.float64)])


def state_of(bodies, dims=2):
    """(x, v, m): float64 (n, dims) positions and velocities and float64 masses, holding the float32 values of the records."""
    b = np.asarray(bodies)
    x = np.array(b["pos"][:, :dims], np.float32).astype(np.float64)
    v = np.array(b["vel"][:, :dims], np.float32).astype(np.float64)
    m = np.array(b["mass"], np.float32).astype(np.float64)
    return x, v, m


def one_group(x, v, m):
    """(values, bounds) of ONE group given its members' (k, dims) x and v and (k,) m: dicts with the double fields of nb_group."""
    k, dims = x.shape
    w = np.where(m > 0, m, 0.0)
    mass = math.fsum(w)
    b_mass = k * U * math.fsum(np.abs(w))
    heavy = mass > 0
    ww = w if heavy else np.ones(k)
    W = mass if heavy else float(k)
    val = {"mass": mass, "pos": np.zeros(3), "vel": np.zeros(3)}
    bnd = {"mass": b_mass, "pos": np.zeros(3), "vel": np.zeros(3)}
    with np.errstate(invalid="ignore", over="ignore"):
        for name, a in (("pos", x), ("vel", v)):
            for d in range(dims):
                terms = ww * a[:, d]                               # exact: 24 x 24 bits
                val[name][d] = math.fsum(terms) / W
                bnd[name][d] = k * U * math.fsum(np.abs(terms)) / W + U * abs(val[name][d])
        dv = v - val["vel"][:dims]
        dx = x - val["pos"][:dims]
        sigma2 = math.fsum(ww * (dv * dv).sum(axis=1)) / W
        r_max = math.sqrt(float((dx * dx).sum(axis=1).max()))
    d_vel, d_pos = float(np.linalg.norm(bnd["vel"])), float(np.linalg.norm(bnd["pos"]))
    val["sigma2"], val["r_max"] = sigma2, r_max
    bnd["sigma2"] = 2.0 * math.sqrt(sigma2) * d_vel + d_vel * d_vel + (k + 8) * U * sigma2
    bnd["r_max"] = d_pos + 8 * U * r_max
    return val, bnd


def catalog(bodies, radius, min_members, dims=2, label=None):
    """(cat, bound): two DTYPE arrays, one record per group of at least ``min_members`` bodies in ascending order of label; ``bound``
    holds, in the double fields, what the library's value may differ from ``cat``'s by.  ``label``: the groups, if the caller has
    groups_model's answer for these bodies and this radius already."""
    b = np.asarray(bodies)
    x, v, m = state_of(b, dims)
    if label is None:
        label = gm.groups(b["pos"][:, 0], b["pos"][:, 1], radius)[0]
    label = np.asarray(label, np.int64)
    order = np.argsort(label, kind="stable")                       # members in ascending index behind their label
    heads = np.flatnonzero(np.r_[True, label[order][1:] != label[order][:-1]])
    ends = np.r_[heads[1:], label.size]
    keep = [(h, e) for h, e in zip(heads, ends) if e - h >= min_members]
    cat, bound = np.zeros(len(keep), DTYPE), np.zeros(len(keep), DTYPE)
    for row, (h, e) in enumerate(keep):
        idx = order[h:e]
        val, bnd = one_group(x[idx], v[idx], m[idx])
        cat[row]["label"] = bound[row]["label"] = label[idx[0]]
        cat[row]["members"] = bound[row]["members"] = e - h
        for f in FIELDS:
            cat[row][f], bound[row][f] = val[f], bnd[f]
    return cat, bound


def mismatches(got, cat, bound, scale=1.0):
    """Descriptions of everything in the library's records ``got`` that is not the model's: label and members exactly, the double
    fields within ``scale`` x the bound (NaN where the model has NaN)."""
    out = []
    if got.shape != cat.shape:
        return [f"{got.shape[0]} records, the model has {cat.shape[0]}"]
    if got.shape[0] == 0:
        return out
    for f in ("label", "members"):
        bad = np.flatnonzero(got[f] != cat[f])
        if bad.size:
            out.append(f"{f}: {bad.size} differ, first row {bad[0]}: {got[f][bad[0]]} vs {cat[f][bad[0]]}")
    for f in FIELDS:
        g, w, b = (np.asarray(a[f], np.float64).reshape(got.shape[0], -1) for a in (got, cat, bound))
        with np.errstate(invalid="ignore"):
            ok = (np.abs(g - w) <= scale * b) | (np.isnan(g) & np.isnan(w)) | (g == w)
        bad = np.flatnonzero(~ok.all(axis=1))
        if bad.size:
            r = bad[0]
            out.append(f"{f}: {bad.size} rows out of bound, first row {r} (label {cat['label'][r]}, {cat['members'][r]} members): "
                       f"{g[r].tolist()} vs {w[r].tolist()}, bound {b[r].tolist()}")
    return out
