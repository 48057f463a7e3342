"""The numpy statement of nb_group_binding's contract (include/nbody.h), on top of tests/groups_model.py (the groups),
tests/group_catalog_model.py (the rows, ``vel`` and its bound) and tests/potential_model.py (``phi_f64``).  Per kept group G:

    phi[i] = potential_model.phi_f64 of the members alone     - sum_{j in G, j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2)
    e[i]   = 1/2 |v_i - vel_G|^2 + phi[i]                      vel_G the catalogue model's
    bound = #(e < 0)     most_bound = the first index of the smallest e     e_min     potential = 1/2 fsum(w_i phi[i])

and NaN in both planes for a body whose group is not kept.

THE ORDER OF THE DEVICE'S SUMS (stated here, not repeated by the model, whose bars hold for any order).  The bodies are sorted by
(label, index); a group is a segment [s, s + k) of sorted positions.  The positions are cut into runs [64 r, 64 r + 64).  On an fp32
handle phi of the body at position p is  0 - (((S_a + S_a+1) + ...) + S_b)  in float64, over the runs a .. b that meet the segment in
ascending r, where S_r is the float32 sum, started at 0 and taken in ascending position j by fused multiply-add m_j * inv + S, of the
members j != p in run r: at most 64 terms.  On an fp64 handle it is one float64 sum over j = s .. s + k - 1, j != p, in that order.  The
records are a segmented scan over the sorted order in the catalogue's tree (tests/group_catalog_model.py).

THE BARS, none of them measured.  U = 2^-52, k = members.
    bar_phi  fp32 handle, masses >= 0: 4e-6 |phi|, nb_potentials' bar (tests/potential_model.py: every term within 3 float32 roundings
             and 1 ulp of v_rsq_f32, runs of <= 64 terms of one sign, the rest in float64).
             fp64 handle: (k + 8) U sum |terms|: a float64 sum of k terms in any order is within (k - 1) 2^-53 sum |terms| of the exact
             one, and the 8 covers what a term carries on both sides (displacement, two or three fused multiply-adds, rsqrt_f64 at
             1.4e-16, the product; the model's square root and quotient).
    bar_e    bar_phi + |v - V| d_V + 1/2 d_V^2 + 8 U (1/2 |v - V|^2 + |phi|),  d_V the norm of the catalogue model's bound on vel
    potential    1/2 sum w_i bar_phi[i] + (k + 8) U 1/2 sum |w_i phi_i|
    e_min        the largest bar_e of the group
The discrete fields are held to windows, so that no input needs a lucky margin:
    #(e < -bar_e) <= bound <= #(e < +bar_e);     most_bound is a member with e[most_bound] <= min e + 2 max bar_e.
``window_widths`` gives hi - lo per group: the tests require it to be at most max(1, members / 1000) BEFORE they look at the device, so
that the windows cannot hide a failure.
"""
import math
from types import SimpleNamespace

import numpy as np

import group_catalog_model as cm
import groups_model as gm
import potential_model as pm

U = 2.0 ** -52
DTYPE = np.dtype([("label", np.uint32), ("members", np.uint32), ("bound", np.uint32), ("most_bound", np.uint32),
                  ("e_min", np.float64), ("potential", np.float64)])
NONE = 0xFFFFFFFF


def binding(bodies, radius, min_members, eps, dims=2, label=None, fp64=False):
    """The model of ``bodies`` (BODY_DTYPE or BODY3_DTYPE records): a namespace with the planes ``phi``, ``e`` and their bars
    ``bar_phi``, ``bar_e`` (n,), the records ``rec`` (DTYPE), per row ``bar_potential``, ``bar_e_min``, ``lo``, ``hi`` (the window of
    ``bound``) and ``idx`` (the members' indices, ascending), and ``kept`` (n,) bool.  ``label``: groups_model's answer, if the caller
    has it.  ``fp64``: the bars of an NB_FP64 handle."""
    b = np.asarray(bodies)
    n = b.shape[0]
    x, v, m = cm.state_of(b, dims)
    if label is None:
        label = gm.groups(b["pos"][:, 0], b["pos"][:, 1], radius)[0]
    label = np.asarray(label, np.int64)
    cat, cbound = cm.catalog(b, radius, min_members, dims, label)
    order = np.argsort(label, kind="stable")
    heads = np.flatnonzero(np.r_[True, label[order][1:] != label[order][:-1]])
    ends = np.r_[heads[1:], n]
    keep = [(h, t) for h, t in zip(heads, ends) if t - h >= min_members]
    assert len(keep) == cat.shape[0]
    out = SimpleNamespace(phi=np.full(n, np.nan), e=np.full(n, np.nan), bar_phi=np.full(n, np.nan), bar_e=np.full(n, np.nan),
                          kept=np.zeros(n, bool), rec=np.zeros(len(keep), DTYPE), bar_potential=np.zeros(len(keep)),
                          bar_e_min=np.zeros(len(keep)), lo=np.zeros(len(keep), np.int64), hi=np.zeros(len(keep), np.int64), idx=[])
    e2 = pm.eps_of(eps) ** 2
    for row, (h, t) in enumerate(keep):
        idx = order[h:t]
        k = idx.size
        assert cat["label"][row] == idx[0] and cat["members"][row] == k
        w = np.where(m[idx] > 0, m[idx], 0.0)
        with np.errstate(all="ignore"):
            phi = pm.phi_f64(x[idx], m[idx], eps) + 0.0          # (0 - s: a sum of nothing is +0, not phi_f64's -0)
            if fp64:
                mag = np.empty(k)
                for a in range(k):                                   # sum |terms| of member a
                    d = x[idx] - x[idx[a]]
                    tt = np.abs(m[idx]) / np.sqrt(np.einsum("ij,ij->i", d, d) + e2)
                    tt[a] = 0.0
                    mag[a] = math.fsum(tt)
                bar_phi = (k + 8) * U * mag
            else:
                bar_phi = 4e-6 * np.abs(phi)
            dv = v[idx] - cat["vel"][row][:dims]
            dv2 = (dv * dv).sum(axis=1)
            e = 0.5 * dv2 + phi
            d_v = float(np.linalg.norm(cbound["vel"][row]))
            bar_e = bar_phi + np.sqrt(dv2) * d_v + 0.5 * d_v * d_v + 8 * U * (0.5 * dv2 + np.abs(phi))
            out.phi[idx], out.e[idx], out.bar_phi[idx], out.bar_e[idx] = phi, e, bar_phi, bar_e
            out.kept[idx] = True
            r = out.rec[row]
            r["label"], r["members"] = idx[0], k
            r["bound"] = int((e < 0).sum())
            ordered = ~np.isnan(e)
            if ordered.any() and np.nanmin(e) < np.inf:
                at = int(np.flatnonzero(e == np.nanmin(e))[0])
                r["most_bound"], r["e_min"] = idx[at], e[at]
            else:
                r["most_bound"], r["e_min"] = NONE, np.inf
            wp = w * phi
            r["potential"] = 0.5 * math.fsum(wp) if np.isfinite(wp).all() else 0.5 * float(np.sum(wp))
            out.bar_potential[row] = 0.5 * float(np.sum(w * bar_phi)) + (k + 8) * U * 0.5 * float(np.sum(np.abs(wp)))
            out.bar_e_min[row] = float(np.max(bar_e))
            out.lo[row], out.hi[row] = int((e < -bar_e).sum()), int((e < bar_e).sum())
        out.idx.append(idx)
    return out


def window_widths(model):
    """hi - lo of every group's ``bound`` window, and what the tests allow it to be: max(1, members / 1000)."""
    return model.hi - model.lo, np.maximum(1, model.rec["members"] // 1000)


def windows_are_tight(model):
    width, allowed = window_widths(model)
    return bool((width <= allowed).all())


def mismatches(model, phi=None, e=None, rec=None, scale=1.0):
    """Descriptions of everything in the library's answer that is not the model's.  ``phi`` / ``e``: the planes, NaN exactly where the
    model has NaN, within ``scale`` x the bars elsewhere.  ``rec``: label, members exactly; potential and e_min within their bars; bound
    inside its window; most_bound a member whose model e is within 2 max bar_e of the minimum.  With ``e`` and ``rec`` both given, the
    records are also held to the device's own plane: e[most_bound] == e_min == the minimum over the members, bound == #(e < 0)."""
    out = []
    for name, got, want, bar in (("phi", phi, model.phi, model.bar_phi), ("e", e, model.e, model.bar_e)):
        if got is None:
            continue
        if got.shape != want.shape or got.dtype != np.float64:
            out.append(f"{name}: shape {got.shape} dtype {got.dtype}")
            continue
        nan = np.isnan(got)
        if not np.array_equal(nan, ~model.kept):
            out.append(f"{name}: NaN on {int(nan.sum())} bodies, {int((~model.kept).sum())} belong to no kept group")
            continue
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(model.kept & ~((np.abs(got - want) <= scale * bar) | (got == want)))
        if bad.size:
            i = bad[0]
            out.append(f"{name}: {bad.size} bodies out of bar, first body {i}: {got[i]!r} vs {want[i]!r}, bar {bar[i]!r}")
    if rec is None:
        return out
    if rec.shape != model.rec.shape:
        return out + [f"{rec.shape[0]} records, the model has {model.rec.shape[0]}"]
    for f in ("label", "members"):
        bad = np.flatnonzero(rec[f] != model.rec[f])
        if bad.size:
            out.append(f"{f}: {bad.size} differ, first row {bad[0]}: {rec[f][bad[0]]} vs {model.rec[f][bad[0]]}")
    for row in range(rec.shape[0]):
        r, w, idx = rec[row], model.rec[row], model.idx[row]
        tag = f"row {row} (label {w['label']}, {w['members']} members)"
        if not abs(r["potential"] - w["potential"]) <= scale * model.bar_potential[row]:
            out.append(f"{tag}: potential {r['potential']!r} vs {w['potential']!r}, bar {model.bar_potential[row]!r}")
        if not (abs(r["e_min"] - w["e_min"]) <= scale * model.bar_e_min[row] or r["e_min"] == w["e_min"]):
            out.append(f"{tag}: e_min {r['e_min']!r} vs {w['e_min']!r}, bar {model.bar_e_min[row]!r}")
        if not model.lo[row] <= r["bound"] <= model.hi[row]:
            out.append(f"{tag}: bound {r['bound']} outside {model.lo[row]} .. {model.hi[row]}")
        mb = int(r["most_bound"])
        if mb == NONE or w["most_bound"] == NONE:
            if mb != w["most_bound"]:
                out.append(f"{tag}: most_bound {mb} vs {w['most_bound']}")
        elif mb not in idx:
            out.append(f"{tag}: most_bound {mb} is no member")
        elif not model.e[mb] <= w["e_min"] + 2 * scale * model.bar_e_min[row]:
            out.append(f"{tag}: most_bound {mb} has model e {model.e[mb]!r}, the minimum is {w['e_min']!r}, bar {model.bar_e_min[row]!r}")
        if e is not None and mb != NONE and mb in idx:
            own = e[idx]
            if not (e[mb] == r["e_min"] and np.nanmin(own) == r["e_min"]):
                out.append(f"{tag}: e_min {r['e_min']!r}, the plane has {e[mb]!r} at most_bound and a minimum of {np.nanmin(own)!r}")
            if int((own < 0).sum()) != r["bound"]:
                out.append(f"{tag}: bound {r['bound']}, the plane has {int((own < 0).sum())} members with e < 0")
            first = idx[np.flatnonzero(own == r["e_min"])[0]]
            if first != mb:
                out.append(f"{tag}: most_bound {mb}, the first member with the smallest e is {first}")
        if len(out) > 8:
            break
    return out
