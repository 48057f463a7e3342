"""numpy statement of the two direct forms of nb_field (include/nbody.h), used by the field tests.  With d = x_j - p:

    phi(p) = - sum_j m_j / sqrt(|d|^2 + eps^2)        acc(p) = sum_j m_j d / (|d|^2 + eps^2)^(3/2)

A point is not a body: there is no self term.  A point on a body takes -m_j / eps into phi and nothing into acc (d = 0); with
eps = 0 a pair whose r^2 is exactly 0 adds nothing to either output.

``field_f64``   brute force in float64 from the values the handle holds (float32 inputs stay float32 values, eps is the float32 the
                handle holds): phi, acc and, per component of acc, the cancellation-free scale S = sum_j |term_j|, the quantity the
                fp32 arithmetic is bounded against.
``field_f32``   the fp32 sweep of field_tiled_f32 (nbodysim_amd/csrc/nb_field.hip.h): float32 displacement, r^2 by fused
                multiply-adds onto eps^2, inv = a float32 reciprocal square root, phi += m_j inv and, with inv2 = inv inv and
                s = m_j (inv2 inv), a_c += d_c s, each a fused multiply-add into a float32 run over 64 consecutive j (a run starts
                at every multiple of 64 from j = 0), the runs added in float64 per wave (run k belongs to wave k mod 4) and the four
                waves in order: ((S0 + S1) + S2) + S3.  ``rsq_ulp`` perturbs the correctly rounded reciprocal square root by up to
                that many ulps with ``rng``, as potential_model.phi_f32 does for the hardware's 1-ulp v_rsq_f32.
"""
from __future__ import annotations

import numpy as np

from potential_model import D, F, RUN, WAVES, _fma32, eps_of


def field_f64(points, pos, m, eps):
    """points (k, d), pos (n, d), m (n,), any float dtype: (phi (k,), acc (k, d), S (k, d)) in float64, point by point."""
    q = np.asarray(points).astype(D)
    p = np.asarray(pos).astype(D)
    w = np.asarray(m).astype(D)
    e2 = eps_of(eps) ** 2
    k, dims = q.shape
    phi, acc, scale = np.zeros(k, D), np.zeros((k, dims), D), np.zeros((k, dims), D)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(k):
            d = p - q[i]
            r2 = np.einsum("ij,ij->i", d, d) + e2
            inv = np.where(r2 > 0, 1.0 / np.sqrt(r2), 0.0)
            phi[i] = -np.sum(w * inv)
            t = d * (w * inv ** 3)[:, None]
            acc[i] = t.sum(0)
            scale[i] = np.abs(t).sum(0)
    return phi, acc, scale


def field_f32(points, pos, m, eps, rsq_ulp: int = 0, rng=None):
    """The fp32 form (see above) at points (k, d) float32 for pos (n, d) float32, m (n,) float32: (phi (k,), acc (k, d)) float64."""
    q = np.ascontiguousarray(points, F)
    p = np.ascontiguousarray(pos, F)
    w = np.ascontiguousarray(m, F)
    n, dims = p.shape
    k = q.shape[0]
    e2 = F(F(eps) * F(eps))
    guard = not e2 > 0
    waves = np.zeros((WAVES, 1 + dims, k), D)
    with np.errstate(all="ignore"):
        for r, j0 in enumerate(range(0, n, RUN)):
            run = np.zeros((1 + dims, k), F)
            for j in range(j0, min(j0 + RUN, n)):
                r2 = np.full(k, e2, F)
                d = []
                for c in range(dims):
                    d.append((p[j, c] - q[:, c]).astype(F))
                    r2 = _fma32(d[c], d[c], r2)
                inv = (1.0 / np.sqrt(r2.astype(D))).astype(F)
                if rsq_ulp:
                    step = rng.integers(-rsq_ulp, rsq_ulp + 1, k)
                    inv = (inv.view(np.int32) + step.astype(np.int32)).view(F)
                if guard:
                    inv = np.where(r2 == 0, F(0), inv)
                mj = np.full(k, w[j], F)
                run[0] = _fma32(mj, inv, run[0])
                s = (mj * ((inv * inv).astype(F) * inv).astype(F)).astype(F)
                for c in range(dims):
                    run[1 + c] = _fma32(d[c], s, run[1 + c])
            waves[r % WAVES] += run.astype(D)
    tot = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    return 0.0 - tot[0], np.ascontiguousarray(tot[1:].T)


def acc_err(got, want, scale) -> np.ndarray:
    """|got - want| / S per component (absolute where S is 0)."""
    got, want, scale = np.asarray(got, D), np.asarray(want, D), np.asarray(scale, D)
    return np.abs(got - want) / np.where(scale != 0, scale, 1.0)
