"""numpy statement of the two direct forms of nb_potentials (include/nbody.h), used by the potential tests.

    phi_i = - sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2)         (the self term is left out by INDEX)

``phi_f64``   brute force in float64 from the values the handle holds (float32 inputs stay float32 values, eps is the float32 the
              handle holds): what an NB_FP64 handle computes to rounding, and the yardstick of the fp32 form.
``phi_f32``   the fp32 sweep of potential_tiled_f32 (nbodysim_amd/csrc/nb_potential.hip.h): float32 displacement, r^2 by fused
              multiply-adds onto eps^2, a float32 reciprocal square root, the terms m_j / r added by fused multiply-add into a
              float32 run over 64 consecutive j (a run starts at every multiple of 64 from j = 0), the runs added in float64 per
              wave (run k belongs to wave k mod 4) and the four waves in order: ((S0 + S1) + S2) + S3.
              The hardware's v_rsq_f32 is within 1 ulp of the exact value and is not restated bit for bit: ``rsq_ulp`` perturbs the
              correctly rounded value by that many ulps with the given ``rng`` (uniformly -rsq_ulp .. +rsq_ulp), which is how the
              4e-6 bar of the tests is probed.
"""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64
RUN = 64          # terms of a float32 run: one wave's share of an LDS tile of 256
WAVES = 4


def eps_of(eps) -> float:
    return float(F(eps))


def phi_f64(pos, m, eps) -> np.ndarray:
    """pos (n, d) and m (n,), any float dtype: phi in float64, row by row."""
    p = np.asarray(pos).astype(D)
    w = np.asarray(m).astype(D)
    n = p.shape[0]
    e2 = eps_of(eps) ** 2
    out = np.zeros(n, D)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            d = p - p[i]
            t = w / np.sqrt(np.einsum("ij,ij->i", d, d) + e2)
            t[i] = 0.0
            out[i] = -np.sum(t)
    return out


def _fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32."""
    return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)


def phi_f32(pos, m, eps, rsq_ulp: int = 0, rng=None) -> np.ndarray:
    """The fp32 form (see above) for every body of pos (n, d) float32, m (n,) float32; the result is float64."""
    p = np.ascontiguousarray(pos, F)
    w = np.ascontiguousarray(m, F)
    n, dims = p.shape
    e2 = F(F(eps) * F(eps))
    idx = np.arange(n)
    waves = np.zeros((WAVES, n), D)
    with np.errstate(all="ignore"):
        for k, j0 in enumerate(range(0, n, RUN)):
            run = np.zeros(n, F)
            for j in range(j0, min(j0 + RUN, n)):
                r2 = np.full(n, e2, F)
                for c in range(dims):
                    d = (p[j, c] - p[:, c]).astype(F)
                    r2 = _fma32(d, d, r2)
                inv = (1.0 / np.sqrt(r2.astype(D))).astype(F)
                if rsq_ulp:
                    step = rng.integers(-rsq_ulp, rsq_ulp + 1, n)
                    inv = (inv.view(np.int32) + step.astype(np.int32)).view(F)
                inv = np.where(idx == j, F(0), inv)
                run = _fma32(np.full(n, w[j], F), inv, run)
            waves[k % WAVES] += run.astype(D)
    return -(((waves[0] + waves[1]) + waves[2]) + waves[3])


def rel_err(got, want) -> np.ndarray:
    """|got - want| / |want| per body (absolute where want is 0)."""
    got, want = np.asarray(got, D), np.asarray(want, D)
    den = np.where(want != 0, np.abs(want), 1.0)
    return np.abs(got - want) / den
