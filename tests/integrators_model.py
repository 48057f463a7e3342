"""The composed integrators of include/nbody.h (NB_INTEGRATOR_DKD, NB_INTEGRATOR_FR4) in numpy: the table of coefficients and one step.

A step of size h is a leading drift followed by stages; a stage is (force at the current x; v += a k h; x += v d h):

    integrator   leading drift   stages (k, d)
    dkd          1/2             (1, 1/2)
    fr4          theta/2         (theta, (1 - theta)/2), (1 - 2 theta, (1 - theta)/2), (theta, theta/2)      theta = 1 / (2 - 2^(1/3))

Every coefficient * h is formed in double from the float h the library's nb_step receives and rounded once to the handle's real.
"""
import numpy as np

THETA = 1.3512071919596576340476878089715           # 1 / (2 - 2^(1/3)): the literal of nb_capi.hip
LEAD = {"dkd": 0.5, "fr4": 0.5 * THETA}
STAGES = {
    "dkd": ((1.0, 0.5),),
    "fr4": ((THETA, 0.5 * (1.0 - THETA)), (1.0 - 2.0 * THETA, 0.5 * (1.0 - THETA)), (THETA, 0.5 * THETA)),
}


def scaled(c, h, dtype):
    """c * h as a launch receives it: h is a C float, the product is formed in double and rounded once to `dtype`."""
    return np.dtype(dtype).type(float(c) * float(np.float32(h)))


def steps_of(h, name, dtype):
    """(leading drift, ((kick, drift), ...)) of one step of size h, in `dtype`."""
    return scaled(LEAD[name], h, dtype), tuple((scaled(k, h, dtype), scaled(d, h, dtype)) for k, d in STAGES[name])


def axpy(y, a, s, dtype, strict):
    """y + a * s.  strict: the product and the sum each rounded to `dtype` (the library's strict form).  Otherwise, for float32,
    formed in double and rounded once — the library's fma up to a rare double rounding; for float64 the strict form (numpy has no
    fma), which is the fma exactly where a * s is exact, as with a power-of-two s."""
    dtype = np.dtype(dtype).type
    if strict or dtype is np.float64:
        return (y + (a * dtype(s)).astype(dtype)).astype(dtype)
    return (y.astype(np.float64) + a.astype(np.float64) * float(s)).astype(dtype)


def step(x, v, accel, h, name, dtype=np.float64, strict=True):
    """One step.  x, v: arrays of `dtype`; accel(x) -> a, an array of `dtype` and the shape of x.  Returns (x, v, a) with a the last
    stage's evaluation (what the library leaves in acc[])."""
    lead, stages = steps_of(h, name, dtype)
    x = axpy(np.asarray(x, dtype), np.asarray(v, dtype), lead, dtype, strict)
    v = np.asarray(v, dtype)
    a = None
    for hk, hd in stages:
        a = np.asarray(accel(x), dtype)
        v = axpy(v, a, hk, dtype, strict)
        x = axpy(x, v, hd, dtype, strict)
    return x, v, a


def accel_plain(x, m, eps):
    """The softened direct sum in fp64 with a plain numpy sum: a_i = sum_j m_j (x_j - x_i) / (|x_j - x_i|^2 + eps^2)^(3/2)."""
    x = np.asarray(x, np.float64)
    d = x[None, :, :] - x[:, None, :]
    w = np.asarray(m, np.float64)[None, :] * ((d * d).sum(-1) + eps * eps) ** -1.5
    return (d * w[:, :, None]).sum(1)
