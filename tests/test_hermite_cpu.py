"""CPU: NB_INTEGRATOR_HERMITE4 — the numpy model alone (tests/hermite_model.py: the jerk against a central difference of the
acceleration, the order of the step, the float32 bar of the pair terms) and what the library decides before it looks for a device."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hermite_model as hm  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"
EPS = 0.05
T = 2.0 ** -4
HERMITE4 = getattr(L, "NB_INTEGRATOR_HERMITE4", 5)

# The float32 bars, per component, in units of the cancellation-free scales S_a and S_j of hermite_model.acc_jerk_f64 (a rounding of one
# term is at most relative to the magnitudes that went into it, one of a partial sum at most relative to the sum of the magnitudes).
# Counted in units of u = 2^-24 (one rounding to nearest), first order, not tuned, for the 3-D term (the 2-D term has fewer):
#   d_c, dv_c               1 each (one subtraction of exact inputs)
#   r^2                     2 (d enters squared) + 3 (its fused multiply-adds; the partial sums are positive) = 5
#   inv                     5 / 2 + 2 (the hardware's reciprocal square root is good to 1 ulp = 2 u) = 4.5
#   inv2 = inv inv          2 x 4.5 + 1 = 10
#   s = (m inv) inv2        4.5 + 1 + 10 + 1 = 16.5
#   a term  s d_c           16.5 + 1 = 17.5 of |term|                     (the product's own rounding is counted with the run, below)
#   rv = d . dv             each product 1 + 1 + 1 = 3 of |d_k dv_k|, the two fused multiply-adds 1 each of the sum of the magnitudes:
#                           5 of RV = sum_k |d_k dv_k|
#   c = (-3 rv) inv2        5 + 1 + 10 + 1 = 17 of 3 RV inv2
#   t_c = fma(c, d_c, dv_c) (17 + 1) of |c d_c|, 1 of |dv_c|, and the fused multiply-add's 1 of both: at most 19 of
#                           T_c = |dv_c| + 3 RV |d_c| / R^2
#   j term  s t_c           19 + 16.5 = 35.5 of m T_c / R^3, which is the summand of S_j
#   a float32 run of 64     64 fused multiply-adds, each rounds a partial sum that is at most the run's share of S: 64
# The float64 sums across the runs add nothing visible.  81.5 u = 4.9e-6 for a, 99.5 u = 5.9e-6 for j.
BAR_A = (17.5 + 64) * 2.0 ** -24
BAR_J = (35.5 + 64) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def fixture1000():
    flat = np.load(GOLD / "ic_plummer_1024.npy")[:1000]
    return flat[:, 0:2].copy(), flat[:, 2:4].copy(), flat[:, 6].copy()


def cloud3(n=300, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (n, 3)).astype(np.float32), rng.normal(0, 0.5, (n, 3)).astype(np.float32),
            rng.uniform(0.5, 2.0, n).astype(np.float32) / n)


# ------------------------------------------------------------------------------------------------------- the model ---
@pytest.mark.parametrize("case", ["fixture-2d", "cloud-3d"])
def test_the_jerk_is_the_derivative_of_the_acceleration_along_the_flow(case):
    """Independent of the formula: j = (a(x + v delta) - a(x - v delta)) / (2 delta) in float64.  delta = 1e-5: the truncation is
    delta^2 / 6 of the third derivative along the flow, which for a softened pair is at most about 15 (|dv| / eps)^2 |j| (15: the
    largest coefficient in the third derivative of r^-3); with relative speeds up to 3 and eps = 0.05 that is
    (1e-5 x 3 / 0.05)^2 x 15 / 6 = 9e-7 of |j|.  The rounding, 1e-16 |a| / delta, is far below.  Bar: 1e-5 of max |j| per component."""
    x, v, m = fixture1000() if case == "fixture-2d" else cloud3()
    x, v = x.astype(np.float64), v.astype(np.float64)
    delta = 1e-5
    _, j = hm.acc_jerk_f64(x, v, m, EPS)
    ap, _ = hm.acc_jerk_f64(x + v * delta, v, m, EPS)
    am, _ = hm.acc_jerk_f64(x - v * delta, v, m, EPS)
    err = np.abs((ap - am) / (2 * delta) - j).max() / np.abs(j).max()
    print(f"{case}: max |central difference - j| / max |j| = {err:.3g} (bar 1e-5)")
    assert err <= 1e-5


@functools.lru_cache(maxsize=None)
def model_runs():
    """{k: (x, |dE/E|)} for k steps over T, and the 256-step reference positions."""
    x, v, m = fixture1000()
    e0 = hm.energy(x, v, m, EPS)
    out = {}
    for k in (4, 8, 16, 32, 256):
        xk, vk, _, _ = hm.run(x, v, m, EPS, [np.float32(T / k)] * k)
        out[k] = (xk, abs(hm.energy(xk, vk, m, EPS) - e0) / abs(e0))
    return out


def test_order_of_the_model():
    """The first 1000 fixture bodies over T = 2^-4 in 4, 8, 16, 32 steps against 256: halving the step divides the position error by
    about 16 (a third-order scheme gives 8)."""
    runs = model_runs()
    ref = runs[256][0]
    err = {k: np.abs(runs[k][0] - ref).max() for k in (4, 8, 16, 32)}
    for k in (4, 8, 16, 32):
        print(f"k {k}: position error {err[k]:.3g}, |dE/E| {runs[k][1]:.3g}")
    for k in (4, 8, 16):
        ratio = err[k] / err[2 * k]
        print(f"error({k}) / error({2 * k}) = {ratio:.3g}")
        assert ratio > 12
    de = [runs[k][1] for k in (4, 8, 16)]
    assert de[0] / de[1] > 12 and de[1] / de[2] > 12


@pytest.mark.parametrize("ulp", [0, 1])
def test_float32_restatement_meets_the_derived_bars(ulp):
    x, v, m = fixture1000()
    a, j, sa, sj = hm.acc_jerk_f64(x, v, m, EPS, scales=True)
    ga, gj = hm.acc_jerk_f32(x, v, m, EPS, ulp, np.random.default_rng(5))
    ea, ej = hm.err_over_scale(ga, a, sa), hm.err_over_scale(gj, j, sj)
    print(f"rsq +-{ulp} ulp: a / S_a max {ea.max():.3g} (bar {BAR_A:.3g}); j / S_j max {ej.max():.3g} (bar {BAR_J:.3g}); "
          f"of max |a| {np.abs(ga - a).max() / np.abs(a).max():.3g}, of max |j| {np.abs(gj - j).max() / np.abs(j).max():.3g}")
    assert ea.max() <= BAR_A and ej.max() <= BAR_J
    assert np.abs(ga - a).max() <= 1e-5 * np.abs(a).max() and np.abs(gj - j).max() <= 1e-5 * np.abs(j).max()   # the project's force bar


def test_float32_restatement_in_3d_and_without_softening():
    x, v, m = cloud3()
    x[7], x[200] = x[3], x[100]                                  # two pairs on one position
    for eps in (EPS, 0.0):
        a, j, sa, sj = hm.acc_jerk_f64(x, v, m, eps, scales=True)
        ga, gj = hm.acc_jerk_f32(x, v, m, eps)
        assert np.isfinite(a).all() and np.isfinite(j).all() and np.isfinite(ga).all() and np.isfinite(gj).all()
        assert hm.err_over_scale(ga, a, sa).max() <= BAR_A and hm.err_over_scale(gj, j, sj).max() <= BAR_J


def test_the_self_pair_adds_nothing_and_a_shared_position_only_its_formula():
    x = np.array([[0.0, 0.0], [0.0, 0.0], [3.0, 4.0]], np.float32)
    v = np.array([[1.0, 0.0], [0.0, 2.0], [0.0, 0.0]], np.float32)
    m = np.array([2.0, 5.0, 0.0], np.float32)
    e = hm.eps_of(EPS)
    a, j = hm.acc_jerk_f64(x, v, m, EPS)
    assert np.array_equal(a[0], [0.0, 0.0]) and np.allclose(j[0], np.array([-1.0, 2.0]) * 5.0 / e ** 3, rtol=1e-15)
    a, j = hm.acc_jerk_f64(x, v, m, 0.0)
    assert np.array_equal(a[:2], np.zeros((2, 2))) and np.array_equal(j[:2], np.zeros((2, 2)))


# ------------------------------------------------------------------------------------------------------ the library ---
def small_bodies(n=16):
    b = nb.bodies_array(n)
    b["mass"] = 1.0
    b["pos"][:, 0] = np.arange(n)
    return b


def hermite_params():
    p = L.default_params()
    p.integrator = HERMITE4
    return p


def test_abi_additions():
    header = (Path(__file__).resolve().parents[1] / "include" / "nbody.h").read_text()
    assert "NB_INTEGRATOR_HERMITE4 = 5" in header and "#define NB_ABI_VERSION 8" in header and "4 is unassigned" in header
    assert "int nb_jerks(nb_sim *s, double *acc, double *jerk);" in header
    assert L.NB_INTEGRATOR_HERMITE4 == 5 and nb.load().nb_abi_version() == 8


def test_the_value_4_is_still_refused():
    lib = nb.load()
    b = small_bodies()
    for value in (4, 6):
        p = L.default_params()
        p.integrator = value
        assert not lib.nb_create(b.ctypes.data, b.shape[0], C.byref(p))
        assert lib.nb_last_error_code() == L.NB_EINVAL and b"bad integrator" in lib.nb_last_error()


@pytest.mark.parametrize("change", [dict(), dict(precision=L.NB_FP64), dict(dims=3), dict(precision=L.NB_FP64, dims=3), dict(eps=0.0),
                                    dict(flags=L.NB_FLAG_MASS_SCALING | L.NB_FLAG_NO_UNIFORM_MASS | L.NB_FLAG_BODY_ORDER)])
def test_create_takes_a_hermite_handle_as_far_as_the_device(change):
    """Without a device nb_create gets as far as NB_ENODEVICE: the parameters were accepted.  With one it returns a handle."""
    lib = nb.load()
    b = small_bodies()
    p = hermite_params()
    for k, v in change.items():
        setattr(p, k, v)
    h = lib.nb_create(b.ctypes.data, b.shape[0], C.byref(p))
    if h:
        lib.nb_destroy(h)
    else:
        assert lib.nb_last_error_code() == L.NB_ENODEVICE, lib.nb_last_error()


REFUSED = [
    (dict(force=L.NB_FORCE_TREE), b"NB_FORCE_TREE"),
    (dict(shard_world=2, shard_rank=0), b"shard_world > 1"),
    (dict(i_begin=0, i_count=8), b"i_count < n"),
    (dict(flags=L.NB_FLAG_SHARD_SINGLE), b"NB_FLAG_SHARD_SINGLE"),
    (dict(flags=L.NB_FLAG_SHARD_ALLREDUCE), b"NB_FLAG_SHARD_ALLREDUCE"),
    (dict(extras=L.NB_EXTRA_VCLAMP), b"extras"),
    (dict(extras=L.NB_EXTRA_BOUNDARY), b"extras"),
    (dict(extras=L.NB_EXTRA_COLLIDE), b"extras"),
    (dict(sum_order=L.NB_SUM_SEQUENTIAL), b"NB_SUM_SEQUENTIAL"),
    (dict(rsqrt_mode=L.NB_RSQRT_QUAKE), b"NB_RSQRT_QUAKE"),
]


@pytest.mark.parametrize("change,partner", REFUSED, ids=[p.decode() + str(i) for i, (_, p) in enumerate(REFUSED)])
def test_create_refuses_the_partners_by_name_before_looking_for_a_device(change, partner):
    lib = nb.load()
    b = small_bodies()
    p = hermite_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert not lib.nb_create(b.ctypes.data, b.shape[0], C.byref(p)), change
    text = lib.nb_last_error()
    assert lib.nb_last_error_code() == L.NB_EINVAL and b"HERMITE4" in text and partner in text, (change, text)


def test_the_dump_header_round_trips_the_value(tmp_path):
    lib = nb.load()
    b = small_bodies(5)
    p = hermite_params()
    p.eps, p.dt = 0.25, 2.0 ** -7
    path = str(tmp_path / "hermite4.nbd").encode()
    L.check("nb_write_bodies", lib.nb_write_bodies(path, b.ctypes.data, 5, 7, C.byref(p)))
    n, frame, q = C.c_size_t(), C.c_uint64(), L.nb_params()
    L.check("nb_read_header", lib.nb_read_header(path, C.byref(n), C.byref(frame), C.byref(q)))
    assert (n.value, frame.value, q.integrator, q.eps, q.dt) == (5, 7, 5, 0.25, 2.0 ** -7)
    raw = bytearray(Path(path.decode()).read_bytes())
    for bad in (4, 6):
        raw[56:60] = bad.to_bytes(4, "little")                   # the integrator word of the 64-byte header
        Path(path.decode()).write_bytes(bytes(raw))
        assert lib.nb_read_header(path, None, None, None) == L.NB_EFORMAT


def test_jerks_on_a_null_handle_fails_cleanly():
    lib = nb.load()
    out = np.zeros(4)
    assert lib.nb_jerks(None, out.ctypes.data, out.ctypes.data) == L.NB_EINVAL
    assert b"nb_jerks" in lib.nb_last_error() and b"NULL handle" in lib.nb_last_error()


def test_the_simulation_keyword_maps_the_string():
    seen = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, k):
            return getattr(self._lib, k)

        def nb_create(self, bodies, n, params):
            seen.append(int(params._obj.integrator))
            return self._lib.nb_create(bodies, n, params)

    try:
        nb.Simulation(small_bodies(), eps=0.1, integrator="hermite4", library=Spy(nb.load())).close()
    except L.NBodyError as e:
        assert e.code == L.NB_ENODEVICE, e                       # accepted; there is no device here
    assert seen == [5] and callable(nb.Simulation.jerks)
