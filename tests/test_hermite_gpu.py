"""GPU: NB_INTEGRATOR_HERMITE4 (include/nbody.h) — nb_jerks against the fp64 model (tests/hermite_model.py) at the sizes where the
kernels change path, the trajectory and its order against the model, and the state a handle carries between steps.

One process; after a HIP error nothing more is started.  Every reference is computed once and shared.
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import max_rel

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hermite_model as hm  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
EPS = 0.05
HF = 2e-3
T = 2.0 ** -4
BAR_A = (17.5 + 64) * 2.0 ** -24      # fp32, of S_a per component: tests/test_hermite_cpu.py has the derivation
BAR_J = (35.5 + 64) * 2.0 ** -24      # fp32, of S_j per component: the same
BAR_F64 = 1e-12                       # of S: n x 1.1e-16 of sequential float64 adds (n <= 1000) + the 1.4e-16 reciprocal square root
#                                       (tests/test_field_gpu.py's reasoning) + under 40 roundings of 1.1e-16 in a term
SIZES = (1, 2, 63, 64, 65, 127, 129, 255, 256, 257, 1000, 5693)     # wave, i-tile and j-tile edges, the padded tail, several tiles
_HIP_ERROR = []


@pytest.fixture(autouse=True)
def _stop_after_a_hip_error():
    """Remember a HIP error so that no later test of this module touches the GPU."""
    if _HIP_ERROR:
        pytest.fail(f"not run: an earlier test of this module met a HIP error ({_HIP_ERROR[0]})")


class watched:
    """Remember a HIP error raised inside the block."""

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is not None and issubclass(et, nb.NBodyError) and getattr(ev, "code", 0) == L.NB_EHIP:
            _HIP_ERROR.append(str(ev))
        return False


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    bad = np.argwhere(bits(a) != bits(b))
    assert bad.size == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def bodies_of(x, v, m):
    x = np.asarray(x, np.float32)
    n, dims = x.shape
    b = nb.bodies_array(n)
    if dims == 3:
        b = b.view(nb.BODY3_DTYPE)
    b["pos"], b["vel"], b["mass"], b["radius"] = x, np.asarray(v, np.float32), np.asarray(m, np.float32), 1.0
    return b


def hermite(b, eps=EPS, **kw):
    dims = b["pos"].shape[1]
    return nb.Simulation(b, eps=eps, integrator="hermite4", **(dict(dims=3, **kw) if dims == 3 else kw))


@functools.lru_cache(maxsize=None)
def cloud(n, dims):
    """Individual masses, 64 massless bodies (from 129 bodies on), the last body on the position of the first with another velocity."""
    rng = np.random.default_rng(100 * dims + n)
    x = rng.normal(0, 1, (n, dims)).astype(np.float32)
    v = rng.normal(0, 0.5, (n, dims)).astype(np.float32)
    m = (rng.uniform(0.5, 2.0, n) / n).astype(np.float32)
    if n >= 129:
        m[1:n - 1:(n - 2) // 64][:64] = 0.0
    if n >= 3:
        x[n - 1] = x[0]
    return x, v, m


@functools.lru_cache(maxsize=None)
def want(n, dims, eps):
    return hm.acc_jerk_f64(*cloud(n, dims), eps, scales=True)


def check_planes(got, ref, bar_a, bar_j, what):
    a, j, sa, sj = ref
    assert got[0].dtype == np.float64 and got[0].shape == a.shape and got[1].shape == j.shape, what
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), what
    ea, ej = hm.err_over_scale(got[0], a, sa).max(), hm.err_over_scale(got[1], j, sj).max()
    print(f"{what}: a / S_a {ea:.3g} (bar {bar_a:.3g}), j / S_j {ej:.3g} (bar {bar_j:.3g})")
    assert ea <= bar_a and ej <= bar_j, (what, ea, ej)


# ----------------------------------------------------------------------------------------- nb_jerks against the model ---
@pytest.mark.parametrize("precision,dims", [("fp32", 2), ("fp32", 3), ("fp64", 2), ("fp64", 3)])
def test_jerks_against_the_fp64_model(precision, dims):
    """Every size, eps > 0: individual masses, massless bodies, two bodies on one position (the formula's m dv / eps^3 in the jerk)."""
    bars = (BAR_A, BAR_J) if precision == "fp32" else (BAR_F64, BAR_F64)
    with watched():
        for n in SIZES:
            if precision == "fp64" and n > 1000:
                continue
            x, v, m = cloud(n, dims)
            with hermite(bodies_of(x, v, m), precision=precision) as sim:
                got = sim.jerks()
            check_planes(got, want(n, dims, EPS), *bars, f"{precision} {dims}-D n {n}")
            if n == 1:
                assert not got[0].any() and not got[1].any()             # the self pair adds exactly 0


@pytest.mark.parametrize("precision,dims", [("fp32", 2), ("fp32", 3), ("fp64", 2), ("fp64", 3)])
def test_jerks_without_softening(precision, dims):
    """eps = 0, the guard form: finite, and the pairs with r^2 = 0 (the self pair, the shared position) add 0."""
    bars = (BAR_A, BAR_J) if precision == "fp32" else (BAR_F64, BAR_F64)
    with watched():
        for n in (2, 65, 257, 1000):
            x, v, m = cloud(n, dims)
            with hermite(bodies_of(x, v, m), eps=0.0, precision=precision) as sim:
                got = sim.jerks()
            check_planes(got, want(n, dims, 0.0), *bars, f"{precision} {dims}-D n {n} eps 0")
        x = np.zeros((2, dims), np.float32)
        v = np.arange(2 * dims, dtype=np.float32).reshape(2, dims)
        with hermite(bodies_of(x, v, [1.0, 2.0]), eps=0.0, precision=precision) as sim:
            a, j = sim.jerks()
        assert not a.any() and not j.any()


@pytest.mark.parametrize("precision,dims", [("fp32", 2), ("fp32", 3), ("fp64", 2)])
def test_fast_bodies_next_to_the_tail_padding(precision, dims):
    """|v| = 1e3 on the last bodies of a tile that is otherwise padding: no NaN, no inf, and the model's values."""
    bars = (BAR_A, BAR_J) if precision == "fp32" else (BAR_F64, BAR_F64)
    x, v, m = (q.copy() for q in cloud(257, dims))
    v[255], v[256] = 1e3, -1e3
    with watched():
        with hermite(bodies_of(x, v, m), precision=precision) as sim:
            got = sim.jerks()
    check_planes(got, hm.acc_jerk_f64(x, v, m, EPS, scales=True), *bars, f"{precision} {dims}-D fast tail")


@pytest.mark.parametrize("precision,dims", [("fp32", 2), ("fp32", 3), ("fp64", 2), ("fp64", 3)])
def test_either_plane_alone_and_any_lanes_p_have_the_bits_of_the_joint_call(precision, dims):
    x, v, m = cloud(1000, dims)
    with watched():
        with hermite(bodies_of(x, v, m), precision=precision) as sim:
            a, j = sim.jerks()
            same_bits(sim.jerks(jerk=False), a, "acc alone")
            same_bits(sim.jerks(acc=False), j, "jerk alone")
            with pytest.raises(ValueError):
                sim.jerks(acc=False, jerk=False)
            assert sim._lib.nb_jerks(sim._h, None, None) == L.NB_EINVAL and b"both NULL" in sim._lib.nb_last_error()
        for p in (1, 2, 4):
            with hermite(bodies_of(x, v, m), precision=precision, lanes_p=p) as sim:
                ap, jp = sim.jerks()
            same_bits(ap, a, f"acc with lanes_p {p}")
            same_bits(jp, j, f"jerk with lanes_p {p}")


def test_jerks_is_the_hermite_handles_call():
    x, v, m = cloud(65, 2)
    with watched():
        with nb.Simulation(bodies_of(x, v, m), eps=EPS, integrator="fr4") as sim:
            with pytest.raises(nb.NBodyError) as e:
                sim.jerks()
            assert e.value.code == L.NB_EINVAL and "HERMITE4" in str(e.value) and "integrator is 3" in str(e.value)


# ------------------------------------------------------------------------------------------------------ trajectory ---
@functools.lru_cache(maxsize=None)
def fixture1000():
    flat = np.load(GOLD / "ic_plummer_1024.npy")[:1000]
    return flat[:, 0:2].copy(), flat[:, 2:4].copy(), flat[:, 6].copy()


@functools.lru_cache(maxsize=None)
def model_five_steps():
    """After 5 steps of HF: (x, v, a1, j1) and the predicted state (x_p, v_p) of the fifth step."""
    x, v, m = fixture1000()
    x4, v4, a4, j4 = hm.run(x, v, m, EPS, [np.float32(HF)] * 4)
    return hm.step(x4, v4, a4, j4, m, EPS, np.float32(HF)), hm.predict(x4, v4, a4, j4, np.float32(HF))


@pytest.mark.parametrize("precision,bar", [("fp64", 2e-7), ("fp32", 1e-5)])
def test_five_steps_against_the_fp64_model(precision, bar):
    """Bars of the KDK and DKD tests against the fp64 model: 2e-7 for fp64 handles, 1e-5 for fp32.  The acc of nb_sync is a1, the
    evaluation at the predicted point: the acc plane nb_jerks gives a twin handle uploaded with the model's predicted state.

    A twin is uploaded through float records, so what it evaluates is the predicted state ROUNDED TO FLOAT.  On these bodies that
    rounding alone moves the fp64 model's own acceleration by 4.0e-6 (close pairs at eps = 0.05: measured here as `records`, and on
    the device: the fp64 handle's acc is 4.0e-6 from its twin's and 5.7e-8 from the model's a1).  The comparison is therefore held in
    two legs, each to the bar: nb_sync's acc against the model's a1 at the unrounded predicted state, and the twin's plane against
    the model at the rounded one; the direct difference is held to the bar plus `records`, which is below the fp32 bar anyway."""
    x, v, m = fixture1000()
    (x5, v5, a5, _), (xp, vp) = model_five_steps()
    xr, vr = xp.astype(np.float32), vp.astype(np.float32)
    ar, _ = hm.acc_jerk_f64(xr, vr, m, EPS)
    records = max_rel(ar, a5)
    with watched():
        with hermite(bodies_of(x, v, m), precision=precision) as sim:
            sim.advance(5, np.float32(HF))
            got = sim.sync().copy()
            assert sim.frame == 5
        with hermite(bodies_of(xr, vr, m), precision=precision) as twin:
            a_twin = twin.jerks(jerk=False)
    ep, ev = max_rel(got["pos"], x5), max_rel(got["vel"], v5)
    ea, em, et = max_rel(got["acc"], a_twin), max_rel(got["acc"], a5), max_rel(a_twin, ar)
    print(f"{precision}: pos {ep:.2e}, vel {ev:.2e}, acc against the model {em:.2e}, the twin against the model at its records {et:.2e}, "
          f"acc against the twin {ea:.2e} (bar {bar:g}; the float records alone {records:.2e})")
    assert ep < bar and ev < bar and em < bar and et < bar, (ep, ev, em, et)
    assert ea < bar + records, (ea, records)


@pytest.mark.parametrize("precision,bar", [("fp64", 2e-7), ("fp32", 1e-5)])
def test_changing_dt_between_calls_lands_where_the_model_lands(precision, bar):
    x, v, m = fixture1000()
    hs = [np.float32(HF), np.float32(HF / 2), np.float32(HF / 2)]
    xm, vm, _, _ = hm.run(x, v, m, EPS, hs)
    with watched():
        with hermite(bodies_of(x, v, m), precision=precision) as sim:
            for h in hs:
                sim.advance(1, h)
            got = sim.sync().copy()
    ep, ev = max_rel(got["pos"], xm), max_rel(got["vel"], vm)
    print(f"{precision} h, h/2, h/2: pos {ep:.2e}, vel {ev:.2e} (bar {bar:g})")
    assert ep < bar and ev < bar, (ep, ev)


@functools.lru_cache(maxsize=None)
def model_energy_errors():
    x, v, m = fixture1000()
    e0 = hm.energy(x, v, m, EPS)
    out = {}
    for k in (4, 8, 16):
        xk, vk, _, _ = hm.run(x, v, m, EPS, [np.float32(T / k)] * k)
        out[k] = abs(hm.energy(xk, vk, m, EPS) - e0) / abs(e0)
    return out


def test_order_on_the_device():
    """fp64 handle, T = 2^-4 in 4, 8, 16 steps, energy from nb_energy (fp64 on the device): |dE/E| within 10 % of the model's
    (6.3e-8, 2.8e-9, 1.0e-10) and both ratios above 12 (the model: 22.8 and 26.5; a third-order scheme gives 8)."""
    x, v, m = fixture1000()
    ref = model_energy_errors()
    de = {}
    with watched():
        for k in (4, 8, 16):
            with hermite(bodies_of(x, v, m), precision="fp64") as sim:
                e0 = sum(sim.energy())
                sim.advance(k, np.float32(T / k))
                de[k] = abs(sum(sim.energy()) - e0) / abs(e0)
    for k in (4, 8, 16):
        print(f"k {k}: |dE/E| device {de[k]:.4g}, model {ref[k]:.4g}")
    print(f"ratios {de[4] / de[8]:.3g}, {de[8] / de[16]:.3g}")
    for k in (4, 8, 16):
        assert abs(de[k] - ref[k]) <= 0.1 * ref[k], (k, de[k], ref[k])
    assert de[4] / de[8] > 12 and de[8] / de[16] > 12


# ----------------------------------------------------------------------------------------------------------- state ---
def plummer(n=1000, dims=2):
    return nb.plummer_3d(n, 5).view(nb.BODY3_DTYPE) if dims == 3 else nb.plummer_2d(n, 5)


@pytest.mark.parametrize("precision,dims,n", [("fp32", 2, 1000), ("fp32", 2, 5693), ("fp64", 2, 1000), ("fp32", 3, 1000), ("fp64", 3, 1000)])
def test_steps_carry_their_pair_and_are_counted(precision, dims, n):
    """nb_step(1) + nb_step(3) = nb_step(4) in every bit, and two handles agree; nb_frame grows by 1 a step; 4 steps on a fresh handle
    are 5 profiled force launches and the next 4 are 4; nb_step_begin is refused; nb_describe names the integrator."""
    ic = plummer(n, dims)
    out = []
    with watched():
        for calls in ((1, 3), (4,), (4,)):
            with hermite(ic, precision=precision) as sim:
                d = sim.describe()
                assert d.endswith(" integrator=hermite4") and "symmetric=0" in d, d
                sim.profile(True)
                for k in calls:
                    before = sim.frame
                    sim.advance(k, HF)
                    assert sim.frame == before + k
                out.append(sim.sync().copy())
                assert sim.profile_read()[1] == 5
                sim.advance(4, HF)
                sim.wait()
                assert sim.profile_read()[1] == 4
                with pytest.raises(nb.NBodyError) as e:
                    sim.step_begin(HF)
                assert e.value.code == L.NB_EINVAL and "HERMITE4" in str(e.value)
    for f in ("pos", "vel", "acc"):
        same_bits(out[0][f], out[1][f], f"{precision} {dims}-D: {f} of 1 + 3 steps against 4")
        same_bits(out[1][f], out[2][f], f"{precision} {dims}-D: {f} of two handles")
    assert np.isfinite(out[0]["pos"]).all() and np.abs(out[0]["acc"]).max() > 0


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_an_upload_of_its_own_records_is_a_fresh_handle(precision):
    """A run interrupted by nb_upload of its own nb_sync records continues as a fresh handle created from those records, bit for bit:
    the upload invalidates the carried pair."""
    ic = plummer()
    with watched():
        with hermite(ic, precision=precision) as sim:
            sim.advance(2, HF)
            rec = sim.sync().copy()
            sim.upload(rec)
            sim.advance(2, HF)
            a = sim.sync().copy()
        with hermite(rec, precision=precision) as fresh:
            fresh.advance(2, HF)
            b = fresh.sync().copy()
    for f in ("pos", "vel", "acc"):
        same_bits(a[f], b[f], f"{precision}: {f} after the upload")


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_jerks_between_two_steps_changes_no_bit_of_the_run(precision):
    ic = plummer()
    with watched():
        with hermite(ic, precision=precision) as sim:
            sim.advance(2, HF)
            frame = sim.frame
            mid = sim.sync().copy()
            a, j = sim.jerks()
            assert sim.frame == frame and np.abs(j).max() > 0
            for f in ("pos", "vel", "acc"):
                same_bits(sim.sync()[f], mid[f], f"{precision}: {f} across nb_jerks")
            sim.advance(2, HF)
            with_call = sim.sync().copy()
        with hermite(ic, precision=precision) as sim:
            sim.advance(4, HF)
            without = sim.sync().copy()
    for f in ("pos", "vel", "acc"):
        same_bits(with_call[f], without[f], f"{precision}: {f} with nb_jerks between the steps")


def test_a_restart_from_a_dump_follows_the_run(tmp_path):
    """The dump's header carries the integrator; the restarted handle re-evaluates at the corrected state, so it follows the model
    inside the trajectory bar and is not required to match the original run's bits."""
    x, v, m = fixture1000()
    (x5, v5, _, _), _ = model_five_steps()
    with watched():
        with hermite(bodies_of(x, v, m)) as sim:
            sim.advance(2, np.float32(HF))
            sim.dump(tmp_path / "mid.nbd")
        back, frame, p = nb.read_bodies(tmp_path / "mid.nbd")
        assert frame == 2 and p.integrator == L.NB_INTEGRATOR_HERMITE4
        with nb.Simulation(back, eps=p.eps, integrator="hermite4", first_frame=frame) as again:
            again.advance(3, np.float32(HF))
            got = again.sync().copy()
            assert again.frame == 5
    ep, ev = max_rel(got["pos"], x5), max_rel(got["vel"], v5)
    print(f"restart after 2 of 5 steps: pos {ep:.2e}, vel {ev:.2e} (bar 1e-5)")
    assert ep < 1e-5 and ev < 1e-5, (ep, ev)
