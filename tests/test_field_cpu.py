"""CPU: nb_field — the fp32 form of the sweep (tests/field_model.py) against the float64 sum, the model's conventions, the argument
check that needs no device, and the binding."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

import field_model as fm
import potential_model as pm

# phi is nb_potentials' arithmetic word for word: its bar, derived in tests/test_potential_cpu.py.
BAR_F32 = 4e-6
# acc, per component, against S = sum_j |term_j| of that component (the quantity the arithmetic bounds: a rounding error of a term is
# relative to the term, one of a partial sum is at most relative to the sum of the magnitudes).  Counted as BAR_F32 is counted in
# tests/test_potential_cpu.py, in units of 2^-24, not tuned: about 6.5 per term (what reaches 1/r there, the displacement and the two
# fused multiply-adds halved by the square root and the 1-ulp reciprocal square root, 2.5, enters cubed here but is dominated by the
# reciprocal square root's 1 x 3; with the displacement d_c, the three products inv inv, inv2 inv, m_j s) = 3.9e-7, plus the 63 roundings
# of a float32 run of 64 terms = 3.8e-6; the float64 sums across the runs add nothing visible.  4.14e-6 in all.  The restatement
# below stays under 8e-7 on every case, the reciprocal square root perturbed by +-1 ulp.
BAR_ACC = (6.5 + 63) * 2.0 ** -24
CASES = [("ic_plummer_1024", 0.05), ("ic_plummer_1024", 1e-3), ("ic_plummer_4096", 0.05), ("ic_plummer_4096", 1e-3),
         ("ic_random_333", 0.05), ("default_ics_first4096", 1.0)]


def points_for(pos, seed=11):
    """257 points: 200 uniform in the bounding box of the bodies, 57 at a body + 1e-3 (close to a body, on none)."""
    rng = np.random.default_rng(seed)
    lo, hi = pos.min(0), pos.max(0)
    box = rng.uniform(lo, hi, (200, pos.shape[1])).astype(np.float32)
    near = (pos[rng.choice(pos.shape[0], 57, replace=False)] + np.float32(1e-3)).astype(np.float32)
    pts = np.concatenate([box, near])
    assert not (pts[:, None, :] == pos[None, :, :]).all(2).any()
    return pts


@pytest.mark.parametrize("name,eps", CASES)
def test_fp32_form_is_within_its_bars_of_the_fp64_sum(gold, name, eps):
    """Both with the correctly rounded reciprocal square root and with one perturbed by up to 1 ulp either way (v_rsq_f32)."""
    flat = gold[name].astype(np.float32)
    pos, m = flat[:, 0:2], flat[:, 6]
    pts = points_for(pos)
    phi, acc, scale = fm.field_f64(pts, pos, m, eps)
    assert np.isfinite(phi).all() and (phi < 0).all() and np.isfinite(acc).all() and (scale > 0).all()
    for ulp in (0, 1):
        got_phi, got_acc = fm.field_f32(pts, pos, m, eps, ulp, np.random.default_rng(5))
        ephi, eacc = pm.rel_err(got_phi, phi), fm.acc_err(got_acc, acc, scale)
        mag = np.abs(got_acc - acc).max(1) / np.linalg.norm(acc, axis=1)
        print(f"{name} eps {eps:g} rsq +-{ulp} ulp: phi max {ephi.max():.3g} (bar {BAR_F32:g}); acc / S max {eacc.max():.3g} median "
              f"{np.median(eacc):.3g} (bar {BAR_ACC:.3g}); acc / |a| max {mag.max():.3g} (no bar)")
        assert ephi.max() <= BAR_F32
        assert eacc.max() <= BAR_ACC


def test_phi_of_the_model_is_the_potential_models_phi_at_a_massless_body():
    """The phi path is potential_tiled_f32's body: at the position of a massless body, with eps > 0, the same bits."""
    rng = np.random.default_rng(2)
    pos = rng.normal(0, 1, (300, 2)).astype(np.float32)
    m = rng.uniform(0.5, 2.0, 300).astype(np.float32)
    tracers = [0, 63, 64, 255, 256, 299]
    m[tracers] = 0
    want = pm.phi_f32(pos, m, 0.05)[tracers]
    got, _ = fm.field_f32(pos[tracers], pos, m, 0.05)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_model_conventions_for_a_point_on_a_body():
    """A point on a body adds -m / eps and zero acc; eps = 0 there is finite and equals the sum without that body."""
    pos = np.array([[1.0, 2.0], [4.0, 6.0], [-2.0, 6.0]], np.float32)
    m = np.array([3.0, 7.0, 5.0], np.float32)
    pts = pos[:1].copy()
    e = pm.eps_of(0.05)
    r1, r2 = np.sqrt(25 + e * e), np.sqrt(25 + e * e)
    want_phi = -3.0 / e - 7.0 / r1 - 5.0 / r2
    want_acc = np.array([7.0 * 3 / r1 ** 3 + 5.0 * -3 / r2 ** 3, 7.0 * 4 / r1 ** 3 + 5.0 * 4 / r2 ** 3])
    phi, acc, scale = fm.field_f64(pts, pos, m, 0.05)
    assert abs(phi[0] - want_phi) <= 1e-15 * abs(want_phi) and np.abs(acc[0] - want_acc).max() <= 1e-15 * scale.max()
    phi32, acc32 = fm.field_f32(pts, pos, m, 0.05)
    assert pm.rel_err(phi32, phi).max() <= BAR_F32 and fm.acc_err(acc32, acc, scale).max() <= BAR_ACC
    assert phi32[0] < -3.0 / e                                   # the -m / eps term is there
    for model in (lambda *a: fm.field_f64(*a)[:2], fm.field_f32):
        on, on_acc = model(pts, pos, m, 0.0)
        off, off_acc = model(pts, pos[1:], m[1:], 0.0)
        assert np.isfinite(on).all() and np.isfinite(on_acc).all()
        assert np.array_equal(on, off) and np.array_equal(on_acc, off_acc)
        assert abs(on[0] + 12.0 / 5.0) < 1e-5


def test_a_null_handle_is_refused_first_without_a_device():
    lib = nb.load()
    pts = np.zeros((4, 2), np.float32)
    phi, acc = np.full(4, -7.0), np.full((4, 2), -7.0)
    assert lib.nb_field(None, pts.ctypes.data, 4, phi.ctypes.data, acc.ctypes.data) == L.NB_EINVAL
    assert b"nb_field: NULL handle" in lib.nb_last_error() and lib.nb_last_error_code() == L.NB_EINVAL
    assert lib.nb_field(None, None, 0, None, None) == L.NB_EINVAL and b"nb_field: NULL handle" in lib.nb_last_error()
    assert (phi == -7.0).all() and (acc == -7.0).all()


def test_prototype_header_and_front_end():
    header = (ROOT / "include" / "nbody.h").read_text()
    assert re.search(r"^int nb_field\(nb_sim \*s, const float \*points, size_t npoints, double \*phi, double \*acc\);$", header, re.M)
    assert re.search(r"^#define NB_FIELD_POINTS_MAX 4194304$", header, re.M) and L.NB_FIELD_POINTS_MAX == 4194304
    want = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    restype, argtypes = L.PROTOTYPES["nb_field"]
    assert restype is C.c_int and argtypes == want
    fn = nb.load().nb_field
    assert fn.restype is C.c_int and list(fn.argtypes) == want
    assert callable(nb.Simulation.field)
    # no new flag, extras bit or ABI number came with it
    assert "nb_debug_" not in header and L.NB_ABI_VERSION == 8 == nb.load().nb_abi_version()
    assert re.search(r"^#define NB_ABI_VERSION 8$", header, re.M)
