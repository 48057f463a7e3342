"""CPU: nb_potentials — the fp32 form of the sweep (tests/potential_model.py) against the float64 sum, the argument checks that need
no device, and the binding."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

import potential_model as pm

# 4e-6 relative per body is the worst case of the arithmetic, not a tuned number: about 3.5 ulp per term (the displacement, two
# fused multiply-adds, a 1-ulp reciprocal square root, the product) = 2.1e-7, plus the 63 roundings of a float32 run of 64
# same-signed terms = 3.8e-6; the float64 sums across the runs add nothing visible.
BAR_F32 = 4e-6
CASES = [("ic_plummer_1024", 0.05), ("ic_plummer_1024", 1e-3), ("ic_plummer_4096", 0.05), ("ic_plummer_4096", 1e-3),
         ("ic_random_333", 0.05), ("default_ics_first4096", 1.0)]


@pytest.mark.parametrize("name,eps", CASES)
def test_fp32_form_is_within_its_bar_of_the_fp64_sum(gold, name, eps):
    """Both with the correctly rounded reciprocal square root and with one perturbed by up to 1 ulp either way (v_rsq_f32)."""
    flat = gold[name].astype(np.float32)
    pos, m = flat[:, 0:2], flat[:, 6]
    want = pm.phi_f64(pos, m, eps)
    assert np.isfinite(want).all() and (want < 0).all()
    for ulp in (0, 1):
        got = pm.phi_f32(pos, m, eps, ulp, np.random.default_rng(5))
        err = pm.rel_err(got, want)
        print(f"{name} eps {eps:g} rsq +-{ulp} ulp: max {err.max():.3g} median {np.median(err):.3g} (bar {BAR_F32:g})")
        assert err.max() <= BAR_F32


def test_model_leaves_the_self_term_out_by_index():
    """Two bodies on one position see each other (-m / eps); a body alone has phi = 0; eps = 0 is finite without a shared position."""
    pos = np.array([[1.0, 2.0], [1.0, 2.0], [4.0, 6.0]], np.float32)
    m = np.array([3.0, 5.0, 7.0], np.float32)
    e = pm.eps_of(0.05)
    want = np.array([-5.0 / e - 7.0 / np.sqrt(25 + e * e), -3.0 / e - 7.0 / np.sqrt(25 + e * e), -8.0 / np.sqrt(25 + e * e)])
    assert pm.rel_err(pm.phi_f64(pos, m, 0.05), want).max() < 1e-15
    assert pm.rel_err(pm.phi_f32(pos, m, 0.05), want).max() < BAR_F32
    assert pm.phi_f64(pos[:1], m[:1], 0.0)[0] == 0.0 and pm.phi_f32(pos[:1], m[:1], 0.0)[0] == 0.0
    free = pm.phi_f32(pos[1:], m[1:], 0.0)
    assert np.isfinite(free).all() and pm.rel_err(free, [-7.0 / 5.0, -5.0 / 5.0]).max() < BAR_F32
    assert not np.isfinite(pm.phi_f32(pos, m, 0.0)[:2]).any() and np.isfinite(pm.phi_f32(pos, m, 0.0)[2])


def test_null_arguments_are_refused_without_a_device():
    lib = nb.load()
    phi = np.full(4, -7.0)
    assert lib.nb_potentials(None, phi.ctypes.data) == L.NB_EINVAL and b"nb_potentials: NULL handle" in lib.nb_last_error()
    assert lib.nb_last_error_code() == L.NB_EINVAL
    assert lib.nb_potentials(None, None) == L.NB_EINVAL
    assert (phi == -7.0).all()


def test_prototype_header_and_front_end():
    header = (ROOT / "include" / "nbody.h").read_text()
    assert re.search(r"^int nb_potentials\(nb_sim \*s, double \*phi\);$", header, re.M)
    restype, argtypes = L.PROTOTYPES["nb_potentials"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p]
    fn = nb.load().nb_potentials
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    assert callable(nb.Simulation.potentials)
    # no new flag, extras bit or ABI number came with it
    assert "nb_debug_" not in header and L.NB_ABI_VERSION == nb.load().nb_abi_version()
