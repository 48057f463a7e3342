"""CPU: nb_group_binding — the interface (header, record layout, exported symbol, binding), the numpy statement of its contract
(tests/group_binding_model.py) against closed forms, and the condition that keeps the windows of the GPU tests from hiding a failure:
for every fixed input of tests/test_group_binding_gpu.py the model alone gives a window of at most max(1, members / 1000)."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import group_binding_model as bm  # noqa: E402
import test_group_binding_gpu as tg  # noqa: E402  (its fixed inputs only; none of its tests is imported by name)

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "nbody.h").read_text()


def bodies(x, y, mass, vx=None, vy=None):
    b = nb.bodies_array(len(x))
    b["pos"][:, 0], b["pos"][:, 1], b["mass"] = x, y, mass
    if vx is not None:
        b["vel"][:, 0], b["vel"][:, 1] = vx, vy
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_keeps_the_abi_number():
    decl = ("int nb_group_binding(nb_sim *s, float radius, uint32_t min_members, double *phi, double *e,\n"
            "                     nb_group_energy *out, size_t capacity, size_t *count);")
    assert decl in HEADER and "#define NB_ABI_VERSION 8" in HEADER


def test_dtype_is_32_bytes_and_matches_the_headers_static_asserts():
    d = L.GROUP_ENERGY_DTYPE
    assert d.itemsize == 32 and nb.GROUP_ENERGY_DTYPE is d
    assert d.names == ("label", "members", "bound", "most_bound", "e_min", "potential")
    assert [d.fields[f][1] for f in d.names] == [0, 4, 8, 12, 16, 24]
    assert "static_assert(sizeof(nb_group_energy) == 32" in HEADER and "_Static_assert(sizeof(nb_group_energy) == 32" in HEADER
    asserted = dict(re.findall(r"offsetof\(nb_group_energy, (\w+)\) == (\d+)", HEADER))
    assert set(asserted) == {"members", "bound", "most_bound", "e_min", "potential"}
    for name, off in asserted.items():
        assert d.fields[name][1] == int(off), name
    assert bm.DTYPE.itemsize == 32 and bm.DTYPE.names == d.names
    src = '#include "nbody.h"\nint main(void) { return sizeof(nb_group_energy) == 32 ? 0 : 1; }\n'
    for cc, std in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        r = subprocess.run([cc, std, "-x", "c" if cc == "gcc" else "c++", "-fsyntax-only", f"-I{ROOT / 'include'}", "-"], input=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_library_exports_the_symbol_and_the_bindings_exist():
    lib = nb.load()
    assert lib.nb_abi_version() == 8
    assert hasattr(lib, "nb_group_binding") and "nb_group_binding" in L.PROTOTYPES
    assert callable(getattr(nb.Simulation, "group_binding", None))
    syms = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T nb_group_binding\n" in syms
    assert "group_binding(float radius, uint32_t min_members, double *phi, double *e, nb_group_energy *out, size_t capacity)" in \
        (ROOT / "nbodysim_amd" / "host" / "Simulation.hpp").read_text()


def test_null_handle_and_null_count_are_refused_without_a_device():
    import ctypes as C
    lib = nb.load()
    count = C.c_size_t(77)
    assert lib.nb_group_binding(None, 1.0, 2, None, None, None, 0, C.byref(count)) == L.NB_EINVAL
    assert lib.nb_last_error().decode() == "nb_group_binding: NULL handle" and count.value == 77


# ---------------------------------------------------------------------------------------------------------------------
# the model against closed forms
# ---------------------------------------------------------------------------------------------------------------------
def test_two_bodies():
    b = bodies([0.0, 0.5], [0.0, 0.0], [2.0, 3.0], [1.0, -1.0], [0.0, 0.0])
    m = bm.binding(b, 1.0, 2, 0.25)
    r = 1.0 / np.sqrt(0.25 + 0.0625)
    assert np.allclose(m.phi, [-3.0 * r, -2.0 * r], rtol=1e-15)
    # vel = (2 - 3) / 5 = -0.2: v - vel = 1.2 and -0.8
    assert np.allclose(m.e, [0.72 - 3.0 * r, 0.32 - 2.0 * r], rtol=1e-14)
    rec = m.rec[0]
    assert (rec["label"], rec["members"], rec["bound"], rec["most_bound"]) == (0, 2, 2, 0) and rec["e_min"] == m.e[0]
    assert np.isclose(rec["potential"], -6.0 * r, rtol=1e-15)                    # U = -m0 m1 / r: every pair once
    assert bm.binding(b, 1.0, 3, 0.25).rec.shape == (0,) and np.isnan(bm.binding(b, 1.0, 3, 0.25).phi).all()


def test_equilateral_triangle():
    s = 0.5
    b = bodies([0.0, s, s / 2], [0.0, 0.0, s * np.sqrt(3) / 2], [1.0, 1.0, 1.0])
    m = bm.binding(b, 1.0, 2, 0.0)
    assert np.allclose(m.phi, -2.0 / s, rtol=1e-6) and np.allclose(m.e, m.phi)   # (float32 positions: the sides agree to 1e-7)
    assert np.isclose(m.rec["potential"][0], -3.0 / s, rtol=1e-6) and m.rec["bound"][0] == 3


def test_coincident_bodies_and_a_massless_member():
    k, mass, eps = 6, 1.5, 0.25
    b = bodies(np.full(k, 3.0), np.full(k, -2.0), np.full(k, mass))
    m = bm.binding(b, 1.0, 2, eps)
    assert np.allclose(m.phi, -(k - 1) * mass / eps, rtol=1e-15)                 # the self term is left out by index, not by distance
    assert m.rec["most_bound"][0] == 0                                          # a tie goes to the smallest index
    b["mass"][2] = 0.0                                                           # a massless member feels the others and adds nothing
    m = bm.binding(b, 1.0, 2, eps)
    assert np.isclose(m.phi[2], -(k - 1) * mass / eps) and np.allclose(np.delete(m.phi, 2), -(k - 2) * mass / eps)
    assert np.isclose(m.rec["potential"][0], -0.5 * (k - 1) * (k - 2) * mass * mass / eps, rtol=1e-15)
    with np.errstate(all="ignore"):
        m0 = bm.binding(b, 1.0, 2, 0.0)
    assert not np.isfinite(m0.phi).any()
    alone = bm.binding(bodies([0.0], [0.0], [1.0]), 1.0, 1, 0.5)
    assert alone.phi[0] == 0 and alone.e[0] == 0 and not np.signbit(alone.phi[0]) and alone.rec["most_bound"][0] == 0
    assert alone.rec["bound"][0] == 0 and alone.rec["potential"][0] == 0


def test_mismatches_sees_what_it_should():
    b, radius, wl = tg.tails_input(257)
    m = bm.binding(b, radius, 2, 0.5, label=wl)
    assert not bm.mismatches(m, m.phi.copy(), m.e.copy(), m.rec.copy())
    i = int(np.flatnonzero(m.kept)[0])
    phi = m.phi.copy()
    phi[i] *= 1 + 1e-5
    assert any(t.startswith("phi:") for t in bm.mismatches(m, phi))
    e = m.e.copy()
    e[int(np.flatnonzero(~m.kept)[0])] = 0.0
    assert any("NaN" in t for t in bm.mismatches(m, e=e))
    rec = m.rec.copy()
    rec["bound"][0] += 1
    rec["most_bound"][1] = m.idx[1][np.argmax(m.e[m.idx[1]])]
    bad = bm.mismatches(m, e=m.e, rec=rec)
    assert any("bound" in t and "row 0" in t for t in bad) and any("most_bound" in t and "row 1" in t for t in bad)


# ---------------------------------------------------------------------------------------------------------------------
# the window condition, for every fixed input of the GPU file
# ---------------------------------------------------------------------------------------------------------------------
def assert_tight(m, what):
    width, allowed = bm.window_widths(m)
    assert (width <= allowed).all(), f"{what}: window widths {width[width > allowed].tolist()}"


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_windows_of_the_tails_inputs(n):
    b, radius, wl = tg.tails_input(n)
    for mm in (1, 2, 5):
        assert_tight(bm.binding(b, radius, mm, 0.5, label=wl), f"tails n {n} min_members {mm}")
    if n == 1000:
        assert_tight(bm.binding(b, radius, 2, 0.5, label=wl, fp64=True), "fp64")
        light = b.copy()
        light["mass"] *= np.float32(1.0 / 1000)
        assert_tight(bm.binding(light, radius, 2, 0.5, label=wl), "tree and sharded handles")


@pytest.mark.parametrize("T", [64, 128, 256, 512, 1024])
def test_windows_of_the_boundary_inputs(T):
    for prefix in (1, 63, T - 1):
        for size in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
            b, label = tg.boundary_input(prefix, size)
            assert_tight(bm.binding(b, 1.0, 2, 0.5, label=label), f"T {T} prefix {prefix} size {size}")


def test_windows_of_the_other_inputs():
    b, label = tg.two_adjacent_groups()
    assert_tight(bm.binding(b, 1.0, 1, 0.5, label=label), "two adjacent groups")
    assert_tight(bm.binding(tg.chain_input(), 1.0, 2, 0.5, label=np.zeros(3000, np.int64)), "chain")
    assert_tight(bm.binding(tg.coincident_input(), 1.0, 1, 1.0), "coincident")
    b3 = nb.plummer_3d(1000, 7).view(L.BODY3_DTYPE)
    assert_tight(bm.binding(b3, 0.06, 1, 0.05, dims=3), "dims = 3")


def test_lattice_giant_has_both_signs_a_window_of_zero_and_a_clear_minimum():
    b, label, m = tg.lattice_giant()
    width, _ = bm.window_widths(m)
    assert m.rec["members"][0] == 8192 and 0 < m.rec["bound"][0] < 8192 and width[0] == 0
    e = np.sort(m.e[m.kept])
    assert e[1] - e[0] > 10 * m.bar_e_min[0]                                     # the runner-up is far outside 2 bars: most_bound is decided
