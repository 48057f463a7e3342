"""CPU: nb_raster — the interface (header, ctypes struct against the C sizeof, the exported symbol, the argument checks that need no
device) and the properties of the numpy statement of its contract (tests/raster_model.py) on a committed fixture."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import raster_model as rm  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"


def test_header_declares_the_struct_and_the_entry_point():
    header = (ROOT / "include" / "nbody.h").read_text()
    assert "typedef struct nb_view {" in header and "} nb_view;" in header
    assert "int nb_raster(nb_sim *s, const nb_view *view, uint32_t *count, float *mass);" in header
    assert "#define NB_ABI_VERSION 8" in header


def test_ctypes_struct_has_the_size_and_offsets_of_the_c_struct(tmp_path):
    src = tmp_path / "view_size.c"
    src.write_text('#include <stdio.h>\n#include "nbody.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(nb_view), offsetof(nb_view, width), offsetof(nb_view, center_x), '
                   'offsetof(nb_view, mass_quantum), offsetof(nb_view, _reserved0)); return 0; }\n')
    exe = tmp_path / "view_size"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    V = L.nb_view
    assert got == [C.sizeof(V), V.width.offset, V.center_x.offset, V.mass_quantum.offset, V._reserved0.offset] == [32, 4, 12, 24, 28]
    assert [name for name, _ in V._fields_] == ["struct_size", "width", "height", "center_x", "center_y", "scale", "mass_quantum", "_reserved0"]


def test_library_exports_the_symbol_and_refuses_a_null_handle_first():
    lib = nb.load()
    assert lib.nb_abi_version() == 8
    assert hasattr(lib, "nb_raster") and "nb_raster" in L.PROTOTYPES and hasattr(nb.Simulation, "raster")
    syms = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T nb_raster\n" in syms
    v = L.nb_view()
    v.struct_size, v.width, v.height, v.scale = C.sizeof(L.nb_view), 4, 4, 1.0
    plane = np.full(16, 0xDEADBEEF, np.uint32)
    assert lib.nb_raster(None, C.byref(v), plane.ctypes.data, None) == L.NB_EINVAL
    assert b"nb_raster: NULL handle" in lib.nb_last_error() and lib.nb_last_error_code() == L.NB_EINVAL
    assert lib.nb_raster(None, None, None, None) == L.NB_EINVAL and b"NULL handle" in lib.nb_last_error()
    assert (plane == 0xDEADBEEF).all()


# ---------------------------------------------------------------------------------------------------------------------
# the model's own properties
# ---------------------------------------------------------------------------------------------------------------------
def fixture():
    flat = np.load(GOLD / "ic_random_333.npy").astype(np.float32)
    return flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()


def cutting_view(x, y):
    """A 17 x 13 view about the median that leaves bodies out on all four sides."""
    cx, cy = float(np.median(x)), float(np.median(y))
    scale = 1.6 * min(17 / float(np.ptp(x)), 13 / float(np.ptp(y)))
    return dict(width=17, height=13, center=(cx, cy), scale=scale)


def test_model_counts_the_bodies_inside():
    x, y, m = fixture()
    v = cutting_view(x, y)
    inside, px = rm.pixels(x, y, **v)
    sx = (x - np.float32(v["center"][0])) * np.float32(v["scale"]) + np.float32(8.5)
    sy = (y - np.float32(v["center"][1])) * np.float32(v["scale"]) + np.float32(6.5)
    assert (sx[~inside] < 0).any() and (sx[~inside] >= 17).any() and (sy[~inside] < 0).any() and (sy[~inside] >= 13).any()
    count, mass = rm.raster(x, y, m, quantum=2.0 ** -10, **v)
    assert count.shape == (13, 17) and count.dtype == np.uint32 and mass.shape == (13, 17) and mass.dtype == np.float32
    assert int(count.sum()) == int(inside.sum()) and 0 < int(inside.sum()) < x.size
    assert px[inside].min() >= 0 and px[inside].max() < 17 * 13
    # the unit sums are those of the bodies inside, and the mass plane is their exact product with the quantum
    U = rm.unit_sums(x, y, m, quantum=2.0 ** -10, **v)
    assert int(U.sum()) == int(rm.units(m[inside], 2.0 ** -10).sum())
    assert np.array_equal(mass, (U.astype(np.float64) * 2.0 ** -10).astype(np.float32))
    # whole view: everything inside
    full = dict(width=17, height=13, center=v["center"], scale=v["scale"] / 4)
    assert int(rm.raster(x, y, m, **full)[0].sum()) == x.size


def test_model_does_not_depend_on_the_order_of_the_bodies():
    x, y, m = fixture()
    v = cutting_view(x, y)
    c0, m0 = rm.raster(x, y, m, quantum=1e-3, **v)
    perm = np.random.default_rng(5).permutation(x.size)
    c1, m1 = rm.raster(x[perm], y[perm], m[perm], quantum=1e-3, **v)
    assert np.array_equal(c0, c1) and np.array_equal(m0.view(np.uint32), m1.view(np.uint32)) and m0.max() > 0


def test_model_edges_lower_inclusive_upper_exclusive():
    # scale 1, centre (4, 3) on an 8 x 6 view: sx = x, sy = y exactly
    v = dict(width=8, height=6, center=(4.0, 3.0), scale=1.0)
    x = np.array([0.0, 7.5, 8.0, -0.5, 3.0, 3.0, 3.0, np.nan, np.inf, 2.0, -0.0], np.float32)
    y = np.array([0.0, 5.5, 2.0, 2.0, 6.0, -0.5, 5.0, 1.0, 1.0, -np.inf, 0.0], np.float32)
    inside, px = rm.pixels(x, y, **v)
    assert inside.tolist() == [True, True, False, False, False, False, True, False, False, False, True]
    assert px[inside].tolist() == [0, 5 * 8 + 7, 5 * 8 + 3, 0]
    count, _ = rm.raster(x, y, np.ones_like(x), **v)
    assert count[0, 0] == 2 and count[5, 7] == 1 and count[5, 3] == 1 and int(count.sum()) == 4


def test_model_units_round_to_even_and_saturate():
    q = np.float32(0.25)
    m = np.array([0.125, 0.375, 0.625, 0.0, -1.0, np.nan, np.inf, 0.25 * 2.0 ** 32, 0.25 * (2.0 ** 32 - 256), 1e-9], np.float32)
    assert rm.units(m, q).tolist() == [0, 2, 2, 0, 0, 0, 4294967295, 4294967295, 4294967040, 0]
