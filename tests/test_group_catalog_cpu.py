"""CPU: nb_group_catalog — the interface (header, record layout, exported symbol, binding, the argument checks that need no device)
and the numpy statement of its contract (tests/group_catalog_model.py) against a brute-force loop."""
import ctypes as C
import re
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import group_catalog_model as cm  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "nbody.h").read_text()


def test_header_declares_the_entry_point_and_keeps_the_abi_number():
    assert "int nb_group_catalog(nb_sim *s, float radius, uint32_t min_members, nb_group *out, size_t capacity, size_t *count);" in HEADER
    assert "#define NB_ABI_VERSION 8" in HEADER
    script = (ROOT / "nbodysim_amd" / "csrc" / "nbody.map").read_text()
    assert re.search(r"global:\s*nb_\*;", script)                  # the version script exports the nb_ prefix: the new symbol with it


def test_dtype_is_80_bytes_and_matches_the_headers_static_asserts():
    assert L.GROUP_DTYPE.itemsize == 80 and nb.GROUP_DTYPE is L.GROUP_DTYPE
    assert L.GROUP_DTYPE.names == ("label", "members", "mass", "pos", "vel", "sigma2", "r_max")
    assert "static_assert(sizeof(nb_group) == 80" in HEADER and "_Static_assert(sizeof(nb_group) == 80" in HEADER
    asserted = dict(re.findall(r"offsetof\(nb_group, (\w+)\) == (\d+)", HEADER))
    assert set(asserted) == {"members", "mass", "pos", "vel", "sigma2", "r_max"}
    for name, off in asserted.items():
        assert L.GROUP_DTYPE.fields[name][1] == int(off), name
    assert L.GROUP_DTYPE.fields["label"][1] == 0
    assert L.GROUP_DTYPE.fields["pos"][0].shape == (3,) and L.GROUP_DTYPE.fields["vel"][0].shape == (3,)
    # and the compiler agrees with the header
    src = '#include "nbody.h"\nint main(void) { return sizeof(nb_group) == 80 ? 0 : 1; }\n'
    for cc, std in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        r = subprocess.run([cc, std, "-x", "c" if cc == "gcc" else "c++", "-fsyntax-only", f"-I{ROOT / 'include'}", "-"], input=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_library_exports_the_symbol_and_the_bindings_exist():
    lib = nb.load()
    assert lib.nb_abi_version() == 8
    assert hasattr(lib, "nb_group_catalog") and "nb_group_catalog" in L.PROTOTYPES
    assert callable(getattr(nb.Simulation, "group_catalog", None))
    syms = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T nb_group_catalog\n" in syms


def test_arguments_are_refused_without_a_device():
    lib = nb.load()
    out = np.full(4, 0xAB, np.uint8).repeat(80).view(L.GROUP_DTYPE)
    before = out.tobytes()
    count = C.c_size_t(77)
    assert lib.nb_group_catalog(None, 1.0, 2, out.ctypes.data, 4, C.byref(count)) == L.NB_EINVAL
    assert b"nb_group_catalog: NULL handle" in lib.nb_last_error() and lib.nb_last_error_code() == L.NB_EINVAL
    # the arguments are looked at before anything of the handle is: a block of zero bytes stands in for one here
    dummy = (C.c_uint8 * 65536)()
    assert lib.nb_group_catalog(C.addressof(dummy), 1.0, 2, out.ctypes.data, 4, None) == L.NB_EINVAL
    assert b"nb_group_catalog: NULL count" in lib.nb_last_error()
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.nb_group_catalog(C.addressof(dummy), radius, 2, out.ctypes.data, 4, C.byref(count)) == L.NB_EINVAL
        assert lib.nb_last_error().decode().startswith("nb_group_catalog: radius must be finite and > 0"), radius
    for radius in (1e-30, 1e30):
        assert lib.nb_group_catalog(C.addressof(dummy), radius, 2, out.ctypes.data, 4, C.byref(count)) == L.NB_EINVAL
        assert lib.nb_last_error().decode().startswith("nb_group_catalog: radius * radius must be finite and > 0 in float"), radius
    assert lib.nb_group_catalog(C.addressof(dummy), 1.0, 0, out.ctypes.data, 4, C.byref(count)) == L.NB_EINVAL
    assert b"min_members" in lib.nb_last_error()
    assert out.tobytes() == before and count.value == 77


# ---------------------------------------------------------------------------------------------------------------------
# the model against a loop that shares nothing with it but the definitions
# ---------------------------------------------------------------------------------------------------------------------
def brute_force(b, radius, min_members):
    """Groups by flood fill over the float32 predicate, values in exact rational arithmetic."""
    n = b.shape[0]
    x, y = b["pos"][:, 0], b["pos"][:, 1]
    r2 = np.float32(radius) * np.float32(radius)
    seen, rows = np.zeros(n, bool), []
    for start in range(n):
        if seen[start]:
            continue
        seen[start] = True
        todo, members = [start], []
        while todo:
            i = todo.pop()
            members.append(i)
            for j in range(n):
                if not seen[j]:
                    dx, dy = x[j] - x[i], y[j] - y[i]
                    if dx * dx + dy * dy < r2:
                        seen[j] = True
                        todo.append(j)
        if len(members) < min_members:
            continue
        members.sort()
        m = [Fraction(float(b["mass"][i])) if b["mass"][i] > 0 else Fraction(0) for i in members]
        mass = sum(m)
        w = m if mass > 0 else [Fraction(1)] * len(members)
        W = mass if mass > 0 else Fraction(len(members))
        pos = [sum(wi * Fraction(float(b["pos"][i, d])) for wi, i in zip(w, members)) / W for d in range(2)]
        vel = [sum(wi * Fraction(float(b["vel"][i, d])) for wi, i in zip(w, members)) / W for d in range(2)]
        s2 = sum(wi * sum((Fraction(float(b["vel"][i, d])) - vel[d]) ** 2 for d in range(2)) for wi, i in zip(w, members)) / W
        r2max = max(sum((Fraction(float(b["pos"][i, d])) - pos[d]) ** 2 for d in range(2)) for i in members)
        rows.append((members[0], len(members), float(mass), [float(p) for p in pos], [float(u) for u in vel], float(s2), float(r2max) ** 0.5))
    return rows                                                    # start runs upwards: ascending label


def test_model_against_a_brute_force_loop_on_200_bodies():
    rng = np.random.default_rng(23)
    b = nb.bodies_array(200)
    b["pos"] = rng.uniform(-6, 6, (200, 2)).astype(np.float32)
    b["vel"] = rng.normal(0, 1, (200, 2)).astype(np.float32)
    b["mass"] = rng.uniform(0.5, 2.0, 200).astype(np.float32)
    b["mass"][[3, 50, 51]] = [0.0, -1.0, 0.0]
    b["pos"][120:124] = [50.0, 50.0]                               # coincident bodies, away from the rest
    b["mass"][120:124] = 0.0                                       # ... without mass: the unweighted means
    for min_members in (1, 2, 4):
        want = brute_force(b, 0.9, min_members)
        cat, bound = cm.catalog(b, 0.9, min_members)
        assert cat.shape[0] == len(want) and len(want) >= (10 if min_members < 4 else 3)
        assert [int(a) for a in cat["label"]] == [r[0] for r in want] and [int(a) for a in cat["members"]] == [r[1] for r in want]
        for row, r in enumerate(want):
            tol = lambda v: 4 * cm.U * abs(v) + 1e-300                 # both are the exact value rounded a few times
            assert abs(cat["mass"][row] - r[2]) <= tol(r[2])
            for d in range(2):
                assert abs(cat["pos"][row][d] - r[3][d]) <= tol(r[3][d]) and abs(cat["vel"][row][d] - r[4][d]) <= tol(r[4][d])
            assert cat["pos"][row][2] == 0 and cat["vel"][row][2] == 0
            assert abs(cat["sigma2"][row] - r[5]) <= 64 * cm.U * r[5] + 1e-300 and abs(cat["r_max"][row] - r[6]) <= 64 * cm.U * r[6] + 1e-300
            assert (bound["mass"][row] >= 0) and (bound["pos"][row] >= 0).all() and bound["sigma2"][row] >= 0 and bound["r_max"][row] >= 0
    cat, _ = cm.catalog(b, 0.9, 1)
    massless = cat[cat["label"] == 120][0]
    assert massless["members"] == 4 and massless["mass"] == 0 and massless["r_max"] == 0 and massless["pos"].tolist() == [50.0, 50.0, 0.0]
    assert np.allclose(massless["vel"][:2], b["vel"][120:124].astype(np.float64).mean(axis=0), rtol=1e-15, atol=0)
    assert (cat["members"] == 1).any() and cat["members"].sum() == 200


def test_model_massless_group_and_exact_zeros():
    b = nb.bodies_array(5)
    b["pos"] = [[1.5, 2.5]] * 3 + [[100.0, 0.0], [100.25, 0.0]]
    b["vel"] = [[0.5, -1.0], [0.25, 3.0], [7.0, 7.0], [2.0, 1.0], [2.0, 1.0]]
    b["mass"] = [0.75, 1.5, 1.25, 0.0, 0.0]
    cat, bound = cm.catalog(b, 0.5, 2)
    assert cat["label"].tolist() == [0, 3] and cat["members"].tolist() == [3, 2]
    assert cat["r_max"][0] == 0.0 and cat["pos"][0].tolist() == [1.5, 2.5, 0.0] and cat["mass"][0] == 3.5
    assert cat["mass"][1] == 0.0 and cat["pos"][1].tolist() == [100.125, 0.0, 0.0] and cat["vel"][1].tolist() == [2.0, 1.0, 0.0]
    assert cat["sigma2"][1] == 0.0 and cat["r_max"][1] == 0.125
