"""CPU: nb_groups — the interface (header, exported symbol, binding, the argument checks that need no device) and the numpy statement
of its contract (tests/groups_model.py) on hand-made cases with known answers."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import groups_model as gm  # noqa: E402
import neighbors_model as nm  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def test_header_declares_the_entry_point_and_keeps_the_abi_number():
    header = (ROOT / "include" / "nbody.h").read_text()
    assert "int nb_groups(nb_sim *s, float radius, uint32_t *label, uint32_t *size, uint64_t *ngroups);" in header
    assert "#define NB_ABI_VERSION 8" in header


def test_library_exports_the_symbol_and_the_bindings_exist():
    lib = nb.load()
    assert lib.nb_abi_version() == 8
    assert hasattr(lib, "nb_groups") and "nb_groups" in L.PROTOTYPES
    assert callable(getattr(nb.Simulation, "groups", None))
    syms = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T nb_groups\n" in syms
    hpp = (ROOT / "nbodysim_amd" / "host" / "Simulation.hpp").read_text()
    assert "void groups(float radius, uint32_t *label, uint32_t *size, uint64_t *ngroups)" in hpp and "nb_groups(sim_" in hpp


def test_null_handle_and_all_null_destinations_are_refused_without_a_device():
    lib = nb.load()
    plane = np.full(16, 0xDEADBEEF, np.uint32)
    count = C.c_uint64(77)
    assert lib.nb_groups(None, 1.0, plane.ctypes.data, None, C.byref(count)) == L.NB_EINVAL
    assert b"nb_groups: NULL handle" in lib.nb_last_error() and lib.nb_last_error_code() == L.NB_EINVAL
    assert lib.nb_groups(None, 1.0, None, None, None) == L.NB_EINVAL and b"NULL handle" in lib.nb_last_error()
    # the destinations and the radius are looked at before anything of the handle is: a block of zero bytes stands in for one here
    dummy = (C.c_uint8 * 65536)()
    assert lib.nb_groups(C.addressof(dummy), 1.0, None, None, None) == L.NB_EINVAL
    assert b"nb_groups: label, size and ngroups are all NULL" in lib.nb_last_error()
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.nb_groups(C.addressof(dummy), radius, plane.ctypes.data, None, None) == L.NB_EINVAL
        assert lib.nb_last_error().decode().startswith("nb_groups: radius must be finite and > 0"), radius
    for radius in (1e-30, 1e30):
        assert lib.nb_groups(C.addressof(dummy), radius, plane.ctypes.data, None, None) == L.NB_EINVAL
        assert lib.nb_last_error().decode().startswith("nb_groups: radius * radius must be finite and > 0 in float"), radius
    assert (plane == 0xDEADBEEF).all() and count.value == 77


# ---------------------------------------------------------------------------------------------------------------------
# the model on cases whose answers are known
# ---------------------------------------------------------------------------------------------------------------------
def test_model_two_bodies_at_the_radius_and_a_hair_below_it():
    r = np.float32(0.75)
    x, y = np.array([0.0, r], np.float32), np.zeros(2, np.float32)
    label, size, ng = gm.groups(x, y, r)
    assert label.tolist() == [0, 1] and size.tolist() == [1, 1] and ng == 2            # d2 == r2 is not < r2
    x[1] = np.nextafter(r, np.float32(0))
    label, size, ng = gm.groups(x, y, r)
    assert label.tolist() == [0, 0] and size.tolist() == [2, 2] and ng == 1
    assert label.dtype == np.uint32 and size.dtype == np.uint32


def test_model_chain_with_shuffled_indices_and_a_gap():
    n, r = 200, 1.0
    perm = np.random.default_rng(5).permutation(n)                 # body perm[t] sits at place t of the chain
    x = np.empty(n, np.float32)
    x[perm] = 0.75 * r * np.arange(n)
    y = np.zeros(n, np.float32)
    label, size, ng = gm.groups(x, y, r)
    assert (label == 0).all() and (size == n).all() and ng == 1
    x[perm[100]] = 1e6                                             # the chain breaks at place 100: two pieces and the body moved away
    label, size, ng = gm.groups(x, y, r)
    assert ng == 3
    left, right = perm[:100], perm[101:]
    assert (label[left] == left.min()).all() and (label[right] == right.min()).all() and label[perm[100]] == perm[100]
    assert (size[left] == 100).all() and (size[right] == 99).all() and size[perm[100]] == 1
    # the rows argument: a slice of the whole, ngroups of all
    part = gm.groups(x, y, r, rows=np.arange(50, 120))
    assert np.array_equal(part[0], label[50:120]) and np.array_equal(part[1], size[50:120]) and part[2] == 3


def test_model_non_finite_bodies_and_coincident_ones():
    x = np.array([0.0, 1.0, 1.0, np.nan, np.inf, 10.0, 2.0], np.float32)
    y = np.array([0.0, 0.0, 0.0, 0.0, 0.0, np.nan, 0.0], np.float32)
    label, size, ng = gm.groups(x, y, 1.5)
    assert label.tolist() == [0, 0, 0, 3, 4, 5, 0] and size.tolist() == [4, 4, 4, 1, 1, 1, 4] and ng == 4
    # strict: at radius 1 only the coincident pair stays linked
    label, size, ng = gm.groups(x, y, 1.0)
    assert label.tolist() == [0, 1, 1, 3, 4, 5, 6] and size.tolist() == [1, 2, 2, 1, 1, 1, 1] and ng == 6


def test_model_lattice_strictness():
    x, y = nm.lattice()
    assert gm.groups(x, y, 1.0)[2] == 256                          # d2 = 1 is not < 1
    label, size, ng = gm.groups(x, y, np.nextafter(np.float32(1), np.float32(2)))
    assert ng == 1 and (label == 0).all() and (size == 256).all()
    # one colour of the checkerboard: no axis links (d2 = 1) exist, the nearest sites are the diagonals (d2 = 2), then d2 = 4
    colour = ((x + y) % 2 == 0)
    label, size, ng = gm.groups(x[colour], y[colour], 1.5)         # r2 = 2.25: one group through the diagonals alone
    assert ng == 1 and (size == 128).all() and (label == 0).all()
    assert gm.groups(x[colour], y[colour], 1.25)[2] == 128         # r2 = 1.5625 < 2: nothing links


def test_model_link_matrix_is_neighbors_models_near_on_a_cloud():
    rng = np.random.default_rng(11)
    x, y = rng.uniform(-10, 10, (2, 400)).astype(np.float32)
    x[7], y[9] = np.nan, np.inf
    radius, n = 1.3, 400
    m = gm.link_matrix(x, y, radius)
    assert np.array_equal(m, m.T) and not m.diagonal().any()       # symmetric, bit for bit
    idx, _, cnt = nm.neighbors(x, y, radius, 32)
    assert cnt.max() <= 32 and cnt.max() > 3
    near = np.zeros((n, n), bool)
    rows = np.repeat(np.arange(n), 32)
    keep = idx.ravel() != nm.NO_NEIGHBOR
    near[rows[keep], idx.ravel()[keep]] = True
    assert np.array_equal(m, near) and np.array_equal(m.sum(axis=1), cnt)
    assert not m[7].any() and not m[9].any()
    # and the components agree with a union-find written another way
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    for a, b in zip(*np.nonzero(m)):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    want = np.array([find(a) for a in range(n)], np.uint32)
    label, size, ng = gm.groups(x, y, radius)
    assert np.array_equal(label, want) and ng == len(set(want.tolist()))
    assert np.array_equal(size, np.bincount(want, minlength=n)[want])
