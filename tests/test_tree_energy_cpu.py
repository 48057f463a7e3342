"""CPU: the numpy statement of the tree potential energy (tests/tree_energy_model.py, NB_FLAG_TREE_ENERGY) — at theta = 0 against
a float64 brute force over all pairs, its quadrupole term against the force term it is the potential of, what the moments buy
against the direct energy — and the interface additions."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tree_energy_model as tem  # noqa: E402
import tree_model as tm  # noqa: E402
import tree_quad_model as tqm  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"
_cache = {}


def small_cases():
    """The small cases of tests/test_tree_leaves_gpu.py (the same generator, restated: a GPU test module is not imported here)."""
    rng = np.random.default_rng(11)
    n = 300
    flat = np.zeros((n, 8), np.float32)
    flat[:, 0:2] = rng.normal(0, 1, (n, 2))
    flat[:, 6] = rng.uniform(0.5, 2.0, n)
    co = flat.copy()
    co[100:110, 0:2] = co[99, 0:2]                           # ten bodies on one position, different masses
    co[100, 6] = 1e8
    tracer = flat.copy()
    tracer[[5, 77, 299], 6] = 0.0
    point = flat[:40].copy()
    point[:, 0:2] = point[0, 0:2]
    pair = flat[:2].copy()                                   # nothing but two bodies on one position
    pair[1, 0:2] = pair[0, 0:2]
    return {"coincident": co, "tracer": tracer, "one": flat[:1].copy(), "two": flat[:2].copy(), "one_point": point, "coincident_pair": pair}


def inputs(name):
    """(x, y, m, eps, positions are shared) of a fixture file or a small case."""
    if name.endswith(".npy"):
        flat, eps = np.load(GOLD / name).astype(np.float32), {"ic_random_333.npy": 0.5, "ic_plummer_1024.npy": 0.05}[name]
    else:
        flat, eps = small_cases()[name], 0.05
    x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
    ins = m != 0
    shared = np.unique(np.stack([x[ins], y[ins]], axis=1), axis=0).shape[0] < int(ins.sum())
    return x, y, m, eps, shared


# ---------------------------------------------------------------------------------------------------------------------
# 1: theta = 0 is the brute force
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ic_random_333.npy", "ic_plummer_1024.npy", "coincident", "tracer", "one", "two", "one_point", "coincident_pair"])
def test_the_model_at_theta_zero_is_the_brute_force(name):
    """No cell is accepted: every leaf adds -m / R and the partners on the body's own position -m / eps each.  Without shared
    positions every leaf is one body and the sums differ by float64 rounding: 1e-12.  A shared leaf's record carries the float32 sum
    of its k masses, (k - 1) 2^-24 relative at most: 2e-6 covers k <= 40.  The model (leaf_mass) takes such a leaf's mass as the
    float64 sum to 2^-48, so it stays far inside that; on ic_random_333, which holds one pair on one position, it meets the 1e-10
    that tests/test_tree_energy_gpu.py asks of the kernel against a direct handle there."""
    x, y, m, eps, shared = inputs(name)
    want = tem.direct(x, y, m, eps)
    for quad in (False, True):
        got = tem.potential(x, y, m, eps, 0.0, quad)
        print(f"{name} quad {quad}: U {got:.15e} brute force {want:.15e}")
        assert abs(got - want) <= (2e-6 if shared else 1e-12) * abs(want)
        if name == "ic_random_333.npy":
            assert shared and abs(got - want) <= 1e-10 * abs(want)
    if name == "one":
        assert got == 0.0
    if name == "coincident_pair":
        assert abs(got + float(m[0]) * float(m[1]) / float(np.float32(eps))) <= 1e-15 * abs(got)
    if name == "coincident_pair" or name == "one_point":     # eps = 0: the pairs on one position are skipped, the result is finite
        assert tem.potential(x, y, m, 0.0, 0.0, False) == 0.0
    if name == "two":
        assert abs(tem.potential(x, y, m, 0.0, 0.0, False) - tem.direct(x, y, m, 0.0)) <= 1e-15 * abs(want)


# ---------------------------------------------------------------------------------------------------------------------
# 2: the term
# ---------------------------------------------------------------------------------------------------------------------
def test_the_force_term_is_the_gradient_of_the_potential_term():
    """Random d (|d| 3 .. 12), M (a sum of outer products), m and eps: a centred difference of the potential term in d (step
    1e-5 |d|: truncation 1e-10 relative) equals tree_quad_model.term_f64, the force term, to 1e-6; so does the monopole form
    with M = 0."""
    rng = np.random.default_rng(23)
    k = 64
    ang, rad = rng.uniform(0, 2 * np.pi, k), rng.uniform(3.0, 12.0, k)
    dx, dy = rad * np.cos(ang), rad * np.sin(ang)
    s = rng.uniform(-0.5, 0.5, (k, 20, 2))
    w = rng.uniform(0.5, 2.0, (k, 20))
    mom = np.stack([(w * s[:, :, 0] ** 2).sum(1), (w * s[:, :, 0] * s[:, :, 1]).sum(1), (w * s[:, :, 1] ** 2).sum(1)], axis=1).astype(np.float32)
    mass = w.sum(1)
    h = 1e-5 * rad
    for eps in (0.0, 0.05, 0.5):
        for mm in (mom, np.zeros_like(mom)):
            gx = (tem.term(mass, mm, dx + h, dy, eps) - tem.term(mass, mm, dx - h, dy, eps)) / (2 * h)
            gy = (tem.term(mass, mm, dx, dy + h, eps) - tem.term(mass, mm, dx, dy - h, eps)) / (2 * h)
            ax, ay = tqm.term_f64(mass, mm, dx, dy, float(np.float32(eps)))
            assert (np.hypot(gx - ax, gy - ay) <= 1e-6 * np.hypot(ax, ay)).all()
    # the quadrupole part on its own is not lost in the monopole
    q = tem.term(mass, mom, dx, dy, 0.05) - tem.term(mass, np.zeros_like(mom), dx, dy, 0.05)
    assert (np.abs(q) > 1e-6 * np.abs(tem.term(mass, mom, dx, dy, 0.05))).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3: what the moments buy
# ---------------------------------------------------------------------------------------------------------------------
def payoff(theta, quad):
    if "payoff" not in _cache:
        x, y, m, eps, _ = inputs("ic_plummer_1024.npy")
        eps = 0.05
        tree = tm.build_canonical(x, y, m)
        _cache["payoff"] = (x, y, m, eps, tree, tqm.moments(tree), tem.direct(x, y, m, eps))
    x, y, m, eps, tree, mom, want = _cache["payoff"]
    key = ("payoff", theta, quad)
    if key not in _cache:
        _cache[key] = abs(tem.potential(x, y, m, eps, theta, quad, tree, mom) - want) / abs(want)
    return _cache[key]


def test_payoff_ordering():
    """ic_plummer_1024, eps = 0.05, |U_model(theta) - U_direct| / |U_direct|: smaller with the moments than without at theta 0.5
    and 1.0, and for either form smaller at theta 0.3 than at theta 1.0."""
    err = {(t, q): payoff(t, q) for t in (1.0, 0.5, 0.3) for q in (False, True)}
    print(", ".join(f"theta {t} {'quadrupole' if q else 'monopole'} {v:.3g}" for (t, q), v in err.items()))
    for t in (0.5, 1.0):
        assert err[t, True] < err[t, False], t
    for q in (False, True):
        assert err[0.3, q] < err[1.0, q], q


# ---------------------------------------------------------------------------------------------------------------------
# 4: interface
# ---------------------------------------------------------------------------------------------------------------------
def test_interface_additions():
    lib = nb.load()
    assert lib.nb_abi_version() == 8 == L.NB_ABI_VERSION
    assert L.NB_FLAG_TREE_ENERGY == 16384
    header = (Path(__file__).resolve().parents[1] / "include" / "nbody.h").read_text()
    assert "NB_FLAG_TREE_ENERGY = 16384" in header and "#define NB_ABI_VERSION 8" in header
    b = nb.bodies_array(16)
    b["mass"] = 1.0
    # with the leaves bit but the direct force; with the tree force but without the leaves bit; both
    for force, flags, partners in ((L.NB_FORCE_DIRECT, 16384 | 4096, (b"NB_FORCE_DIRECT",)), (L.NB_FORCE_TREE, 16384, (b"NB_FLAG_TREE_LEAVES",)),
                                   (L.NB_FORCE_DIRECT, 16384, (b"NB_FORCE_DIRECT", b"NB_FLAG_TREE_LEAVES")),
                                   (L.NB_FORCE_TREE, 16384 | 8192, (b"NB_FLAG_TREE_LEAVES",))):
        p = L.default_params()
        p.force, p.flags = force, flags
        assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))             # refused before a device is looked for
        assert lib.nb_last_error_code() == L.NB_EINVAL
        assert b"NB_FLAG_TREE_ENERGY" in lib.nb_last_error() and all(t in lib.nb_last_error() for t in partners), lib.nb_last_error()
    for flags in (2048, 2048 | 16384 | 4096):                                 # stays an unknown bit
        p = L.default_params()
        p.force, p.flags = L.NB_FORCE_TREE, flags
        assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
        assert lib.nb_last_error_code() == L.NB_EINVAL and b"unknown bits" in lib.nb_last_error()
    # every refusal of a tree handle holds with the bit, with and without the quadrupole bit
    for quad in (0, L.NB_FLAG_TREE_QUADRUPOLE):
        for field, value, text in (("precision", L.NB_FP64, b"NB_FP64"), ("dims", 3, b"dims = 3"), ("integrator", L.NB_INTEGRATOR_KDK, b"KDK"),
                                   ("shard_world", 2, b"shard_world"), ("i_count", 8, b"i_count < n"),
                                   ("sum_order", L.NB_SUM_SEQUENTIAL, b"NB_SUM_SEQUENTIAL")):
            p = L.default_params()
            p.force, p.flags = L.NB_FORCE_TREE, L.NB_FLAG_TREE_LEAVES | L.NB_FLAG_TREE_ENERGY | quad
            setattr(p, field, value)
            assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
            assert lib.nb_last_error_code() == L.NB_EINVAL and text in lib.nb_last_error() and b"NB_FORCE_TREE" in lib.nb_last_error(), field
    for kw in (dict(force="tree"), dict(force="direct"), dict(force="direct", tree_leaves=False), dict(force="tree", tree_leaves=False)):
        with pytest.raises(ValueError, match="tree_energy"):
            nb.Simulation(b, tree_energy=True, **kw)
    assert "tree_energy" in nb.Simulation.__init__.__doc__
