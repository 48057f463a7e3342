"""CPU: the numpy statement of the quadrupole term of the convergent Barnes-Hut force (tests/tree_quad_model.py,
NB_FLAG_TREE_QUADRUPOLE) — the moment recurrence against a float64 brute force, the term against a finite difference of the
expanded potential, what the term buys against the float64 direct sum — and the interface additions."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
import tree_leaves_model as tlm  # noqa: E402
import tree_model as tm  # noqa: E402
import tree_quad_model as tqm  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"
_cache = {}


def case(file):
    """(x, y, m, tree, moments) of a fixture, built once and shared (nothing below writes into it)."""
    if file not in _cache:
        flat = np.load(GOLD / file).astype(np.float32)
        x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
        tree = tm.build_canonical(x, y, m)
        _cache[file] = (x, y, m, tree, tqm.moments(tree))
    return _cache[file]


# ---------------------------------------------------------------------------------------------------------------------
# 1: moments
# ---------------------------------------------------------------------------------------------------------------------
MOMENT_BAR = 4.98e-4


@pytest.mark.parametrize("file", ["ic_random_333.npy", "ic_plummer_1024.npy", "default_ics_first4096.npy"])
def test_moments_against_a_float64_brute_force(file):
    """Per branch, max |M_model - M_f64| over xx, xy, yy relative to tr(M_f64), M_f64 = sum m (y - c)(y - c)^T over the leaves of
    the subtree in float64 about the node's stored (float32) centre.  Measured worst values: ic_random_333 2.75e-6,
    ic_plummer_1024 1.55e-6, default_ics_first4096 1.245e-4 (median 5e-8 on all three; the cells around the 1e9 central mass carry
    the worst: the parallel-axis step takes a child's ROUNDED centre for its centre of mass, and the dipole that leaves about it
    is the heavy mass times an ulp of its position).  The bar is 4 x the worst seen, 4.98e-4, for float32 accumulation over up to
    63 levels.  Leaves and empty quadrants have zeros."""
    x, y, m, tree, mom = case(file)
    px, py, mass, child = (tree[k] for k in ("px", "py", "mass", "child"))
    end = tlm.subtree_end(tree)
    leaves = np.nonzero(child == 0)[0]
    lx, ly, lm = (a[leaves].astype(np.float64) for a in (px, py, mass))
    branches = np.nonzero(child != 0)[0]
    worst = 0.0
    for i in branches:
        a, b = np.searchsorted(leaves, [i, end[i]])
        sx, sy, w = lx[a:b] - float(px[i]), ly[a:b] - float(py[i]), lm[a:b]
        ref = np.array([(w * sx * sx).sum(), (w * sx * sy).sum(), (w * sy * sy).sum()])
        worst = max(worst, np.abs(mom[i].astype(np.float64) - ref).max() / (ref[0] + ref[2]))
    print(f"{file}: {branches.size} branches, worst moment error {worst:.3g} of tr(M)")
    assert mom.dtype == np.float32 and mom.shape == (px.shape[0], 3)
    assert not mom[child == 0].any()
    assert worst <= MOMENT_BAR


# ---------------------------------------------------------------------------------------------------------------------
# 2: the term
# ---------------------------------------------------------------------------------------------------------------------
def test_the_term_is_the_gradient_of_the_second_order_potential():
    """A cell of 20 points (the root of its own tree), eps = 0.05, far positions at 3 to 12 cell sizes.  With d = c - position
    the expansion of sum m_k (|d + s_k|^2 + eps^2)^(-1/2) about the centre of mass is f(d) = m / R + 1.5 d^T M d / R^5 -
    0.5 tr(M) / R^3 and the acceleration is -grad_d f.  The float64 term equals a centred difference of f (step 1e-5 |d|: the
    truncation error is 1e-10 relative, the bar 1e-7), on the whole term and on its quadrupole part alone; the float32 model
    term, Quake rsqrt excepted, equals the float64 one to 1e-5 of |a| (some twenty float32 roundings of 6e-8 each); and the
    term is closer to the sum over the 20 points than the monopole alone at every position."""
    rng = np.random.default_rng(5)
    k, eps = 20, 0.05
    x = rng.uniform(-0.5, 0.5, k).astype(np.float32)
    y = rng.uniform(-0.5, 0.5, k).astype(np.float32)
    m = rng.uniform(0.5, 2.0, k).astype(np.float32)
    tree = tm.build_canonical(x, y, m)
    mom = tqm.moments(tree)
    assert tree["child"][0] != 0
    cx, cy, cm, M = float(tree["px"][0]), float(tree["py"][0]), float(tree["mass"][0]), mom[0].astype(np.float64)

    def f(dx, dy, quad=1.0, mono=1.0):
        r2 = dx * dx + dy * dy + eps * eps
        rmr = M[0] * dx * dx + 2 * M[1] * dx * dy + M[2] * dy * dy
        return mono * cm * r2 ** -0.5 + quad * (1.5 * rmr * r2 ** -2.5 - 0.5 * (M[0] + M[2]) * r2 ** -1.5)

    ang = np.array([0.3, 1.1, 2.0, 2.9, 4.0, 5.5])
    rad = np.array([3.0, 4.5, 6.0, 8.0, 10.0, 12.0])
    bx, by = cx + rad * np.cos(ang), cy + rad * np.sin(ang)
    dx, dy = cx - bx, cy - by
    one = np.repeat(M[None, :], ang.size, axis=0)
    ax, ay = tqm.term_f64(np.full(ang.size, cm), one, dx, dy, eps)
    mx, my = tqm.term_f64(np.full(ang.size, cm), np.zeros_like(one), dx, dy, eps)
    h = 1e-5 * rad
    for quad, gx, gy in ((1.0, ax, ay), (0.0, mx, my)):
        fx = -(f(dx + h, dy, quad) - f(dx - h, dy, quad)) / (2 * h)
        fy = -(f(dx, dy + h, quad) - f(dx, dy - h, quad)) / (2 * h)
        assert (np.hypot(gx - fx, gy - fy) <= 1e-7 * np.hypot(fx, fy)).all()
    qfx = -(f(dx + h, dy, 1.0, 0.0) - f(dx - h, dy, 1.0, 0.0)) / (2 * h)
    qfy = -(f(dx, dy + h, 1.0, 0.0) - f(dx, dy - h, 1.0, 0.0)) / (2 * h)
    assert (np.hypot(ax - mx - qfx, ay - my - qfy) <= 1e-7 * np.hypot(qfx, qfy)).all()
    # the float32 term of the model
    F = np.float32
    dx32, dy32 = (F(cx) - bx.astype(F)), (F(cy) - by.astype(F))
    d2 = dx32 * dx32 + dy32 * dy32
    tx, ty = tqm.term(np.full(ang.size, cm, F), one.astype(F), dx32, dy32, d2, F(F(eps) * F(eps)), quake=False)
    wx, wy = tqm.term_f64(np.full(ang.size, cm), one, dx32.astype(np.float64), dy32.astype(np.float64), float(F(eps)))
    assert tx.dtype == F and (np.hypot(tx - wx, ty - wy) <= 1e-5 * np.hypot(wx, wy)).all()
    # against the 20 points themselves
    sx, sy = x.astype(np.float64)[None, :] - bx[:, None], y.astype(np.float64)[None, :] - by[:, None]
    w = m.astype(np.float64)[None, :] * (sx * sx + sy * sy + eps * eps) ** -1.5
    ex, ey = (sx * w).sum(axis=1), (sy * w).sum(axis=1)
    assert (np.hypot(ax - ex, ay - ey) < np.hypot(mx - ex, my - ey)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3: what it buys
# ---------------------------------------------------------------------------------------------------------------------
def median_error(theta, group, quad):
    key = ("payoff", theta, group, quad)
    if key not in _cache:
        import nbo
        x, y, m, tree, mom = case("ic_plummer_4096.npy")
        eps = 0.05
        if "direct" not in _cache:
            st = {"x": x.astype(np.float64), "y": y.astype(np.float64), "m": m.astype(np.float64)}
            _cache["direct"] = nbo.accel_f64(st, eps)
        ex, ey = _cache["direct"]
        if quad:
            ax, ay = tqm.walk(tree, mom, x, y, m, eps, theta, quake=False, group=group)
        else:
            ax, ay = tlm.walk(tree, x, y, m, eps, theta, quake=False, group=group)
        _cache[key] = float(np.median(np.hypot(ax - ex, ay - ey) / np.hypot(ex, ey)))
    return _cache[key]


@pytest.mark.parametrize("group", [None, 64])
def test_the_quadrupole_term_pays(group):
    """ic_plummer_4096, eps 0.05, the float32 model with the exact rsqrt and float32 moments; per body the error relative to its
    own float64 direct-sum |a|.  The median with the term is at most a quarter of the median without it at theta 0.7 and 0.5, and
    with the term at theta = 0.7 it is below the monopole's at theta = 0.5 (float64 moments give 9-34 x and 2-7 x)."""
    med = {(t, q): median_error(t, group, q) for t in (0.7, 0.5) for q in (False, True)}
    print(f"group {group}: " + ", ".join(f"theta {t} {'quadrupole' if q else 'monopole'} {v:.3g}" for (t, q), v in med.items()))
    for t in (0.7, 0.5):
        assert med[t, True] <= 0.25 * med[t, False], t
    assert med[0.7, True] < med[0.5, False]


def test_the_model_walk_without_branches_is_the_leaves_walk():
    """theta = 0 accepts no cell: the bits of tree_leaves_model.walk, both rsqrt forms, both walks."""
    x, y, m, tree, mom = case("ic_random_333.npy")
    for quake in (True, False):
        for group in (None, 64):
            a = tqm.walk(tree, mom, x, y, m, 0.5, 0.0, quake, group)
            b = tlm.walk(tree, x, y, m, 0.5, 0.0, quake, group)
            assert tm.same_bits(a[0], b[0]) and tm.same_bits(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# 4: interface
# ---------------------------------------------------------------------------------------------------------------------
def test_interface_additions():
    lib = nb.load()
    assert lib.nb_abi_version() == 8 == L.NB_ABI_VERSION
    assert L.NB_FLAG_TREE_QUADRUPOLE == 8192
    header = (Path(__file__).resolve().parents[1] / "include" / "nbody.h").read_text()
    assert "NB_FLAG_TREE_QUADRUPOLE = 8192" in header and "#define NB_ABI_VERSION 8" in header
    b = nb.bodies_array(16)
    b["mass"] = 1.0
    # alone; with the leaves bit but the direct force; with the tree force but without the leaves bit
    for force, flags, partner in ((L.NB_FORCE_DIRECT, 8192, b"NB_FLAG_TREE_LEAVES"), (L.NB_FORCE_DIRECT, 8192 | 4096, b"NB_FORCE_DIRECT"),
                                  (L.NB_FORCE_TREE, 8192, b"NB_FLAG_TREE_LEAVES")):
        p = L.default_params()
        p.force, p.flags = force, flags
        assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))             # refused before a device is looked for
        assert lib.nb_last_error_code() == L.NB_EINVAL
        assert b"NB_FLAG_TREE_QUADRUPOLE" in lib.nb_last_error() and partner in lib.nb_last_error(), lib.nb_last_error()
    p = L.default_params()
    p.flags = 2048                                                            # stays an unknown bit
    assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
    assert lib.nb_last_error_code() == L.NB_EINVAL and b"unknown bits" in lib.nb_last_error()
    # every refusal of a leaves handle holds with the bit
    for field, value, text in (("precision", L.NB_FP64, b"NB_FP64"), ("dims", 3, b"dims = 3"), ("integrator", L.NB_INTEGRATOR_KDK, b"KDK"),
                               ("shard_world", 2, b"shard_world"), ("i_count", 8, b"i_count < n"), ("sum_order", L.NB_SUM_SEQUENTIAL, b"NB_SUM_SEQUENTIAL")):
        p = L.default_params()
        p.force, p.flags = L.NB_FORCE_TREE, L.NB_FLAG_TREE_LEAVES | L.NB_FLAG_TREE_QUADRUPOLE
        setattr(p, field, value)
        assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
        assert lib.nb_last_error_code() == L.NB_EINVAL and text in lib.nb_last_error() and b"NB_FORCE_TREE" in lib.nb_last_error(), field
    with pytest.raises(ValueError):
        nb.Simulation(b, force="tree", tree_quadrupole=True)
    with pytest.raises(ValueError):
        nb.Simulation(b, force="direct", tree_leaves=False, tree_quadrupole=True)
