"""CPU: the numpy statement of the Barnes-Hut force (tests/tree_model.py) against the reference's own step() — the committed
goldens and the live compiled reference — the argument the GPU build rests on (the tree does not depend on the body order), and
the ABI additions of NB_FORCE_TREE."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tree_model as tm  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"
COLS = ("x", "y", "vx", "vy", "ax", "ay")


def state_of(flat):
    return {k: np.ascontiguousarray(flat[:, i], np.float32) for i, k in enumerate(COLS + ("m", "r"))}


def assert_bits(st, want, what):
    for i, k in enumerate(COLS):
        got, ref = np.ascontiguousarray(st[k], np.float32), np.ascontiguousarray(want[:, i], np.float32)
        bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8]} ({got[bad[:4]]} vs {ref[bad[:4]]})"


@pytest.mark.parametrize("canonical", [True, False])
def test_model_equals_the_reference_step_goldens(canonical):
    st = state_of(np.load(GOLD / "ic_plummer_1024.npy"))
    done = 0
    for steps in (1, 10, 100) if canonical else (1, 10):
        tm.step(st, 0.05, 1e-3, steps - done, canonical=canonical)
        done = steps
        assert_bits(st, np.load(GOLD / f"ref_step_s{steps}.npy"), f"step {steps}")


def _live(flat, eps, dt, steps):
    import nbo
    if not nbo.have_ref():
        pytest.skip("the compiled reference is not built here")
    f = np.ascontiguousarray(flat.copy())
    assert nbo.ref().ref_step(f.reshape(-1), f.shape[0], eps, dt, steps) == steps
    return f


def test_model_equals_the_live_reference_on_random_bodies():
    flat = np.load(GOLD / "ic_random_333.npy").astype(np.float32)
    flat[:, 7] = 0.0                                              # radius 0: collide() stays out
    want = _live(flat, 0.5, 1e-3, 3)
    assert_bits(tm.step(state_of(flat), 0.5, 1e-3, 3), want, "random 333")


def test_model_equals_the_live_reference_on_default_bodies():
    flat = np.load(GOLD / "default_ics_first4096.npy").astype(np.float32)
    flat[:, 7] = 0.0
    want = _live(flat, 1.0, 0.01, 2)
    assert_bits(tm.step(state_of(flat), 1.0, 0.01, 2, clamp=True), want, "default 4096")


def test_serial_insertion_equals_canonical_construction_under_permutation():
    rng = np.random.default_rng(5)
    n = 400
    x = rng.normal(0, 1, n).astype(np.float32)
    y = rng.normal(0, 1, n).astype(np.float32)
    m = rng.uniform(0.5, 2.0, n).astype(np.float32)
    x[50:60], y[50:60] = x[40], y[40]                             # coincident bodies, different masses
    x[70], y[70] = x[71], np.nextafter(y[71], np.float32(9))      # a pair one ulp apart
    base = tm.accelerations(x, y, m, 0.05, canonical=True)
    for trial in range(20):
        p = rng.permutation(n)
        # coincident bodies keep their relative order (their masses add up in index order, as in the reference)
        p[np.sort(np.nonzero(np.isin(p, np.arange(50, 60) + 0) | (p == 40))[0])] = np.concatenate([[40], np.arange(50, 60)])
        for canonical in (True, False):
            ax, ay = tm.accelerations(x[p], y[p], m[p], 0.05, canonical=canonical)
            assert tm.same_bits(ax, base[0][p]) and tm.same_bits(ay, base[1][p]), (trial, canonical)


def test_coincident_bodies_share_a_leaf_in_index_order():
    x = np.array([0, 1, 1, 1, -1], np.float32)
    y = np.array([0, 2, 2, 2, -1], np.float32)
    m = np.array([1, 1e8, 1, 1, 1], np.float32)
    for build in (tm.build_canonical, tm.build_serial):
        t = build(x, y, m)
        leaf = np.nonzero((t["px"] == 1) & (t["py"] == 2) & (t["child"] == 0))[0]
        assert leaf.size == 1 and t["mass"][leaf[0]] == np.float32(np.float32(np.float32(1e8) + np.float32(1)) + np.float32(1))
    # the other order rounds differently: the sum follows the body index
    t = tm.build_canonical(x, y, np.array([1, 1, 1, 1e8, 1], np.float32))
    leaf = np.nonzero((t["px"] == 1) & (t["py"] == 2) & (t["child"] == 0))[0]
    assert t["mass"][leaf[0]] == np.float32(np.float32(2) + np.float32(1e8))


def test_quadrant_boundaries_are_strict():
    # root centre (0, 0): a body ON a centre line belongs to the lower quadrant of that axis (x > cx, y > cy are strict)
    x = np.array([-2, 2, 0, 0, 1], np.float32)
    y = np.array([-2, 2, 0, 1, 0], np.float32)
    d = tm.path_digits(x, y, tm.root_cell(x, y), 1)[:, 0]
    assert list(d) == [0, 3, 0, 2, 1]
    m = np.ones(5, np.float32)
    a, b = tm.accelerations(x, y, m, 0.1, canonical=True), tm.accelerations(x, y, m, 0.1, canonical=False)
    assert tm.same_bits(a[0], b[0]) and tm.same_bits(a[1], b[1])


def test_massless_body_is_a_tracer():
    rng = np.random.default_rng(1)
    x, y = rng.normal(0, 1, (2, 64)).astype(np.float32)
    m = np.ones(64, np.float32)
    m[10] = 0.0
    t = tm.build_canonical(x, y, m)
    assert not ((t["px"] == x[10]) & (t["py"] == y[10])).any()
    ax, _ = tm.walk(t, x, y, 0.05)
    assert ax[10] != 0


def test_abi_additions():
    lib = nb.load()
    assert lib.nb_abi_version() == 8 == L.NB_ABI_VERSION
    p = L.default_params()
    assert p.force == L.NB_FORCE_DIRECT == 0 and p.theta == 1.0 and L.NB_FORCE_TREE == 1
    assert p.struct_size == C.sizeof(L.nb_params) and C.sizeof(L.nb_params) % 8 == 0
    assert L.nb_params.force.offset == L.nb_params.pos_rows.offset + 8 and L.nb_params.theta.offset == L.nb_params.force.offset + 4
    assert hasattr(lib, "nb_tree_stats")
    header = (Path(__file__).resolve().parents[1] / "include" / "nbody.h").read_text()
    assert "#define NB_ABI_VERSION 8" in header and "NB_FORCE_TREE = 1" in header


def test_create_refuses_bad_tree_parameters_before_looking_for_a_device():
    lib = nb.load()
    b = nb.bodies_array(16)
    b["mass"] = 1.0
    for field, value, text in (("force", 2, b"bad force"), ("theta", -1.0, b"theta"), ("theta", float("nan"), b"theta"),
                               ("theta", float("inf"), b"theta")):
        p = L.default_params()
        setattr(p, field, value)
        assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
        assert lib.nb_last_error_code() == L.NB_EINVAL and text in lib.nb_last_error()
    for change, text in ((dict(precision=L.NB_FP64), b"NB_FP64"), (dict(dims=3), b"dims = 3"), (dict(shard_world=2, shard_rank=0), b"shard_world"),
                         (dict(i_begin=0, i_count=8), b"i_count < n"), (dict(integrator=L.NB_INTEGRATOR_KDK), b"KDK"),
                         (dict(sum_order=L.NB_SUM_SEQUENTIAL, rsqrt_mode=L.NB_RSQRT_QUAKE), b"NB_SUM_SEQUENTIAL"),
                         (dict(flags=L.NB_FLAG_SHARD_SINGLE), b"NB_FLAG_SHARD_SINGLE")):
        p = L.default_params()
        p.force = L.NB_FORCE_TREE
        for k, v in change.items():
            setattr(p, k, v)
        assert not lib.nb_create(b.ctypes.data, 16, C.byref(p))
        assert lib.nb_last_error_code() == L.NB_EINVAL and text in lib.nb_last_error() and b"NB_FORCE_TREE" in lib.nb_last_error(), lib.nb_last_error()
