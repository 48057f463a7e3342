"""CPU: the collision bit's parameter checks, the numpy restatement's two schedules, and the restatement against the
reference's own step() (stored fixtures, and the live reference where it is built)."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import collide_model as cm  # noqa: E402

GOLD = HERE / "golden"
FIXTURES = {   # tools/make_collide_golden.py
    "collide_isolated_ic.npy": "9c80c96768bb6d3c48498b9c7378bf0c9e749b2228c0c4d71c4da703fc7b379a",
    "collide_isolated_s1.npy": "d831c6d5ff9d989d22d29e9488e77887f42a3f84eec286c0bf6610d7fb5e529b",
    "collide_isolated_s3.npy": "985c37aace16554db8a66fbf4eb816238619d9ff2b64cdb4b8fb895edfa9454d",
}
EPS, DT = 1.0, 1.0 / 64.0


def test_collide_bit_passes_validation():
    """NB_EXTRA_COLLIDE is a known bit: nb_create gets past parameter validation to the device lookup.  The device ordinal is
    out of range, so no handle is created whether or not a GPU is visible: NB_ENODEVICE without one, the ordinal's error
    with one."""
    lib = nb.load()
    b = nb.plummer_2d(64, 1)
    p = L.default_params()
    p.extras = L.NB_EXTRA_COLLIDE | L.NB_EXTRA_VCLAMP | L.NB_EXTRA_BOUNDARY
    p.device = 9999
    assert not lib.nb_create(b.ctypes.data, 64, C.byref(p))
    if lib.nb_device_count() > 0:
        assert b"device 9999 out of range" in lib.nb_last_error(), lib.nb_last_error()
    else:
        assert lib.nb_last_error_code() == L.NB_ENODEVICE, lib.nb_last_error()
    p = L.default_params()
    p.extras = 8                                             # still unknown
    assert not lib.nb_create(b.ctypes.data, 64, C.byref(p)) and lib.nb_last_error_code() == L.NB_EINVAL


@pytest.mark.parametrize("field,value", [("dims", 3), ("integrator", L.NB_INTEGRATOR_KDK), ("shard_world", 2), ("i_count", 32),
                                         ("flags", L.NB_FLAG_SHARD_SINGLE)])
def test_collide_unsupported_combinations_are_refused(field, value):
    lib = nb.load()
    b = nb.plummer_2d(64, 1)
    p = L.default_params()
    p.extras = L.NB_EXTRA_COLLIDE
    setattr(p, field, value)
    if field == "flags":
        p.shard_world = 1
    assert not lib.nb_create(b.ctypes.data, 64, C.byref(p))
    assert lib.nb_last_error_code() == L.NB_EINVAL and b"collisions" in lib.nb_last_error(), lib.nb_last_error()


def test_dump_header_keeps_the_collide_bit(tmp_path):
    lib = nb.load()
    b = nb.plummer_2d(16, 3)
    p = L.default_params()
    p.extras = L.NB_EXTRA_COLLIDE | L.NB_EXTRA_VCLAMP
    path = tmp_path / "c.nbd"
    assert lib.nb_write_bodies(str(path).encode(), b.ctypes.data, 16, 7, C.byref(p)) == L.NB_OK
    _, frame, q = nb.read_bodies(path)
    assert frame == 7 and q.extras == L.NB_EXTRA_COLLIDE | L.NB_EXTRA_VCLAMP


def random_state(n, seed, dtype, spread, rmax):
    rng = np.random.default_rng(seed)
    return {"x": rng.uniform(-spread, spread, n).astype(dtype), "y": rng.uniform(-spread, spread, n).astype(dtype),
            "vx": rng.normal(0, 3, n).astype(dtype), "vy": rng.normal(0, 3, n).astype(dtype),
            "m": (10.0 ** rng.uniform(-3, 0, n)).astype(dtype), "r": rng.uniform(0, rmax, n).astype(np.float32)}


def chain_state(n, dtype):
    st = {"x": (1.9 * np.arange(n)).astype(dtype), "y": np.zeros(n, dtype), "vx": np.where(np.arange(n) % 2, -1.0, 1.0).astype(dtype),
          "vy": np.full(n, 0.25, dtype), "m": np.linspace(1, 3, n).astype(dtype), "r": np.ones(n, np.float32)}
    st["x"][5] = st["x"][4]                                  # a coincident pair inside the chain
    st["y"][5] = st["y"][4]
    return st


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["clump", "chain"])
def test_round_schedule_equals_the_sequential_pass(dtype, case):
    st = random_state(600, 11, dtype, 12.0, 1.2) if case == "clump" else chain_state(120, dtype)
    P = cm.pairs(st["x"], st["y"], st["r"])
    assert len(P) > 100
    a = {k: v.copy() for k, v in st.items()}
    b = {k: v.copy() for k, v in st.items()}
    cm.resolve_sequential(a, P)
    rounds = cm.resolve_rounds(b, P)
    for k in ("x", "y", "vx", "vy"):
        assert cm.same_bits(a[k], b[k]), k
    assert not cm.same_bits(a["x"], st["x"]) and not cm.same_bits(a["vx"], st["vx"])
    assert rounds < len(P) if case == "clump" else rounds >= 100


def test_pairs_brute_force_sorted_and_complete():
    st = random_state(700, 5, np.float32, 10.0, 1.0)
    P = cm.pairs(st["x"], st["y"], st["r"], chunk=64)
    x, y, r = st["x"].astype(np.float64), st["y"].astype(np.float64), st["r"].astype(np.float64)
    d2 = (x[None, :] - x[:, None]) ** 2 + (y[None, :] - y[:, None]) ** 2
    near = np.abs(d2 - (r[:, None] + r[None, :]) ** 2) > 1e-3        # away from the rounding edge, fp64 decides
    want = {(i, j) for i, j in zip(*np.nonzero((d2 <= (r[:, None] + r[None, :]) ** 2) & near)) if i < j}
    got = {tuple(p) for p in P.tolist()}
    assert want <= got and all(((i, j) in want) or not near[i, j] for i, j in got)
    assert np.all(np.diff(P[:, 0] * 10**6 + P[:, 1]) > 0)


def load_fixture(name):
    path = GOLD / name
    assert hashlib.sha256(path.read_bytes()).hexdigest() == FIXTURES[name], name
    return np.load(path)


def fixture_state(flat):
    return {"x": flat[:, 0].copy(), "y": flat[:, 1].copy(), "vx": flat[:, 2].copy(), "vy": flat[:, 3].copy(), "m": flat[:, 6].copy(),
            "r": flat[:, 7].copy()}


@pytest.mark.parametrize("rounds", [False, True])
def test_restatement_reproduces_the_reference_fixture(rounds):
    ic = load_fixture("collide_isolated_ic.npy")
    st = fixture_state(ic)
    for steps in (1, 2, 3):
        cm.drift(st, DT)
        n = cm.collide(st, rounds=rounds)
        if steps == 1:
            assert n == ic.shape[0] // 2                         # every pair overlaps after the first drift
        if steps in (1, 3):
            gold = load_fixture(f"collide_isolated_s{steps}.npy")
            for i, k in enumerate(("x", "y", "vx", "vy")):
                assert cm.same_bits(st[k], gold[:, i]), (steps, k)
    assert not cm.same_bits(st["vx"], ic[:, 2])


def test_restatement_equals_the_live_reference():
    sys.path.insert(0, str(HERE.parent / "oracle"))
    import nbo
    if not nbo.have_ref():
        pytest.skip("the compiled reference is not built here (fixtures above cover it)")
    ic = load_fixture("collide_isolated_ic.npy")
    rng = np.random.default_rng(9)
    ic = ic.copy()
    ic[:, 2:4] *= rng.uniform(0.5, 1.5, (ic.shape[0], 2)).astype(np.float32)     # other speeds than the fixture's
    f = np.ascontiguousarray(ic.copy())
    assert nbo.ref().ref_step(f.reshape(-1), f.shape[0], EPS, DT, 2) == 2
    st = fixture_state(ic)
    for _ in range(2):
        cm.drift(st, DT)
        cm.collide(st)
    for i, k in enumerate(("x", "y", "vx", "vy")):
        assert cm.same_bits(st[k], f[:, i]), k
