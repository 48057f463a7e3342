"""GPU: hard-sphere collisions (NB_EXTRA_COLLIDE) against the reference's own step() and against the numpy restatement
(tests/collide_model.py), bit for bit."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import collide_model as cm  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
KEYS = (("x", "pos", 0), ("y", "pos", 1), ("vx", "vel", 0), ("vy", "vel", 1))


def bodies_of(flat: np.ndarray) -> np.ndarray:
    b = nb.bodies_array(flat.shape[0])
    b["pos"][:, 0], b["pos"][:, 1], b["vel"][:, 0], b["vel"][:, 1] = flat[:, 0], flat[:, 1], flat[:, 2], flat[:, 3]
    b["mass"], b["radius"] = flat[:, 6], flat[:, 7]
    return b


def assert_state(b: np.ndarray, st: dict, what: str, rows=slice(None)):
    for k, f, c in KEYS:
        got = np.ascontiguousarray(b[f][rows, c])
        want = np.ascontiguousarray(st[k][rows]).astype(np.float32)
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8]} ({got[bad[:4]]} vs {want[bad[:4]]})"


def stats(sim) -> dict:
    return sim.collision_stats()


def describe_resolve(sim) -> str:
    return sim.describe().rsplit("resolve=", 1)[1].split()[0]


# ---------------------------------------------------------------------------------------------------------------------
# 1. isolated pairs: the reference's real step(), 1 and 3 steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetry", [True, False])
def test_isolated_pairs_equal_the_reference_step(symmetry):
    ic = np.load(GOLD / "collide_isolated_ic.npy")
    npair = ic.shape[0]
    # far-away radius-0 filler (never overlaps) lifts n past the symmetric kernel's threshold
    m = 6000
    g = np.arange(m)
    fill = np.zeros((m, 8), np.float32)
    fill[:, 0] = 30000.0 + 10.0 * (g % 80)
    fill[:, 1] = 30000.0 + 10.0 * (g // 80)
    fill[:, 2], fill[:, 3], fill[:, 6] = 1.5, -2.25, 1e-20
    flat = np.concatenate([ic, fill])
    with nb.Simulation(bodies_of(flat), eps=1.0, collide=True, symmetry=symmetry, device=0) as sim:
        assert ("symmetric=1" in sim.describe()) == symmetry
        for steps in (1, 3):
            sim.advance(steps - sim.frame, 1.0 / 64.0)
            b = sim.sync()
            gold = np.load(GOLD / f"collide_isolated_s{steps}.npy")
            st = {k: gold[:, i] for i, k in enumerate(("x", "y", "vx", "vy"))}
            assert_state(b, st, f"step {steps}", rows=slice(0, npair))
        assert stats(sim)["pairs_total"] > 256


# ---------------------------------------------------------------------------------------------------------------------
# 2 / 3. dense cases against the restatement, and the broad phase against a brute-force count
# ---------------------------------------------------------------------------------------------------------------------
def clumps(n: int, seed: int, mass: float = 1e-3) -> np.ndarray:
    rng = np.random.default_rng(seed)
    k = max(1, n // 64)
    centre = rng.uniform(-400, 400, (k, 2))
    which = rng.integers(0, k, n)
    flat = np.zeros((n, 8), np.float32)
    flat[:, 0:2] = centre[which] + rng.normal(0, 6.0, (n, 2))
    flat[:, 2:4] = rng.normal(0, 5.0, (n, 2))
    flat[:, 6] = mass * rng.uniform(0.5, 2.0, n)
    flat[:, 7] = rng.uniform(0.2, 1.0, n)
    return flat


def big_body(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    flat = clumps(n, seed)
    flat[:, 0:2] += 2000.0                                              # the clumps away from the big body
    flat[0, :] = [0, 0, 0.5, -0.5, 0, 0, 1.0, 100.0]
    inside = rng.uniform(0, 2 * np.pi, 300)
    rad = rng.uniform(0, 99.0, 300)
    flat[1:301, 0], flat[1:301, 1] = rad * np.cos(inside), rad * np.sin(inside)
    return flat


def chain(n: int) -> np.ndarray:
    flat = np.zeros((n, 8), np.float32)
    flat[:, 0] = 1.9 * np.arange(n)
    flat[:, 2] = np.where(np.arange(n) % 2, -1.0, 1.0)
    flat[:, 3] = 0.25
    flat[:, 6], flat[:, 7] = 1e-3, 1.0
    return flat


CASES = {"clumps": lambda: clumps(4096, 1), "big_body": lambda: big_body(4096, 2), "chain": lambda: chain(200)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_dense_cases_equal_the_restatement_fp32(case):
    """Handle A (no collisions) and B (collisions) start from the same state; each step B's state goes into A, A steps, the
    CPU resolves A's drifted state, B steps, and the two must agree bit for bit.  |P| is checked against a brute force."""
    flat = CASES[case]()
    b0 = bodies_of(flat)
    with nb.Simulation(b0, eps=1.0, device=0) as A, nb.Simulation(b0, eps=1.0, collide=True, device=0) as B:
        total, most_rounds = 0, 0
        for step in range(4):
            A.upload(B.sync().copy())
            A.advance(1, 0.01)
            st = cm.state_from_bodies(A.sync())
            P = cm.pairs(st["x"], st["y"], st["r"])
            rounds = cm.resolve_rounds(st, P)
            B.advance(1, 0.01)
            b = B.sync()
            assert_state(b, st, f"{case} step {step}")
            s = stats(B)
            assert s["pairs_last_step"] == len(P) and s["rounds_last_step"] == rounds, (s, len(P), rounds)
            total += len(P)
            most_rounds = max(most_rounds, rounds)
        assert total > 0 and stats(B)["pairs_total"] == total
        if case == "chain":
            assert most_rounds >= 150                           # one round per link
        assert describe_resolve(B) in ("lds", "none")
        if case == "big_body":
            assert "large=1" in B.describe()


def _hip():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
        try:
            lib = C.CDLL(name)
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return lib
        except OSError:
            continue
    raise RuntimeError("HIP runtime library not found")


def device_positions_f64(sim) -> np.ndarray:
    sim.wait()
    out = np.empty((sim.n, 2), np.float64)
    assert _hip().hipMemcpy(out.ctypes.data, sim.pos_buffer(L.NB_POS_CURRENT), out.nbytes, 2) == 0
    return out


@pytest.mark.parametrize("n,expect", [(4096, "lds"), (16384, "global")])
def test_dense_clumps_equal_the_restatement_fp64(n, expect):
    """fp64: from a float-representable state with negligible gravity (masses 1e-30) and dt = 1/64 the drift is exact, so
    the CPU knows the drifted fp64 state; positions are compared in full fp64 bits, velocities through nb_sync's floats.
    16 384 dense bodies are more than the LDS holds: the resolution runs on global memory."""
    flat = clumps(n, 3, mass=1e-30)
    flat[:, 7] *= 1.5
    with nb.Simulation(bodies_of(flat), eps=1.0, precision="fp64", collide=True, device=0) as B:
        for step in range(2):
            b = B.sync().copy()
            B.upload(b)
            st = cm.state_from_bodies(b, np.float64)
            cm.drift(st, 1.0 / 64.0)
            P = cm.pairs(st["x"], st["y"], st["r"])
            cm.resolve_rounds(st, P)
            B.advance(1, 1.0 / 64.0)
            pos = device_positions_f64(B)
            assert np.array_equal(pos[:, 0].view(np.uint64), st["x"].view(np.uint64)), f"fp64 x, step {step}"
            assert np.array_equal(pos[:, 1].view(np.uint64), st["y"].view(np.uint64)), f"fp64 y, step {step}"
            assert_state(B.sync(), st, f"fp64 step {step}")
            assert stats(B)["pairs_last_step"] == len(P) > 0
            assert describe_resolve(B) == expect


# ---------------------------------------------------------------------------------------------------------------------
# 4. the reference's own start
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_start_until_contact_then_against_the_restatement():
    ics = nb.default_ics(25000)
    st0 = cm.state_from_bodies(ics)
    assert len(cm.pairs(st0["x"], st0["y"], st0["r"])) == 0             # no disc overlaps another at the start
    with nb.Simulation(ics, eps=1.0, extras=3, collide=True, device=0) as B, nb.Simulation(ics, eps=1.0, extras=3, device=0) as A:
        steps = 0
        while stats(B)["pairs_total"] == 0 and steps < 2000:
            B.advance(1, 0.01)
            steps += 1
        first = stats(B)["pairs_total"]
        print(f"\nreference start: first contact in step {steps} ({first} pairs)")
        assert first > 0, "no contact within 2000 steps"
        checked = 0
        for _ in range(40):
            A.upload(B.sync().copy())
            A.advance(1, 0.01)
            st = cm.state_from_bodies(A.sync())
            P = cm.pairs(st["x"], st["y"], st["r"])
            cm.resolve_rounds(st, P)
            B.advance(1, 0.01)
            assert_state(B.sync(), st, f"reference start, step {B.frame}")
            assert stats(B)["pairs_last_step"] == len(P)
            if len(P):
                # collisions exchange momentum only: the total changes by the rounding of the touched bodies' m v
                (pa, qa, _), _ = A.momentum()
                (pb, qb, _), _ = B.momentum()
                touched = np.unique(P.ravel())
                scale = float(np.sum(st["m"][touched].astype(np.float64) * np.hypot(st["vx"][touched], st["vy"][touched])))
                assert abs(pb - pa) <= 1e-6 * scale and abs(qb - qa) <= 1e-6 * scale, (pa, pb, qa, qb, scale)
                checked += 1
            if checked >= 5:
                break
        assert checked >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. capacity overflow, restart from a dump
# ---------------------------------------------------------------------------------------------------------------------
def test_overflow_reports_enomem_once_and_recovers(tmp_path):
    flat = clumps(4096, 4)
    b0 = bodies_of(flat)
    with nb.Simulation(b0, eps=1.0, collide=True, device=0) as B, nb.Simulation(b0, eps=1.0, device=0) as A:
        B.collide_capacity(4)
        B.advance(1, 0.01)
        with pytest.raises(nb.NBodyError) as e:
            B.wait()
        assert e.value.code == L.NB_ENOMEM and "frame 1" in str(e.value) and "capacity of 4" in str(e.value)
        B.wait()                                                         # reported once
        s = stats(B)
        assert s["overflow_steps"] == 1 and s["pairs_total"] == 0 and s["pairs_last_step"] > 4
        A.advance(1, 0.01)
        assert_state(B.sync(), cm.state_from_bodies(A.sync()), "over capacity: nothing resolved")
        B.collide_capacity(1 << 20)
        A.upload(B.sync().copy())
        A.advance(1, 0.01)
        st = cm.state_from_bodies(A.sync())
        cm.collide(st)
        B.advance(1, 0.01)
        assert_state(B.sync(), st, "after raising the capacity")
        # dump mid-run and restart: the dump carries extras, so collisions stay on, and the runs continue bit-identically
        path = tmp_path / "mid.nbd"
        B.dump(path)
        bodies, frame, p = nb.read_bodies(path)
        assert frame == 2 and p.extras & L.NB_EXTRA_COLLIDE
        with nb.Simulation(bodies, eps=p.eps, extras=p.extras, first_frame=frame, device=0) as R:
            assert "collide=1" in R.describe()
            B.advance(3, 0.01)
            R.advance(3, 0.01)
            rb, bb = R.sync(), B.sync()
            assert rb.tobytes() == bb.tobytes() and R.frame == B.frame == 5
            assert stats(R)["pairs_last_step"] == stats(B)["pairs_last_step"] > 0
