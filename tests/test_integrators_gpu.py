"""GPU: the composed integrators NB_INTEGRATOR_DKD and NB_INTEGRATOR_FR4 (include/nbody.h) on every unsharded path.

* DKD bit for bit by a twin handle: with h = 2^-7 the products v h and a h are exact, so a DKD step is, to the bit, a host drift by
  h/2, one kick-drift step of the twin, and a host drift back by h/2.
* FR4 bit for bit in the strict modes: a float32 replay with one rounding per operation, every stage's acceleration taken from the twin.
* Both against the fp64 model (tests/integrators_model.py) with the oracle's accelerations, inside the bars of the existing KDK tests.
* Reversal on the fp64 handle; nb_step(1) + nb_step(3) = nb_step(4); dump and restart; frames; profiled launches; the body order;
  failed tree builds.

About a thousand bodies everywhere (1000 is no multiple of 64 or 256: the drift's tail), one process; after a HIP error nothing more is
started.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import max_rel

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import integrators_model as im  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
EPS = 0.05
H2 = 2.0 ** -7                   # the twin's step: a power of two
HF = 2e-3
N = 1000
_HIP_ERROR = []


@pytest.fixture(autouse=True)
def _stop_after_a_hip_error():
    """Remember a HIP error so that no later test of this module touches the GPU."""
    if _HIP_ERROR:
        pytest.fail(f"not run: an earlier test of this module met a HIP error ({_HIP_ERROR[0]})")


class watched:
    """Remember a HIP error raised inside the block."""

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is not None and issubclass(et, nb.NBodyError) and getattr(ev, "code", 0) == L.NB_EHIP:
            _HIP_ERROR.append(str(ev))
        return False


def f32(x):
    return float(np.float32(x))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    bad = np.argwhere(bits(a) != bits(b))
    assert bad.size == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def up(sim, b):
    sim.upload(np.ascontiguousarray(b).view(L.BODY_DTYPE))


def bodies_of(flat):
    b = nb.bodies_array(flat.shape[0])
    b["pos"], b["vel"], b["acc"] = flat[:, 0:2], flat[:, 2:4], flat[:, 4:6]
    b["mass"], b["radius"] = flat[:, 6], flat[:, 7]
    return b


@functools.lru_cache(maxsize=None)
def plummer2(n=N):
    return nb.plummer_2d(n, 5)


@functools.lru_cache(maxsize=None)
def plummer3():
    return nb.plummer_3d(N, 5).view(nb.BODY3_DTYPE)


@functools.lru_cache(maxsize=None)
def fixture1024():
    return bodies_of(np.load(GOLD / "ic_plummer_1024.npy"))


@functools.lru_cache(maxsize=None)
def far_out():
    """The far-out, fast bodies of test_extras_clamp_and_boundary_vs_oracle: beyond the soft boundary, near the velocity clamp."""
    n = 512
    rng = np.random.default_rng(2)
    b = nb.bodies_array(n)
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = rng.uniform(6e4, 1.3e5, n)
    b["pos"] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(np.float32)
    b["vel"] = (rng.normal(size=(n, 2)) * 900).astype(np.float32)
    b["mass"] = rng.uniform(1, 100, n).astype(np.float32)
    return b


TREE = dict(force="tree", theta=0.5, tree_leaves=True)
# name -> (bodies, Simulation keywords, what nb_describe must say)
HANDLES = {
    "symmetric-ordered": (plummer2, dict(eps=EPS, body_order=True), "symmetric=1"),
    "symmetric": (lambda: plummer2(5693), dict(eps=EPS, body_order=False), "symmetric=1"),
    "one-sided": (plummer2, dict(eps=EPS, symmetry=False), "symmetric=0"),
    "sequential-quake": (plummer2, dict(eps=EPS, order="sequential", rsqrt="quake"), "sum=sequential"),
    "sequential-exact": (plummer2, dict(eps=EPS, order="sequential"), "sum=sequential"),
    "fp64": (plummer2, dict(eps=EPS, precision="fp64"), "fp64"),
    "3d": (plummer3, dict(eps=EPS, dims=3), "3-D"),
    "tree-leaves": (fixture1024, dict(eps=EPS, **TREE), "walk=group"),
    "tree-quad-rel": (fixture1024, dict(eps=EPS, tree_quadrupole=True, tree_alpha=0.005, **TREE), "quad=1"),
    "tree-quake-leaves-rel": (fixture1024, dict(eps=EPS, rsqrt="quake", tree_alpha=0.005, **TREE), "walk=lane"),
    "tree-reference-quake": (fixture1024, dict(eps=EPS, force="tree", rsqrt="quake"), "force=tree"),
    "extras": (far_out, dict(eps=1.0, extras=3), "symmetric=0"),
}


def open_pair(name, integrator):
    """(A with `integrator`, B the same handle with kick-drift, the bodies)."""
    make, kw, says = HANDLES[name]
    ic = make()
    a = nb.Simulation(ic, integrator=integrator, **kw)
    b = nb.Simulation(ic, **kw)
    da, db = a.describe(), b.describe()
    assert says in da and says in db, (da, db)
    assert da.endswith(f" integrator={integrator}") and da[: -len(f" integrator={integrator}")] == db, (da, db)
    if "order=morton" in da:                   # the twin sorts at every upload: so must A, at every evaluation
        assert a.body_order(every=1) == 1 and b.body_order(every=1) == 1
    return a, b, ic


# ----------------------------------------------------------------------------------------------------- DKD by a twin ---
@pytest.mark.parametrize("name", ["symmetric-ordered", "symmetric", "one-sided", "sequential-quake", "fp64", "3d", "tree-leaves",
                                  "tree-quad-rel", "tree-reference-quake", "extras"])
def test_dkd_is_a_host_drift_a_kick_drift_step_and_a_host_drift_bit_for_bit(name):
    """Three consecutive steps.  fp32 handles: bits(A.vel) == bits(B.vel), bits(A.acc) == bits(B.acc), bits(A.pos) == bits(xm + B.vel h/2).

    The fp64 handle's state reaches the host, and the twin, as float records only.  So that the same identity can be held to the bit
    there, each of its steps starts from A's state put on a 2^-8 grid and uploaded into A as well: x, v and xm = x + v h/2 are then
    floats exactly, and velocities and accelerations (one double, rounded to float on both sides) must agree in every bit.  A.pos is
    the float nearest to xm + v' h/2, of which the host has v' rounded to float: the bar is half a float ulp of the position for the
    one rounding, 2^-25 |v'| h/2 for the other, and the host's own double rounding."""
    fp64 = name == "fp64"
    real = np.float64 if fp64 else np.float32
    h2 = real(H2 / 2)
    with watched():
        a, b, _ = open_pair(name, "dkd")
        with a, b:
            for step in range(3):
                s = a.sync().copy()
                if fp64:
                    s["pos"], s["vel"] = np.round(s["pos"] * 256.0) / 256.0, np.round(s["vel"] * 256.0) / 256.0
                    up(a, s)
                x, v = s["pos"].astype(real), s["vel"].astype(real)
                xm = x + v * h2
                assert np.array_equal((v * h2) / h2, v) and np.array_equal(xm.astype(np.float32).astype(real), xm)
                t = s.copy()
                t["pos"] = xm
                up(b, t)
                b.advance(1, H2)
                a.advance(1, H2)
                ga, gb = a.sync().copy(), b.sync().copy()
                assert a.frame == step + 1
                same_bits(ga["vel"], gb["vel"], f"{name} step {step}: vel")
                same_bits(ga["acc"], gb["acc"], f"{name} step {step}: acc")
                assert not np.array_equal(ga["vel"], s["vel"])
                want = xm + gb["vel"].astype(real) * h2
                if fp64:
                    off = np.abs(ga["pos"].astype(np.float64) - want)
                    bar = (0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2.0 ** -25 * np.abs(gb["vel"]) * h2
                           + 2.0 ** -52 * np.abs(want))
                    print(f"fp64 step {step}: {np.count_nonzero(ga['pos'] == want.astype(np.float32))} of {want.size} positions equal, "
                          f"largest distance {np.max(off / bar):.3f} of the bar")
                    assert (off <= bar).all()
                else:
                    same_bits(ga["pos"], want, f"{name} step {step}: pos")


# ------------------------------------------------------------------------------------------- FR4 in the strict modes ---
@pytest.mark.parametrize("name", ["sequential-quake", "sequential-exact", "tree-quake-leaves-rel"])
@pytest.mark.parametrize("integrator", ["fr4", "dkd"])
def test_strict_handles_equal_the_float32_replay_bit_for_bit(name, integrator):
    """h = 2e-3, two steps: every product and sum of the leading drift, the kicks and the drifts rounded to float32 on its own; the
    acceleration of every stage is the twin's at the replayed positions (with the previous evaluation as the tree's a_prev)."""
    with watched():
        a, b, ic = open_pair(name, integrator)
        with a, b:
            s = a.sync().copy()
            x, v, acc = s["pos"].copy(), s["vel"].copy(), s["acc"].copy()
            for step in range(2):
                def accel(q):
                    t = s.copy()
                    t["pos"], t["vel"], t["acc"] = q, v, acc
                    up(b, t)
                    acc[...] = b.accelerations()
                    return acc.copy()
                x, v, _ = im.step(x, v, accel, HF, integrator, np.float32, strict=True)
                a.advance(1, HF)
                g = a.sync().copy()
                same_bits(g["acc"], acc, f"{name} {integrator} step {step}: acc")
                same_bits(g["vel"], v, f"{name} {integrator} step {step}: vel")
                same_bits(g["pos"], x, f"{name} {integrator} step {step}: pos")


# ------------------------------------------------------------------------------------------------- the fp64 model ---
@functools.lru_cache(maxsize=None)
def model(integrator, dims, steps=5):
    import nbo
    h, eps = f32(HF), f32(EPS)
    if dims == 3:
        st = nbo.state3_from_bodies(plummer3())
        keys = ("x", "y", "z")
    else:
        st = nbo.state_from_bodies(plummer2(), np.float64)
        keys = ("x", "y")
    x = np.stack([st[k] for k in keys], 1)
    v = np.stack([st["v" + k] for k in keys], 1)

    def accel(q):
        for c, k in enumerate(keys):
            st[k] = np.ascontiguousarray(q[:, c])
        return np.stack([np.array(a) for a in (nbo.accel3_f64(st, eps) if dims == 3 else nbo.accel_f64(st, eps))], 1)
    for _ in range(steps):
        x, v, _a = im.step(x, v, accel, h, integrator, np.float64)
    return x, v


@pytest.mark.parametrize("integrator", ["dkd", "fr4"])
@pytest.mark.parametrize("name,bar_pos,bar_vel", [("fp64", 2e-7, 2e-6), ("3d", 1e-5, 1e-5), ("one-sided", 1e-5, 1e-5),
                                                  ("symmetric-ordered", 1e-5, 1e-5)])
def test_five_steps_against_the_fp64_model(nbo, name, integrator, bar_pos, bar_vel):
    """Bars: test_kdk_integrator_vs_numpy_leapfrog (fp64), test_3d_kdk_integrator_matches_numpy_leapfrog (3-D), the 1e-5 of
    tests/test_headline_gpu.py (fp32 2-D)."""
    make, kw, says = HANDLES[name]
    x, v = model(integrator, 3 if name == "3d" else 2)
    with watched():
        with nb.Simulation(make(), integrator=integrator, **kw) as sim:
            assert says in sim.describe()
            sim.advance(5, f32(HF))
            got = sim.sync()
            assert sim.frame == 5
    ep, ev = max_rel(got["pos"], x), max_rel(got["vel"], v)
    print(f"{name} {integrator}: pos {ep:.2e} (bar {bar_pos:g}), vel {ev:.2e} (bar {bar_vel:g})")
    assert ep < bar_pos and ev < bar_vel, (ep, ev)


def test_reversal_on_the_fp64_handle():
    """8 steps, v -> -v through an upload, 8 steps: DKD and FR4 return to x0 as well as the KDK handle does (at most 4 x its error:
    FR4 does three times the operations).  The turn goes through float records, which is what all of them return to."""
    ic = plummer2()
    back = {}
    with watched():
        for integrator in ("kick_drift", "kdk", "dkd", "fr4"):
            with nb.Simulation(ic, eps=EPS, precision="fp64", integrator=integrator) as sim:
                sim.advance(8, f32(HF))
                s = sim.sync().copy()
                s["vel"] = -s["vel"]
                up(sim, s)
                sim.advance(8, f32(HF))
                back[integrator] = float(np.max(np.abs(sim.sync()["pos"].astype(np.float64) - ic["pos"])))
    print("return error max |x - x0|: " + ", ".join(f"{k} {e:.2e}" for k, e in back.items()))
    assert back["dkd"] <= 4 * back["kdk"] and back["fr4"] <= 4 * back["kdk"], back


# ------------------------------------------------------------------------------------------------------ identities ---
@pytest.mark.parametrize("integrator,launches", [("dkd", 1), ("fr4", 3)])
@pytest.mark.parametrize("name", ["symmetric-ordered", "symmetric", "one-sided", "tree-quad-rel"])
def test_steps_are_self_contained_and_counted(name, integrator, launches):
    """nb_step(1) + nb_step(3) = nb_step(4) in every bit; nb_frame grows by 1 a step; a step is 1 (DKD) or 3 (FR4) profiled force launches."""
    make, kw, _ = HANDLES[name]
    out = []
    with watched():
        for calls in ((1, 3), (4,)):
            with nb.Simulation(make(), integrator=integrator, **kw) as sim:
                sim.profile(True)
                for k in calls:
                    before = sim.frame
                    sim.advance(k, HF)
                    assert sim.frame == before + k
                out.append(sim.sync().copy())
                assert sim.profile_read()[1] == 4 * launches
                with pytest.raises(nb.NBodyError) as e:
                    sim.step_begin(HF)
                assert e.value.code == L.NB_EINVAL and integrator.upper() in str(e.value)
    for f in ("pos", "vel", "acc"):
        same_bits(out[0][f], out[1][f], f"{name} {integrator}: {f} of 1 + 3 steps against 4")


@pytest.mark.parametrize("integrator,value", [("dkd", 2), ("fr4", 3)])
@pytest.mark.parametrize("name", ["one-sided", "tree-quad-rel"])
def test_dump_and_restart_in_mid_run_continue_bit_for_bit(tmp_path, name, integrator, value):
    make, kw, _ = HANDLES[name]
    with watched():
        with nb.Simulation(make(), integrator=integrator, **kw) as sim:
            sim.advance(2, HF)
            sim.dump(tmp_path / "mid.nbd")
            sim.advance(2, HF)
            cont = sim.sync().copy()
        back, frame, p = nb.read_bodies(tmp_path / "mid.nbd")
        assert frame == 2 and p.integrator == value
        with nb.Simulation(back, integrator=integrator, first_frame=frame, **kw) as again:
            again.advance(2, HF)
            got = again.sync().copy()
            assert again.frame == 4
    for f in ("pos", "vel", "acc"):
        same_bits(got[f], cont[f], f"{name} {integrator}: {f} after the restart")


@pytest.mark.parametrize("integrator", ["dkd", "fr4"])
def test_the_ordered_handle_follows_the_unordered_one(integrator):
    """The bar of test_kdk_with_the_order_on_follows_the_unordered_handle, on its bodies."""
    ic = nb.plummer_2d(4099, 3)
    out = {}
    with watched():
        for on in (True, False):
            with nb.Simulation(ic, eps=0.02, integrator=integrator, body_order=on) as sim:
                assert (" order=morton/16 " if on else " order=0 ") in sim.describe(), sim.describe()
                sim.advance(3, 1e-3)
                out[on] = sim.sync().copy()
    scale = np.max(np.abs(out[False]["acc"]))
    ep = max_rel(out[True]["pos"], out[False]["pos"].astype(np.float64))
    ea = np.max(np.abs(out[True]["acc"].astype(np.float64) - out[False]["acc"])) / scale
    print(f"{integrator} on against off: pos {ep:.2e}, acc {ea:.2e} of max |a| (bar 2e-6)")
    assert ep < 2e-6 and ea < 2e-6, (ep, ea)


# ---------------------------------------------------------------------------------------------------- failed builds ---
def close_pairs(n=512, one_ulp=False):
    """test_tree_gpu's close pairs: n / 2 pairs 2^-18 apart on a unit grid need some 40 n nodes, more than the capacity of
    16 n + 4096; one ulp apart, no rounded child centre separates them within the depth cap.  Every body moves with v = (0.5, 0):
    the leading drift shifts them all alike."""
    k = np.arange(n // 2)
    flat = np.zeros((n, 8), np.float32)
    flat[0::2, 0], flat[0::2, 1] = (k % 16) - 7.25, (k // 16) - 7.25
    flat[1::2, 0], flat[1::2, 1] = flat[0::2, 0] + np.float32(2.0 ** -18), flat[0::2, 1]
    if one_ulp:
        flat[1::2, 0] = np.nextafter(flat[0::2, 0], np.float32(99))
    flat[:, 2], flat[:, 6] = 0.5, 1.0 / n
    return bodies_of(flat)


@pytest.mark.parametrize("integrator,stages", [("dkd", 1), ("fr4", 3)])
@pytest.mark.parametrize("kind", ["capacity", "depth"])
def test_a_stage_whose_build_fails_applies_neither_kick_nor_drift(kind, integrator, stages):
    """Node capacity and depth cap, reached as test_capacity_overflow_is_reported_once_and_the_handle_stays_usable and
    test_depth_cap_is_reported reach them: NB_ENOMEM once, the velocities unchanged, the positions moved by the unconditional
    leading drift alone, one failed evaluation per stage.  That the DRIFTED positions still fail is checked on the model first."""
    import tree_model as tm
    ic = close_pairs(one_ulp=kind == "depth")
    lead = im.steps_of(H2, integrator, np.float32)[0]
    drifted = ic["pos"] + (ic["vel"] * lead).astype(np.float32)
    if kind == "depth":
        with pytest.raises(OverflowError):
            tm.build_canonical(drifted[:, 0].copy(), drifted[:, 1].copy(), ic["mass"].copy())
    else:
        assert tm.build_canonical(drifted[:, 0].copy(), drifted[:, 1].copy(), ic["mass"].copy())["px"].shape[0] > 16 * ic.shape[0] + 4096
    with watched():
        with nb.Simulation(ic, eps=EPS, force="tree", rsqrt="quake", integrator=integrator) as sim:
            sim.advance(1, H2)
            with pytest.raises(nb.NBodyError) as e:
                sim.wait()
            assert e.value.code == L.NB_ENOMEM and "frame 0" in str(e.value) and "nothing was integrated" in str(e.value)
            assert ("not separated within 63 levels" if kind == "depth" else "more than the capacity") in str(e.value)
            sim.wait()                                      # reported once
            got = sim.sync().copy()
            assert sim.frame == 1 and sim.tree_stats()["overflow_steps"] == stages
    same_bits(got["vel"], ic["vel"], "vel after the failed step")
    same_bits(got["pos"], drifted, "pos after the failed step")
