"""GPU: the body order of the whole-system symmetric kernel (NB_FLAG_BODY_ORDER, nbodysim_amd/csrc/nb_order.hip.h).

The order is forced on at small sizes (``body_order=True`` also lifts the lower size limit of the symmetric scheme), around the
plan's units: tiles of 512 (the automatic choice below 49 152 bodies) or 2 048 particles, chunks of 64.  What is checked:

* exact plumbing on the integer lattice of tests/lattice_model.py, where every partial sum is exact: with the order on every body
  receives its own row whatever the permutation, to the bit, and so does the unordered handle;
* the fp64 oracle to the bars of test_config2_lds_tiled_kernel_at_65536_vs_fp64_direct (1e-5, 1e-5, 2e-5 of max |a|), on against
  off to 2e-6 of max |a|; masses travel with their bodies;
* the re-sort cadence counts force evaluations, not nb_step calls; two handles agree bit for bit; perm is a permutation;
* degenerate boxes; a re-upload; the exact scaling laws; the KDK integrator and the collision pass.

Every case is a few thousand bodies; the oracle runs once per module.  One process; after a HIP error nothing more is started.
"""
import numpy as np
import pytest

import lattice_model as lm
from conftest import max_rel

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

pytestmark = pytest.mark.gpu

EPS, DT = 0.02, 1e-3
LDT = 2.0 ** -10
_HIP_ERROR = []


class _watch:
    """Remember a HIP error raised inside the block so that no later test touches the GPU."""

    def __enter__(self):
        if _HIP_ERROR:
            pytest.fail(f"not run: an earlier test of this module met a HIP error ({_HIP_ERROR[0]})")
        return self

    def __exit__(self, et, ev, tb):
        if et is not None and issubclass(et, nb.NBodyError) and getattr(ev, "code", 0) == L.NB_EHIP:
            _HIP_ERROR.append(str(ev))
        return False


def f32(x):
    return float(np.float32(x))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b, fields=("pos", "vel", "acc")):
    return all(np.array_equal(bits(a[f]), bits(b[f])) for f in fields)


def ordered(sim, every=16):
    d = sim.describe()
    assert "symmetric=1" in d and f" order=morton/{every} " in d, d
    return d


def unordered(sim):
    d = sim.describe()
    assert " order=0 " in d, d
    return d


# --------------------------------------------------------------------------------------------------- exact plumbing ---
@pytest.mark.parametrize("n", [2048 + 64 + 3, 3 * 2048])
@pytest.mark.parametrize("masses", [lm.UNIFORM, lm.MIXED], ids=["equal", "individual"])
@pytest.mark.parametrize("tile", [0, 2048], ids=["tile512", "tile2048"])
def test_lattice_accelerations_are_exact_with_the_order_on_and_off(n, masses, tile):
    """Lattice bodies in random index order: on and off carry the bits of the int64 closed form, so every body got its own row."""
    K = lm.pick_K(n, max(masses))
    for seed in lm.seeds_for(K, 2):
        b, k, m = lm.lattice_bodies(n, K, masses, seed)
        want = lm.exact_acc(k, m)
        with _watch():
            with nb.Simulation(b, eps=1.0, body_order=True, sym_tile=tile) as on:
                d = ordered(on)
                assert f"tile={tile or 512} " in d and f"uniform_mass={int(len(masses) == 1)}" in d, d
                a_on = on.accelerations()
                on.advance(1, LDT)                      # the fused gather: v = 0 + a dt through perm, dt a power of two
                one = on.sync()
            with nb.Simulation(b, eps=1.0, body_order=False) as off:
                unordered(off)
                a_off = off.accelerations()
        bad = np.argwhere((bits(a_on) != bits(want)).any(axis=1)).ravel()
        assert bad.size == 0, (f"{bad.size} bodies differ from the lattice sum with the order on; first {bad[:8].tolist()}: got "
                               f"{(a_on[bad[0]] / 2.0 ** lm.UNIT_F32).tolist()} want {(want[bad[0]] / 2.0 ** lm.UNIT_F32).tolist()} lattice units\n{d}")
        assert np.array_equal(bits(a_off), bits(want)) and np.array_equal(bits(a_on), bits(a_off))
        assert np.array_equal(bits(one["acc"]), bits(want)) and np.array_equal(bits(one["vel"]), bits(want * np.float32(LDT)))


# ------------------------------------------------------------------------------------------------------- the oracle ---
@pytest.fixture(scope="module")
def plummer():
    return nb.plummer_2d(4099, 3)


@pytest.fixture(scope="module")
def plummer_oracle(plummer, nbo):
    d = nbo.step_f64(nbo.state_from_bodies(plummer, np.float64), f32(EPS), f32(DT), 3)
    return np.stack([d["x"], d["y"]], 1), np.stack([d["vx"], d["vy"]], 1), np.stack([d["ax"], d["ay"]], 1)


def assert_bars(got, ref, what):
    pos64, vel64, acc64 = ref
    ep, ev = max_rel(got["pos"], pos64), max_rel(got["vel"], vel64)
    ea = np.max(np.abs(got["acc"].astype(np.float64) - acc64)) / np.max(np.abs(acc64))
    print(f"{what}: pos {ep:.2e} vel {ev:.2e} (bar 1e-5), acc {ea:.2e} of max |a| (bar 2e-5)")
    assert ep < 1e-5 and ev < 1e-5 and ea < 2e-5, (what, ep, ev, ea)


def test_three_steps_against_the_fp64_oracle_and_on_against_off(plummer, plummer_oracle):
    with _watch():
        with nb.Simulation(plummer, eps=EPS, body_order=True) as on:
            ordered(on)
            on.advance(3, DT)
            got = on.sync().copy()
        with nb.Simulation(plummer, eps=EPS, body_order=False) as off:
            unordered(off)
            off.advance(3, DT)
            ref = off.sync().copy()
    assert_bars(got, plummer_oracle, "order on")
    scale = np.max(np.abs(plummer_oracle[2]))
    d = np.max(np.abs(got["acc"].astype(np.float64) - ref["acc"])) / scale
    print(f"on against off: acc {d:.2e} of max |a| (bar 2e-6)")
    assert d < 2e-6, d


@pytest.mark.parametrize("mass_scaling", [False, True], ids=["general", "folded"])
def test_masses_travel_with_their_bodies(nbo, mass_scaling):
    """One body of 5 000 at 1 000 x the mass of the rest: a mass that stayed behind at its index would pull from the wrong place."""
    ic = nb.plummer_2d(5000, 11)
    ic["mass"][1234] *= np.float32(1000.0)
    d = nbo.step_f64(nbo.state_from_bodies(ic, np.float64), f32(EPS), f32(DT), 3)
    ref = np.stack([d["x"], d["y"]], 1), np.stack([d["vx"], d["vy"]], 1), np.stack([d["ax"], d["ay"]], 1)
    with _watch():
        with nb.Simulation(ic, eps=EPS, body_order=True, uniform_mass=False, mass_scaling=mass_scaling) as sim:
            desc = ordered(sim)
            assert f"uniform_mass=0 mass_scaled={int(mass_scaling)}" in desc, desc
            sim.advance(3, DT)
            got = sim.sync().copy()
    assert_bars(got, ref, f"one heavy body, mass_scaling={mass_scaling}")


# ---------------------------------------------------------------------------------------------------------- cadence ---
def test_the_cadence_counts_force_evaluations_and_perm_is_a_permutation(plummer):
    n = plummer.shape[0]

    def run(*calls):
        with nb.Simulation(plummer, eps=EPS, body_order=True) as sim:
            assert sim.body_order(every=2) == 2
            ordered(sim, 2)
            first = sim.body_order(perm=True)[1].copy()
            for k in calls:
                sim.advance(k, 0.05)                       # a long step: the bodies cross patches, the sorts differ
            out = sim.sync().copy()
            return out, first, sim.body_order(perm=True)[1].copy()
    with _watch():
        a, first, perm_a = run(1, 4)
        b, _, perm_b = run(5)
        c, _, _ = run(5)
    assert same(a, b), "advance(1) + advance(4) and advance(5) differ: the cadence is counted per call"
    assert same(b, c), "two fresh handles differ"
    for p in (first, perm_a, perm_b):
        assert np.array_equal(np.sort(p), np.arange(n, dtype=np.uint32))
    assert np.array_equal(perm_a, perm_b) and not np.array_equal(first, perm_a)      # it was sorted again on the way


def test_an_unordered_handle_has_no_order_to_read(plummer):
    with _watch():
        with nb.Simulation(plummer, eps=EPS) as sim:           # below the size rule: the caller's order
            unordered(sim)
            assert sim.body_order() == 0
            with pytest.raises(nb.NBodyError):
                sim.body_order(every=4)
        with nb.Simulation(plummer, eps=EPS, body_order=True, order="sequential", rsqrt="quake") as sim:
            unordered(sim)                                     # the parity mode keeps the caller's order whatever the bit


# ------------------------------------------------------------------------------------------------------- degenerate ---
def _lattice_record(k, m=None):
    b = nb.bodies_array(k.shape[0])
    b["pos"] = np.ldexp(k.astype(np.float64), lm.UNIT_F32).astype(np.float32)
    b["mass"] = 1.0 if m is None else m
    return b


DEGENERATE = {
    "coincident": lambda: np.tile(np.array([[37, 211]], np.int64), (300, 1)),
    "vertical-line": lambda: np.stack([np.full(300, 99, np.int64), np.random.default_rng(5).permutation(512)[:300]], 1),
    "n1": lambda: np.array([[5, 7]], np.int64),
    "n63": lambda: np.random.default_rng(6).integers(0, 512, (63, 2)),
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_boxes_give_the_unordered_bits(name):
    """Lattice sites, so that the sums are exact and `the unordered handle's bits` is a fair demand of another kernel."""
    k = DEGENERATE[name]()
    b = _lattice_record(k)
    with _watch():
        with nb.Simulation(b, eps=1.0, body_order=True) as on:
            ordered(on)
            a_on = on.accelerations()
            perm = on.body_order(perm=True)[1]
            on.advance(1, LDT)                          # one step: the drifted bodies leave the lattice, a second step is not exact
            one_on = on.sync().copy()
        with nb.Simulation(b, eps=1.0, body_order=False) as off:
            a_off = off.accelerations()
            off.advance(1, LDT)
            one_off = off.sync().copy()
    assert np.isfinite(a_on).all() and all(np.isfinite(one_on[f]).all() for f in ("pos", "vel", "acc"))
    assert np.array_equal(bits(a_on), bits(a_off)) and np.array_equal(bits(a_on), bits(lm.exact_acc(k, np.ones(len(k), np.int64))))
    assert same(one_on, one_off)
    assert np.array_equal(np.sort(perm), np.arange(len(k), dtype=np.uint32))
    if name == "coincident":
        assert np.array_equal(perm, np.arange(len(k), dtype=np.uint32))      # ties go by index: the identity
    if name == "vertical-line":
        assert np.array_equal(perm, np.argsort(k[:, 1], kind="stable").astype(np.uint32))   # x keys are all 0: the order of y


# ---------------------------------------------------------------------------------------------------------- refresh ---
def test_upload_mid_run_starts_the_order_over(plummer):
    moved = nb.plummer_2d(plummer.shape[0], 8)
    with _watch():
        with nb.Simulation(plummer, eps=EPS, body_order=True) as sim:
            sim.body_order(every=2)
            sim.advance(3, DT)                                 # mid-cycle: without the reset the next evaluation would not sort
            sim.upload(moved)
            sim.advance(1, DT)
            got = sim.sync().copy()
        with nb.Simulation(moved, eps=EPS, body_order=True) as fresh:
            fresh.body_order(every=2)
            fresh.advance(1, DT)
            want = fresh.sync().copy()
    assert same(got, want)


# ------------------------------------------------------------------------------------------------------ scaling law ---
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_exact_scaling_laws_hold_with_the_order_on(precision):
    """The identities of test_exact_scaling_laws_hold_bit_for_bit_at_full_size at 4 099 bodies: the keys are covariant under a
    power-of-two scaling of the coordinates, so the order, and with it every bit, is the same."""
    ic = nb.plummer_2d(4099, 7)
    ic["mass"] = np.float32(1.0 / 4096)

    def acc_of(b, eps, **kw):
        with nb.Simulation(b, eps=eps, precision=precision, body_order=True, **kw) as sim:
            ordered(sim)
            return sim.accelerations().copy(), sim.body_order(perm=True)[1].copy()
    with _watch():
        for kw in (dict(), dict(uniform_mass=False, mass_scaling=False)):
            a1, p1 = acc_of(ic, EPS, **kw)
            assert np.isfinite(a1).all()
            heavy = ic.copy()
            heavy["mass"] *= np.float32(2.0)
            a2, p2 = acc_of(heavy, EPS, **kw)
            assert np.array_equal(p1, p2) and np.array_equal(bits(a1 * np.float32(2.0)), bits(a2)), ("mass x 2", kw)
            wide = ic.copy()
            wide["pos"] *= np.float32(2.0)
            a3, p3 = acc_of(wide, 2.0 * EPS, **kw)
            assert np.array_equal(p1, p3) and np.array_equal(bits(a1 * np.float32(0.25)), bits(a3)), ("length x 2", kw)


# -------------------------------------------------------------------------------------------------- KDK and collide ---
def test_kdk_with_the_order_on_follows_the_unordered_handle(plummer):
    out = {}
    with _watch():
        for on in (True, False):
            with nb.Simulation(plummer, eps=EPS, integrator="kdk", body_order=on) as sim:
                (ordered if on else unordered)(sim)
                sim.advance(3, DT)
                out[on] = sim.sync().copy()
    scale = np.max(np.abs(out[False]["acc"]))
    ep = max_rel(out[True]["pos"], out[False]["pos"].astype(np.float64))
    ea = np.max(np.abs(out[True]["acc"].astype(np.float64) - out[False]["acc"])) / scale
    print(f"KDK on against off: pos {ep:.2e}, acc {ea:.2e} of max |a| (bar 2e-6)")
    assert ep < 2e-6 and ea < 2e-6, (ep, ea)


def test_collisions_with_the_order_on_resolve_the_same_pairs(plummer):
    ic = plummer.copy()
    ic["radius"] = np.float32(0.01)
    out, stats = {}, {}
    with _watch():
        for on in (True, False):
            with nb.Simulation(ic, eps=EPS, collide=True, body_order=on) as sim:
                (ordered if on else unordered)(sim)
                sim.advance(2, DT)
                out[on] = sim.sync().copy()
                stats[on] = sim.collision_stats()
    assert stats[True]["pairs_total"] == stats[False]["pairs_total"] > 0, stats
    assert stats[True]["overflow_steps"] == 0 and np.isfinite(out[True]["pos"]).all()
    print(f"collide on against off: {stats[True]['pairs_total']} pairs, pos {max_rel(out[True]['pos'], out[False]['pos'].astype(np.float64)):.2e}")
