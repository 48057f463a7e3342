"""GPU: nb_raster — the bodies binned into a pixel image on the device, against the numpy statement of the contract
(tests/raster_model.py).  Every comparison is exact equality: the planes are integer sums and do not depend on any order."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import raster_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
SENTINEL_C, SENTINEL_M = np.uint32(0xDEADBEEF), np.float32(-77.25)


def bodies_of(x, y, m, z=None) -> np.ndarray:
    b = nb.bodies_array(len(x))
    b["pos"][:, 0], b["pos"][:, 1], b["mass"] = x, y, m
    if z is not None:
        b.view(L.BODY3_DTYPE)["pos"][:, 2] = z
    return b


def direct(bodies, **kw):
    kw.setdefault("eps", 0.5)
    return nb.Simulation(bodies, device=0, **kw)


@functools.lru_cache(maxsize=None)
def fixture():
    """ic_random_333 as (x, y, m), read once and shared; the arrays are not written to."""
    flat = np.load(GOLD / "ic_random_333.npy").astype(np.float32)
    out = tuple(flat[:, c].copy() for c in (0, 1, 6))
    for a in out:
        a.setflags(write=False)
    return out


def fitting_view(x, y, width=17, height=13, zoom=0.9):
    """zoom < 1: everything inside; zoom > 1: bodies cut off."""
    cx, cy = float(np.median(x)), float(np.median(y))
    half = max(float(np.abs(x - np.float32(cx)).max()) / width, float(np.abs(y - np.float32(cy)).max()) / height)
    return dict(width=width, height=height, center=(cx, cy), scale=zoom * 0.5 / half)


def assert_planes(got, x, y, m, view, quantum, what=""):
    """both planes of `got` = sim.raster(..., mass_quantum=quantum) equal the model bit for bit"""
    count, mass = got
    wc, wm = rm.raster(x, y, m, quantum=quantum, **view)
    assert count.dtype == np.uint32 and count.shape == wc.shape and mass.dtype == np.float32 and mass.shape == wm.shape
    bad = np.argwhere(count != wc)
    assert bad.size == 0, f"{what}: {bad.shape[0]} count pixels differ, first {bad[:4].tolist()}: {count[tuple(bad[0])]} vs {wc[tuple(bad[0])]}"
    bad = np.argwhere(mass.view(np.uint32) != wm.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.shape[0]} mass pixels differ, first {bad[:4].tolist()}: {mass[tuple(bad[0])]!r} vs {wm[tuple(bad[0])]!r}"
    return wc, wm


# ---------------------------------------------------------------------------------------------------------------------
# 1. plain view
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoom", [0.9, 1.7])
def test_plain_view(zoom):
    x, y, m = fixture()
    v = fitting_view(x, y, zoom=zoom)
    q = 2.0 ** -12
    with direct(bodies_of(x, y, m)) as sim:
        wc, wm = assert_planes(sim.raster(mass_quantum=q, **v), x, y, m, v, q, f"zoom {zoom}")
        only = sim.raster(**v)
        assert isinstance(only, np.ndarray) and np.array_equal(only, wc)
    inside, _ = rm.pixels(x, y, **v)
    if zoom < 1:
        assert inside.all() and int(wc.sum()) == x.size
    else:
        sx = (x - np.float32(v["center"][0])) * np.float32(v["scale"]) + np.float32(8.5)
        sy = (y - np.float32(v["center"][1])) * np.float32(v["scale"]) + np.float32(6.5)
        assert (sx < 0).any() and (sx >= 17).any() and (sy < 0).any() and (sy >= 13).any()      # cut off on all four sides
        assert 0 < int(wc.sum()) == int(inside.sum()) < x.size
    assert wc.max() > 1 and (wc == 0).any() and wm.max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_edges_are_inclusive_below_and_exclusive_above():
    # scale 1 and centre (4, 3) on an 8 x 6 view: sx = x and sy = y exactly, on integers and halves
    v = dict(width=8, height=6, center=(4.0, 3.0), scale=1.0)
    gx, gy = np.meshgrid(np.arange(-1.0, 9.01, 0.5), np.arange(-1.0, 7.01, 0.5))
    x = np.concatenate([gx.ravel(), [np.nan, 2.0, np.inf, 2.0, -np.inf, 3.5]]).astype(np.float32)
    y = np.concatenate([gy.ravel(), [2.0, np.nan, 2.0, np.inf, 2.0, -np.inf]]).astype(np.float32)
    m = np.full(x.size, 0.25, np.float32)
    with direct(bodies_of(x, y, m)) as sim:
        count, mass = sim.raster(mass_quantum=0.25, **v)
    assert_planes((count, mass), x, y, m, v, 0.25, "lattice")
    # every pixel holds the four lattice points k, k + 0.5 of each axis: the left / top edge is in, the right / bottom edge, -0.5 and
    # the six bodies with a NaN or infinite coordinate are out
    assert np.array_equal(count, np.full((6, 8), 4, np.uint32)) and np.array_equal(mass, np.full((6, 8), 1.0, np.float32))

    def one(px, py):
        with direct(bodies_of([px, 100.0], [py, 100.0], [1.0, 1.0])) as s:
            return s.raster(**v)

    assert one(0.0, 0.0)[0, 0] == 1 and one(7.5, 0.0)[0, 7] == 1 and one(0.0, 5.5)[5, 0] == 1
    for px, py in ((8.0, 2.0), (2.0, 6.0), (-0.5, 2.0), (2.0, -0.5), (np.nan, 2.0), (2.0, np.inf)):
        assert int(one(px, py).sum()) == 0, (px, py)


# ---------------------------------------------------------------------------------------------------------------------
# 3. contention and grouping
# ---------------------------------------------------------------------------------------------------------------------
N_ODD = 4099                 # not a multiple of 64 or 256: 17 batches of 256 bodies, the last one 3 bodies
GROUPINGS = {
    "one pixel": lambda i: np.zeros_like(i),
    "i % 3": lambda i: i % 3,
    "i % 64": lambda i: i % 64,
    "i % 67": lambda i: i % 67,
    "runs of 2": lambda i: ((i + 1) // 2) % 67,      # on odd indices: the runs (63, 64), (255, 256), ... straddle waves and workgroups
    "runs of 65": lambda i: (i // 65) % 67,          # every run straddles a wave boundary, every fourth or so a workgroup boundary
}


@pytest.mark.parametrize("case", list(GROUPINGS))
def test_contention_and_grouping(case):
    i = np.arange(N_ODD)
    pix = GROUPINGS[case](i)
    v = dict(width=67, height=1, center=(33.5, 0.5), scale=1.0)          # sx = x, sy = y: pixel = floor(x)
    x = (pix + 0.5).astype(np.float32)
    y = np.full(N_ODD, 0.5, np.float32)
    q = 2.0 ** -10
    u = 1 + (i * 7919) % 1000                                            # individual masses: whole quanta, exactly
    m = (u * q).astype(np.float32)
    with direct(bodies_of(x, y, m)) as sim:
        count, mass = sim.raster(mass_quantum=q, **v)
    assert_planes((count, mass), x, y, m, v, q, case)
    want_c = np.bincount(pix, minlength=67)
    want_u = np.bincount(pix, weights=u.astype(np.float64), minlength=67)       # < 2^53: exact
    assert np.array_equal(count[0], want_c) and int(count.sum()) == N_ODD
    assert np.array_equal(mass[0], (want_u * q).astype(np.float32))
    if case == "one pixel":
        assert count[0, 0] == N_ODD and mass[0, 0] == np.float32(int(u.sum()) * q)


def test_pixels_that_meet_in_one_slot_of_the_workgroup_table():
    """The 67 pixels above take 67 different slots of the LDS table.  Here every pixel of a 16384 x 1 view whose home slot is one of
    three neighbouring ones (the fullest such triple: about two dozen pixels) is in use, in every wave: each add but three finds its
    slot taken by another pixel and probes on, through slots that are other pixels' homes."""
    home = ((np.arange(16384, dtype=np.uint64) * 2654435761) % 2 ** 32) >> 21       # raster_table_add's hash, 2048 slots
    per_slot = np.bincount(home.astype(np.int64), minlength=2048)
    s0 = int(np.argmax(per_slot[:-2] + per_slot[1:-1] + per_slot[2:]))
    pixels = np.flatnonzero((home >= s0) & (home <= s0 + 2))
    assert pixels.size >= 20 and np.unique(home[pixels]).size <= 3
    i = np.arange(N_ODD)
    pix = pixels[(i * 5) % pixels.size]
    v = dict(width=16384, height=1, center=(8192.0, 0.5), scale=1.0)     # sx = x exactly: pixel = floor(x)
    x, y = (pix + 0.5).astype(np.float32), np.full(N_ODD, 0.5, np.float32)
    q = 2.0 ** -10
    u = 1 + (i * 7919) % 1000
    m = (u * q).astype(np.float32)
    with direct(bodies_of(x, y, m)) as sim:
        count, mass = sim.raster(mass_quantum=q, **v)
    assert_planes((count, mass), x, y, m, v, q, "colliding slots")
    assert np.array_equal(count[0], np.bincount(pix, minlength=16384)) and int(count.sum()) == N_ODD
    assert np.array_equal(mass[0], (np.bincount(pix, weights=u.astype(np.float64), minlength=16384) * q).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 4. mass units
# ---------------------------------------------------------------------------------------------------------------------
def test_mass_units():
    q = np.float32(2.0 ** -13)
    decades = (10.0 ** np.arange(-6, 7)).astype(np.float32)             # twelve decades; 1e6 / q = 2^33 * 0.95: clamps at 2^32 - 1
    special = np.array([0.5 * q, 1.5 * q, 2.5 * q, 0.0, -3.0, np.nan, np.inf, 3.0, 3.0, np.nan], np.float32)
    m = np.concatenate([decades, special])
    pix = np.concatenate([np.arange(13), [13, 14, 15, 16, 17, 18, 19, 20, 20, 20]])
    v = dict(width=32, height=1, center=(16.0, 0.5), scale=1.0)
    x, y = (pix + 0.25).astype(np.float32), np.full(m.size, 0.5, np.float32)
    with direct(bodies_of(x, y, m)) as sim:
        count, mass = sim.raster(mass_quantum=float(q), **v)
    assert_planes((count, mass), x, y, m, v, float(q), "units")
    u = rm.units(m, q)
    assert u[12] == 4294967295 and u[0] == 0 and u[6] == 8192                  # the heaviest clamps, the lightest weighs nothing
    assert mass[0, 12] == np.float32(4294967295.0 * 2.0 ** -13)
    assert u[13:16].tolist() == [0, 2, 2] and mass[0, 13:16].tolist() == [0.0, 2.0 * q, 2.0 * q]      # ties to even
    # zero, negative and NaN masses are counted and weigh nothing; an infinite one clamps
    assert count[0, 16:21].tolist() == [1, 1, 1, 1, 3] and mass[0, 16:19].tolist() == [0.0, 0.0, 0.0]
    assert mass[0, 19] == mass[0, 12] and mass[0, 20] == 6.0
    assert np.array_equal(count[0, :13], np.ones(13, np.uint32)) and int(count.sum()) == m.size


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_permutation_and_a_second_handle_give_the_same_bits():
    x, y, m = fixture()
    v = fitting_view(x, y, zoom=1.7)
    q = 1e-3
    perm = np.random.default_rng(11).permutation(x.size)
    with direct(bodies_of(x, y, m)) as a, direct(bodies_of(x, y, m)) as b, direct(bodies_of(x[perm], y[perm], m[perm])) as c:
        pa, pb, pc = (s.raster(mass_quantum=q, **v) for s in (a, b, c))
    assert_planes(pa, x, y, m, v, q, "first handle")
    for other in (pb, pc):
        assert np.array_equal(pa[0], other[0]) and np.array_equal(pa[1].view(np.uint32), other[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 6. handle kinds
# ---------------------------------------------------------------------------------------------------------------------
def synced(sim):
    b = sim.sync()
    return b["pos"][:, 0].copy(), b["pos"][:, 1].copy(), b["mass"].copy()


def test_fp64_handle_rounds_to_float():
    x, y, m = fixture()
    v, q = fitting_view(x, y, zoom=1.3), 2.0 ** -11
    with direct(bodies_of(x, y, m), precision="fp64") as sim:
        assert_planes(sim.raster(mass_quantum=q, **v), x, y, m, v, q, "fp64 before a step")
        sim.advance(3, 1e-2)
        got = sim.raster(mass_quantum=q, **v)
        sx, sy, sm = synced(sim)                    # the fp64 state rounded to float
        assert not np.array_equal(sx, x)
        assert_planes(got, sx, sy, sm, v, q, "fp64 after three steps")


def test_dims3_handle_is_projected_on_xy():
    ic = nb.plummer_3d(1000, 7)
    b3 = ic.view(L.BODY3_DTYPE)
    x, y, z, m = (np.ascontiguousarray(a) for a in (b3["pos"][:, 0], b3["pos"][:, 1], b3["pos"][:, 2], b3["mass"]))
    assert np.abs(z).max() > 0.5
    v, q = dict(width=19, height=11, center=(0.1, -0.2), scale=3.0), float(m[0]) / 4
    with direct(ic, dims=3, eps=0.05) as sim:
        assert_planes(sim.raster(mass_quantum=q, **v), x, y, m, v, q, "dims = 3")


def test_tree_handle_before_any_step_and_after_three():
    x, y, m = fixture()
    v, q = fitting_view(x, y, zoom=1.3), 2.0 ** -11
    with nb.Simulation(bodies_of(x, y, m), eps=0.5, force="tree", theta=0.5, tree_leaves=True, device=0) as sim:
        assert_planes(sim.raster(mass_quantum=q, **v), x, y, m, v, q, "tree handle before any step")
        assert sim.tree_stats()["nodes"] == 0
        sim.advance(3, 1e-2)
        got = sim.raster(mass_quantum=q, **v)
        stats = sim.tree_stats()
        sx, sy, sm = synced(sim)
        assert not np.array_equal(sx, x)
        assert_planes(got, sx, sy, sm, v, q, "tree handle after three steps")
        sim.raster(**v)
        assert sim.tree_stats() == stats and sim.frame == 3


def test_blocks_of_a_sharded_run_add_up():
    x, y, m = fixture()
    v, q = fitting_view(x, y, zoom=1.3), 2.0 ** -11
    b = bodies_of(x, y, m)
    with direct(b) as whole, direct(b, i_begin=0, i_count=200) as lo, direct(b, i_begin=200, i_count=133) as hi:
        w = whole.raster(mass_quantum=q, **v)
        a, c = lo.raster(mass_quantum=q, **v), hi.raster(mass_quantum=q, **v)
    assert_planes(a, x[:200], y[:200], m[:200], v, q, "block [0, 200)")
    assert_planes(c, x[200:], y[200:], m[200:], v, q, "block [200, 333)")
    assert np.array_equal(a[0] + c[0], w[0]) and int(a[0].sum()) > 0 and int(c[0].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. touches nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["direct", "tree"])
def test_raster_leaves_the_trajectory_alone(kind):
    x, y, m = fixture()
    v, q = fitting_view(x, y, zoom=1.3), 2.0 ** -11
    kw = dict(force="tree", theta=0.5, tree_leaves=True) if kind == "tree" else {}
    b = bodies_of(x, y, m)
    with direct(b, **kw) as plain, direct(b, **kw) as looked:
        plain.advance(4, 1e-2)
        want = plain.sync().copy()
        looked.advance(2, 1e-2)
        looked.raster(mass_quantum=q, **v)
        assert looked.frame == 2
        looked.advance(1, 1e-2)
        got = looked.raster(mass_quantum=q, **v)                  # no wait in between: the positions of the work enqueued so far
        assert looked.frame == 3
        sx, sy, sm = synced(looked)
        assert_planes(got, sx, sy, sm, v, q, f"{kind}: plane taken behind an unfinished step")
        looked.advance(1, 1e-2)
        have = looked.sync()
        assert looked.frame == plain.frame == 4
        for f in ("pos", "vel", "acc", "mass", "radius"):
            assert np.array_equal(have[f].view(np.uint32), want[f].view(np.uint32)), f"{kind}: {f} differs after nb_raster"


# ---------------------------------------------------------------------------------------------------------------------
# 8. regrow
# ---------------------------------------------------------------------------------------------------------------------
def test_views_grow_and_shrink_on_one_handle():
    x, y, m = fixture()
    q = 2.0 ** -11
    with direct(bodies_of(x, y, m)) as sim:
        for w, h in ((8, 8), (300, 200), (8, 8), (301, 200)):
            v = fitting_view(x, y, w, h, zoom=1.2)
            assert_planes(sim.raster(mass_quantum=q, **v), x, y, m, v, q, f"{w} x {h}")
            assert np.array_equal(sim.raster(**v), rm.raster(x, y, m, **v)[0])


# ---------------------------------------------------------------------------------------------------------------------
# 9. destinations
# ---------------------------------------------------------------------------------------------------------------------
class Pinned:
    """A (height, width) array of `dtype` over an nb_host_alloc block."""

    def __init__(self, height, width, dtype):
        self.lib = nb.load()
        self.ptr = self.lib.nb_host_alloc(height * width * 4)
        assert self.ptr
        self.array = np.frombuffer((C.c_uint8 * (height * width * 4)).from_address(self.ptr), dtype=dtype).reshape(height, width)

    def __enter__(self):
        return self.array

    def __exit__(self, *exc):
        self.array = None
        assert self.lib.nb_host_free(self.ptr) == 0


def test_destinations_and_single_planes():
    x, y, m = fixture()
    v, q = fitting_view(x, y, 40, 30, zoom=1.3), 2.0 ** -11
    wc, wm = rm.raster(x, y, m, quantum=q, **v)
    with direct(bodies_of(x, y, m)) as sim, Pinned(30, 40, np.uint32) as pc, Pinned(30, 40, np.float32) as pm:
        pc[:], pm[:] = SENTINEL_C, SENTINEL_M
        hc, hm = np.full((30, 40), SENTINEL_C, np.uint32), np.full((30, 40), SENTINEL_M, np.float32)
        rc, rmass = sim.raster(mass_quantum=q, out=(hc, hm), **v)           # pageable
        assert rc is hc and rmass is hm
        sim.raster(mass_quantum=q, out=(pc, pm), **v)                      # page-locked, known to the library
        for c_, m_ in ((hc, hm), (pc, pm)):
            assert np.array_equal(c_, wc) and np.array_equal(m_.view(np.uint32), wm.view(np.uint32))
        # count only: the mass array handed in on ANOTHER call stays as it is; then mass only
        hc[:], hm[:], pc[:], pm[:] = SENTINEL_C, SENTINEL_M, SENTINEL_C, SENTINEL_M
        assert sim.raster(out=hc, **v) is hc and np.array_equal(hc, wc) and (hm == SENTINEL_M).all()
        got = sim.raster(mass_quantum=q, out=(None, hm), **v)
        assert got[0] is None and got[1] is hm and np.array_equal(hm.view(np.uint32), wm.view(np.uint32))
        hc[:] = SENTINEL_C
        sim.raster(mass_quantum=q, out=(None, pm), **v)
        assert np.array_equal(pm.view(np.uint32), wm.view(np.uint32)) and (pc == SENTINEL_C).all() and (hc == SENTINEL_C).all()
        sim.raster(mass_quantum=q, out=(pc, None), **v)
        assert np.array_equal(pc, wc)
        # mixed: one plane page-locked, the other pageable
        hm[:] = SENTINEL_M
        sim.raster(mass_quantum=q, out=(pc, hm), **v)
        assert np.array_equal(pc, wc) and np.array_equal(hm.view(np.uint32), wm.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------------------------
def view_of(**kw) -> L.nb_view:
    v = L.nb_view()
    v.struct_size, v.width, v.height, v.center_x, v.center_y, v.scale, v.mass_quantum = C.sizeof(L.nb_view), 8, 8, 0.0, 0.0, 1.0, 1.0
    for k, val in kw.items():
        setattr(v, k, val)
    return v


REFUSED = [
    (dict(struct_size=28), "struct_size"), (dict(width=0), "width"), (dict(width=16385), "width"), (dict(height=0), "height"),
    (dict(height=16385), "height"), (dict(width=8192, height=4096), "width * view->height"), (dict(scale=0.0), "scale"),
    (dict(scale=-1.0), "scale"), (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(center_x=float("nan")), "center_x"), (dict(center_y=float("inf")), "center_y"), (dict(_reserved0=1), "_reserved0"),
    (dict(mass_quantum=0.0), "mass_quantum"), (dict(mass_quantum=-1.0), "mass_quantum"), (dict(mass_quantum=float("inf")), "mass_quantum"),
    (dict(mass_quantum=float("nan")), "mass_quantum"),
]


def test_refusals():
    x, y, m = fixture()
    lib = nb.load()
    count, mass = np.full(64, SENTINEL_C, np.uint32), np.full(64, SENTINEL_M, np.float32)
    with direct(bodies_of(x, y, m)) as sim:
        for kw, field in REFUSED:
            v = view_of(**kw)
            assert lib.nb_raster(sim._h, C.byref(v), count.ctypes.data, mass.ctypes.data) == L.NB_EINVAL, kw
            text = lib.nb_last_error().decode()
            assert text.startswith("nb_raster: ") and f"view->{field}" in text, (kw, text)
        v = view_of()
        assert lib.nb_raster(sim._h, None, count.ctypes.data, mass.ctypes.data) == L.NB_EINVAL and b"NULL view" in lib.nb_last_error()
        assert lib.nb_raster(sim._h, C.byref(v), None, None) == L.NB_EINVAL and b"count and mass are both NULL" in lib.nb_last_error()
        assert lib.nb_raster(None, C.byref(v), count.ctypes.data, None) == L.NB_EINVAL and b"NULL handle" in lib.nb_last_error()
        # a bad quantum is ignored when no mass plane is asked for
        bad_q = view_of(mass_quantum=float("nan"), center_x=float(np.median(x)), center_y=float(np.median(y)))
        assert (count == SENTINEL_C).all() and (mass == SENTINEL_M).all()
        assert lib.nb_raster(sim._h, C.byref(bad_q), count.ctypes.data, None) == L.NB_OK
        assert int(count.sum()) == int(rm.raster(x, y, m, 8, 8, (bad_q.center_x, bad_q.center_y), 1.0)[0].sum()) > 0
        # the Python front end names a bad size itself, before it allocates a plane (a negative one would wrap in the uint32 field)
        for kw, field in ((dict(width=0, height=8), "width"), (dict(width=-3, height=8), "width"), (dict(width=8, height=16385), "height"),
                          (dict(width=8192, height=4096), "width * height")):
            with pytest.raises(ValueError, match=f"raster: {field.replace('*', '[*]')} must be"):
                sim.raster(**kw)
        # NB_ESTATE between nb_step_begin and nb_step_finish
        count[:] = SENTINEL_C
        sim.step_begin(1e-2)
        assert lib.nb_raster(sim._h, C.byref(v), count.ctypes.data, None) == L.NB_ESTATE and b"a split step is in flight" in lib.nb_last_error()
        assert (count == SENTINEL_C).all()
        sim.step_finish()
        assert lib.nb_raster(sim._h, C.byref(v), count.ctypes.data, None) == L.NB_OK


# ---------------------------------------------------------------------------------------------------------------------
# 11. pending report
# ---------------------------------------------------------------------------------------------------------------------
def test_pending_report_leaves_through_nb_raster_once():
    import test_tree_gpu as ttg                     # the input that makes a build fail through the public interface, reused as it is
    flat = ttg.close_pairs()
    x, y, m = flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 6].copy()
    v, q = dict(width=16, height=16, center=(0.0, 0.0), scale=1.0), float(m[0])
    count, mass = np.full((16, 16), SENTINEL_C, np.uint32), np.full((16, 16), SENTINEL_M, np.float32)
    with ttg.tree_sim(ttg.bodies_of(flat), eps=0.05) as sim:
        sim.advance(1, 1e-3)
        with pytest.raises(L.NBodyError) as e:
            sim.raster(mass_quantum=q, out=(count, mass), **v)
        assert e.value.code == L.NB_ENOMEM and "frame 0" in str(e.value) and "nodes" in str(e.value)
        assert (count == SENTINEL_C).all() and (mass == SENTINEL_M).all()          # nothing was written
        got = sim.raster(mass_quantum=q, out=(count, mass), **v)                   # reported once: the next call succeeds
        assert_planes(got, x, y, m, v, q, "after the report")                      # (nothing was integrated: the positions stay)
        assert int(count.sum()) == flat.shape[0]


# ---------------------------------------------------------------------------------------------------------------------
# 12. workgroups that take several batches, carry their table from one to the next and empty it in between
# ---------------------------------------------------------------------------------------------------------------------
def test_workgroups_that_take_several_batches_and_flush_in_between():
    """Everything above gives a workgroup ONE batch of 256 bodies: the grid is min(batches, 16 x CUs) workgroups.  Six batches per
    workgroup (6.3 M bodies on 256 CUs; a tree handle, never stepped: a whole-system direct handle of that size would plan 70 GiB of
    slabs) reach what is left: the table carried from batch to batch, the flush between two batches once more than 1024 of its
    2048 slots are in use, and the adds into the emptied table after it.  One in sixteen bodies sits in a core of a few pixels, the
    others are spread evenly, shuffled together, so that every workgroup holds both kinds of pixel.  The test checks its own
    premise on the model's pixels: workgroup 0 fills more than 1024 slots within its first five batches."""
    with nb.Simulation(bodies_of([0.0, 1.0], [0.0, 1.0], [1.0, 1.0]), eps=0.5, device=0) as probe:
        grid = 16 * probe.sym_info()["cus"]
    n = 6 * grid * 256 + 259                         # workgroup 0 takes seven batches, the last one 3 bodies; most take six
    rng = np.random.default_rng(5)
    x, y = rng.uniform(-1.0, 1.0, (2, n)).astype(np.float32)
    core = rng.random(n) < 1.0 / 16
    x[core], y[core] = rng.normal(0.0, 1e-3, (2, int(core.sum()))).astype(np.float32)
    q = 2.0 ** -10
    m = ((1 + (np.arange(n) * 7919) % 1000) * q).astype(np.float32)      # whole quanta, exactly
    of_group0 = (np.arange(5)[:, None] * grid * 256 + np.arange(256)).ravel()       # the bodies of its first five batches
    views = {
        "scattered": dict(width=2048, height=2048, center=(0.013, -0.007), scale=921.6),       # 1.5 bodies per pixel, 10^4 in the core's
        "crowded": dict(width=128, height=128, center=(0.013, -0.007), scale=57.6),          # 360 per pixel, 4 x 10^5 in the core's
        "one pixel": dict(width=8, height=8, center=(-500.0, -500.0), scale=1e-3),            # sx = sy = 4.5 +- 0.001
    }
    with nb.Simulation(bodies_of(x, y, m), eps=0.5, force="tree", theta=0.5, tree_leaves=True, device=0) as sim:
        for name, v in views.items():
            wc, wm = assert_planes(sim.raster(mass_quantum=q, **v), x, y, m, v, q, name)
            if name != "one pixel":
                inside, pixel = rm.pixels(x[of_group0], y[of_group0], **v)
                assert inside.all() and np.unique(pixel).size > 1024 + 64, name      # the flush comes after the fifth batch at the latest
                assert int(wc.sum()) == n and wc.max() > 10000
            if name != "scattered":                                      # the one-plane kernels keep other LDS arrays
                assert np.array_equal(sim.raster(**v), wc)
                assert np.array_equal(sim.raster(mass_quantum=q, out=(None, np.empty_like(wm)), **v)[1].view(np.uint32), wm.view(np.uint32))
        assert int(wc.sum()) == n and wc[4, 4] == n                      # the last view: every body in the centre pixel
        assert sim.tree_stats()["nodes"] == 0 and sim.frame == 0
