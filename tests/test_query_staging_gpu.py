"""GPU: the query calls (nb_raster, nb_groups, nb_neighbors, nb_tree_nodes) share one page-locked staging buffer on the handle.
Queries of different kinds, with planes that grow and shrink, meet in it here; every pageable result must equal, bit for bit, what
the same call writes by direct DMA into nb_host_alloc memory on a second handle, where the staging is never touched."""
import ctypes as C

import numpy as np
import pytest

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

pytestmark = pytest.mark.gpu
N, GUARD, FILL = 1024, 64, 0xA7
RADIUS_NEAR, RADIUS_LINK, QUANTUM = 1.0, 0.5, 2.0 ** -10


def bodies() -> np.ndarray:
    rng = np.random.default_rng(11)
    b = nb.bodies_array(N)
    b["pos"] = rng.uniform(-10.0, 10.0, (N, 2)).astype(np.float32)
    b["vel"] = rng.uniform(-0.1, 0.1, (N, 2)).astype(np.float32)
    b["mass"] = rng.uniform(0.5, 1.5, N).astype(np.float32)
    return b


class Pageable:
    """`count` elements of `dtype` in the middle of a numpy byte array, GUARD sentinel bytes before and after."""

    def __init__(self, count, dtype):
        size = count * np.dtype(dtype).itemsize
        self.raw = np.full(size + 2 * GUARD, FILL, np.uint8)
        self.array = self.raw[GUARD:GUARD + size].view(dtype)

    def intact(self) -> bool:
        return bool((self.raw[:GUARD] == FILL).all() and (self.raw[-GUARD:] == FILL).all())

    def close(self):
        pass


class PageLocked:
    """`count` elements of `dtype` over an nb_host_alloc block: the copy engine writes it directly."""

    def __init__(self, count, dtype):
        size = count * np.dtype(dtype).itemsize
        self.lib = nb.load()
        self.ptr = self.lib.nb_host_alloc(size)
        assert self.ptr
        self.array = np.frombuffer((C.c_uint8 * size).from_address(self.ptr), dtype=dtype)
        self.array.view(np.uint8)[:] = FILL

    def intact(self) -> bool:
        return True

    def close(self):
        self.array = None
        assert self.lib.nb_host_free(self.ptr) == 0


def run_queries(sim, kind) -> list:
    """The sequence of the issue on `sim`, every destination of `kind`; the results as (name, bytes) in order."""
    lib, out = nb.load(), []

    def call(name, rc, *dst):
        assert rc == L.NB_OK, (name, lib.nb_last_error())
        for k, d in enumerate(dst):
            assert d.intact(), f"{name}: a sentinel beside plane {k} was overwritten"
            out.append((f"{name}[{k}]", d.array.view(np.uint8).copy()))
            d.close()

    def raster(side):
        v = L.nb_view()
        v.struct_size = C.sizeof(L.nb_view)
        v.width = v.height = side
        v.center_x = v.center_y = 0.0
        v.scale, v.mass_quantum = side / 20.0, QUANTUM
        cnt, mass = kind(side * side, np.uint32), kind(side * side, np.float32)
        rc = lib.nb_raster(sim._h, C.byref(v), cnt.array.ctypes.data, mass.array.ctypes.data)
        assert rc != L.NB_OK or 0 < int(cnt.array.sum(dtype=np.uint64)) <= N
        call(f"raster {side}", rc, cnt, mass)

    def groups():
        label, size = kind(N, np.uint32), kind(N, np.uint32)
        call("groups", lib.nb_groups(sim._h, RADIUS_LINK, label.array.ctypes.data, size.array.ctypes.data, None), label, size)

    def neighbors(k):
        idx, d2, cnt = kind(N * k, np.uint32), kind(N * k, np.float32), kind(N, np.uint32)
        call(f"neighbors k={k}", lib.nb_neighbors(sim._h, RADIUS_NEAR, k, *(a.array.ctypes.data for a in (idx, d2, cnt))), idx, d2, cnt)

    def tree_nodes():
        count = C.c_size_t()
        assert lib.nb_tree_nodes(sim._h, None, 0, C.byref(count)) == L.NB_OK and count.value > N
        nodes = kind(count.value, L.NODE_DTYPE)
        call("tree_nodes", lib.nb_tree_nodes(sim._h, nodes.array.ctypes.data, count.value, C.byref(count)), nodes)

    raster(8)
    groups()
    neighbors(32)
    tree_nodes()
    raster(1024)            # 4 MiB per plane: above copy_d2h's 1 MiB bound, four staged pieces, after a regrow of the shared buffer
    neighbors(1)
    groups()
    tree_nodes()
    raster(8)
    return out


def test_queries_of_every_kind_meet_in_one_staging_buffer():
    start = bodies()
    with nb.Simulation(start, force="tree", device=0, eps=0.5) as a, nb.Simulation(start, force="tree", device=0, eps=0.5) as b, \
            nb.Simulation(start, force="tree", device=0, eps=0.5) as never_queried:
        for sim in (a, b, never_queried):
            sim.advance(1, 1e-2)
        want = run_queries(b, PageLocked)
        got = run_queries(a, Pageable)
        assert [name for name, _ in got] == [name for name, _ in want] and len(got) == 18
        for (name, g), (_, w) in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), f"{name}: the staged bytes differ from the directly copied ones"
            assert (g != FILL).any(), f"{name}: nothing was written"
        # the queries leave the trajectory alone
        a.advance(10, 1e-2)
        never_queried.advance(10, 1e-2)
        assert a.sync().tobytes() == never_queried.sync().tobytes()
