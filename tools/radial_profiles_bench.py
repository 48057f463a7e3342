"""Cost of the radial profiles: nb_radial_profiles with ONE centre whose last edge covers the system, with tens of thousands of
small centres, and with every body of one cell a centre, on one GPU, from one process.

    python tools/radial_profiles_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: d262144, d1048576 (Plummer spheres on direct-sum handles, eps 0.01, dt 1e-3), t8388608 (the same on a convergent tree
        handle: leaves, theta 0.5): one centre at the origin, last edge beyond the whole sphere; m1048576: the most bound bodies of
        nb_group_binding's groups on the d1048576 handle as centres; cell16384: 16 384 bodies inside ONE cell, one centre and every
        body a centre (the n^2 sweep, reported as a rate of body-centre tests); all five by default

Protocol (that of tools/pair_counts_bench.py): every handle first steps for at least 2 s (settled clocks); 16 shells, edges 0 and then
16 values spaced geometrically from last / 64 to last.  Per row one untimed call (the first call allocates) and FIVE timed stretches
of back-to-back calls under the host clock: the five per-call figures, their median and their spread (max - min); beside them the
device time of the sweep alone (nb_profile_read: events around the sweep and its combine launch).  Records go into nb_host_alloc
memory, and into a pageable array in a row of its own.  YARDSTICKS in the same process on the same handle: nb_raster's call (count and
mass planes of a 1024 x 1024 view that holds the sphere), the library's other O(n) binning pass; and the host route, one thread:
nb_sync and numpy.histogram with weights for one centre; nb_sync and scipy's cKDTree.query_ball_point with a numpy pass per centre
for many (numpy per centre on a sample of 256 centres, scaled and labelled as scaled, where scipy is missing).  One JSON line per
row, appended to FILE (default profiles/radial_profiles_bench.log) and printed.  The process ends itself after --limit seconds
(default 900).
"""
from __future__ import annotations

import ctypes as C
import json
import signal
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import nbodysim_amd as nb  # noqa: E402
import numpy as np  # noqa: E402
from nbodysim_amd import _lib as L  # noqa: E402

from groups_bench import find_radius, kernel_ms  # noqa: E402
from raster_bench import timed_row  # noqa: E402
from tree_bench import settle  # noqa: E402

DT = 1e-3
NBINS = 16
CENTRES_MAX = 65536


def edges_of(last: float) -> np.ndarray:
    return np.concatenate([[0.0], np.geomspace(last / 64, last, NBINS)]).astype(np.float32)


def open_case(case: str):
    if case.startswith("cell"):
        n = int(case[4:])
        b = nb.bodies_array(n)
        b["pos"] = np.random.default_rng(1).uniform(-0.3, 0.3, (n, 2)).astype(np.float32)
        b["vel"] = np.random.default_rng(2).normal(0, 1, (n, 2)).astype(np.float32)
        b["mass"] = 1.0 / n
        return nb.Simulation(b, eps=0.01, device=0), n
    n = int(case[1:])
    kw = dict(force="tree", theta=0.5, tree_leaves=True) if case[0] == "t" else {}
    return nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, **kw), n


class Pinned:
    """`records` nb_shell records over an nb_host_alloc block"""

    def __init__(self, lib, records: int):
        self.lib, self.ptr = lib, lib.nb_host_alloc(records * 64)
        assert self.ptr
        self.array = np.frombuffer((C.c_uint8 * (records * 64)).from_address(self.ptr), dtype=L.SHELL_DTYPE)

    def __enter__(self):
        return self.array

    def __exit__(self, *exc):
        self.array = None
        assert self.lib.nb_host_free(self.ptr) == 0


def profile_rows(sim, lib, base: dict, cen: np.ndarray, vc, edges: np.ndarray, emit, tests_per_call=None) -> None:
    records = cen.shape[0] * NBINS
    with Pinned(lib, records) as pinned:
        for where, out in (("nb_host_alloc", pinned), ("pageable", np.zeros(records, L.SHELL_DTYPE))):
            def call():
                L.check("nb_radial_profiles", lib.nb_radial_profiles(sim._h, cen.ctypes.data, None if vc is None else vc.ctypes.data, cen.shape[0],
                                                                     edges.ctypes.data, NBINS, out.ctypes.data), lib)
            row = dict(base, call="nb_radial_profiles", centres=int(cen.shape[0]), nbins=NBINS, records_into=where)
            sim.profile(False)
            timed_row(call, row)
            if where == "nb_host_alloc":
                kernel_ms(sim, call, row["calls_per_stretch"], row, "sweep_ms")
                if tests_per_call:
                    row["tests_per_s"] = round(tests_per_call / (row["sweep_ms_median"] * 1e-3), 0)
            row["bodies_in_shells"] = int(out["count"].sum())
            emit(row)


def raster_row(sim, lib, base: dict, n: int, emit) -> None:
    w = h = 1024
    count, mass = np.zeros((h, w), np.uint32), np.zeros((h, w), np.float32)
    v = L.nb_view()
    v.struct_size, v.width, v.height, v.scale, v.mass_quantum = C.sizeof(L.nb_view), w, h, 25.6, 1.0 / n / 16

    def call():
        L.check("nb_raster", lib.nb_raster(sim._h, C.byref(v), count.ctypes.data, mass.ctypes.data), lib)
    row = dict(base, call="nb_raster, count and mass planes, 1024 x 1024 (the yardstick)")
    timed_row(call, row)
    emit(row)


def host_one_centre(sim, lib, base: dict, n: int, edges: np.ndarray, emit) -> None:
    bodies = nb.bodies_array(n)
    t0 = time.perf_counter()
    L.check("nb_sync", lib.nb_sync(sim._h, bodies.ctypes.data), lib)
    t1 = time.perf_counter()
    p, v, m = bodies["pos"].astype(np.float64), bodies["vel"].astype(np.float64), bodies["mass"].astype(np.float64)
    r = np.hypot(p[:, 0], p[:, 1])
    vr = (p * v).sum(axis=1) / np.where(r > 0, r, 1.0)
    terms = (None, m, m * r, m * r * r, m * vr, m * vr * vr, m * (v * v).sum(axis=1), m * (p[:, 0] * v[:, 1] - p[:, 1] * v[:, 0]))
    hist = [np.histogram(r, bins=edges.astype(np.float64), weights=t)[0] for t in terms]
    t2 = time.perf_counter()
    emit(dict(base, call="host route: nb_sync, numpy.histogram with weights (count and seven sums)", threads=1, sync_ms=round((t1 - t0) * 1e3, 2),
              numpy_ms=round((t2 - t1) * 1e3, 1), total_ms=round((t2 - t0) * 1e3, 1), bodies_in_shells=int(hist[0].sum())))


def host_many_centres(sim, lib, base: dict, n: int, cen: np.ndarray, edges: np.ndarray, emit) -> None:
    bodies = nb.bodies_array(n)
    t0 = time.perf_counter()
    L.check("nb_sync", lib.nb_sync(sim._h, bodies.ctypes.data), lib)
    t1 = time.perf_counter()
    p, m = bodies["pos"].astype(np.float64), bodies["mass"].astype(np.float64)
    e = edges.astype(np.float64)

    def one(c, idx):
        r = np.hypot(p[idx, 0] - cen[c, 0], p[idx, 1] - cen[c, 1])
        return np.histogram(r, bins=e, weights=m[idx])[0]
    try:
        from scipy.spatial import cKDTree
        balls = cKDTree(p).query_ball_point(cen.astype(np.float64), float(e[-1]))
        t2 = time.perf_counter()
        total = sum(one(c, np.asarray(idx, np.int64)).sum() for c, idx in enumerate(balls))
        t3 = time.perf_counter()
        emit(dict(base, call="host route: nb_sync, cKDTree.query_ball_point, numpy.histogram of mass per centre", threads=1, centres=int(cen.shape[0]),
                  sync_ms=round((t1 - t0) * 1e3, 2), tree_ms=round((t2 - t1) * 1e3, 1), numpy_ms=round((t3 - t2) * 1e3, 1),
                  total_ms=round((t3 - t0) * 1e3, 1), mass_in_shells=float(total)))
    except ImportError:
        sample = np.random.default_rng(3).choice(cen.shape[0], min(256, cen.shape[0]), replace=False)
        t2 = time.perf_counter()
        for c in sample:
            one(c, np.flatnonzero(np.hypot(p[:, 0] - cen[c, 0], p[:, 1] - cen[c, 1]) < e[-1]))
        t3 = time.perf_counter()
        scaled = (t3 - t2) * cen.shape[0] / sample.size
        emit(dict(base, call="host route: nb_sync, numpy per centre on a sample, SCALED to all centres", threads=1, centres=int(cen.shape[0]),
                  sample=int(sample.size), sync_ms=round((t1 - t0) * 1e3, 2), numpy_ms_scaled=round(scaled * 1e3, 1),
                  total_ms_scaled=round((t1 - t0 + scaled) * 1e3, 1)))


def run(case: str, emit) -> None:
    lib = nb.load()
    many = case.startswith("m")
    sim, n = open_case("d" + case[1:] if many else case)
    with sim:
        settle(sim, DT)
        base = {"case": case, "n": n}
        if case.startswith("cell"):
            edges = edges_of(1.0)
            pos = np.ascontiguousarray(sim.sync()["pos"])
            profile_rows(sim, lib, dict(base, last_edge=1.0), np.zeros((1, 2), np.float32), None, edges, emit, tests_per_call=float(n))
            profile_rows(sim, lib, dict(base, last_edge=1.0), pos, None, edges, emit, tests_per_call=float(n) * n)
        elif many:
            radius, mean = find_radius(sim, lib, n, 1.0)
            rec = sim.group_binding(radius, 2, phi=False, e=False, records=True)
            cat = sim.group_catalog(radius, 2)
            keep = np.argsort(-rec["members"].astype(np.int64), kind="stable")[:CENTRES_MAX]
            pos = sim.sync()["pos"]
            ok = rec["most_bound"][keep] != L.NB_NO_NEIGHBOR
            keep = keep[ok]
            cen = np.ascontiguousarray(pos[rec["most_bound"][keep]], np.float32)
            vc = np.ascontiguousarray(cat["vel"][keep, :2])
            last = 4 * radius
            base = dict(base, linking_length=radius, mean_links=round(mean, 2), groups=int(rec.shape[0]), last_edge=last)
            profile_rows(sim, lib, base, cen, vc, edges_of(last), emit)
            host_many_centres(sim, lib, base, n, cen, edges_of(last), emit)
        else:
            last = float(np.abs(sim.sync()["pos"]).max()) * 1.5 + 1.0
            edges = edges_of(last)
            base = dict(base, last_edge=last)
            profile_rows(sim, lib, base, np.zeros((1, 2), np.float32), None, edges, emit, tests_per_call=float(n))
            raster_row(sim, lib, base, n, emit)
            host_one_centre(sim, lib, base, n, edges, emit)


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "radial_profiles_bench.log", 900
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"radial_profiles_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "radial_profiles_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name)})
        for case in args or ["d262144", "d1048576", "t8388608", "m1048576", "cell16384"]:
            run(case, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
