"""Cost of "which bodies form a clump": nb_groups beside the nb_neighbors count-only call and the host route it replaces, on one GPU,
from one process.

    python tools/groups_bench.py [--out FILE] [--limit SECONDS] [--no-host] [case ...]
        cases: d262144, d1048576 (Plummer spheres on direct-sum handles, eps 0.01, dt 1e-3), t8388608 (the same on a convergent tree
        handle: leaves, theta 0.5) and one1048576 (a 1024 x 1024 unit lattice at radius 1.1: four links per body and ALL bodies in
        ONE group, the worst case of the size pass); the first three by default

    python tools/groups_bench.py --kernels [case ...]
        twenty calls asking for all three outputs and nothing else, to be run under a kernel trace
        (rocprofv3 --kernel-trace --stats -- python ...): the sort (rocPRIM's kernels), neighbors_keys, neighbors_gather, groups_link,
        groups_flatten, groups_roots, groups_tally and groups_sizes each alone.  Default cases d1048576 one1048576.  For the A/B of the
        size pass run it once more with a build whose size pass adds once per body:
            make -C nbodysim_amd/csrc BUILD=$PWD/build/plaintally OUT=$PWD/build/plaintally/libnbody_hip.so EXTRA=-DNB_GROUPS_PLAIN_TALLY
            NBODY_HIP_LIB=build/plaintally/libnbody_hip.so rocprofv3 --kernel-trace --stats -- python tools/groups_bench.py --kernels one1048576
        (the Python binding loads $NBODY_HIP_LIB when set; the LIBRARY reads no environment variables)

Protocol (that of tools/neighbors_bench.py): every handle first steps for at least 2 s (settled clocks); per handle three radii are
found by bisection on nb_neighbors' count-only call, for a mean neighbour count near 1 (sparse), 5 and 30 (one giant group percolates
and the union-find is deepest); then, per row, one untimed call (the first call allocates) and FIVE timed stretches of back-to-back
calls under the host clock; a row reports the five per-call figures, their median and their spread (max - min).  Per handle and radius:
the whole call, all three outputs, into nb_host_alloc memory and into pageable numpy arrays, beside each the device time of the link
kernel alone (nb_profile_read: events around it); the labels alone; ngroups alone (no plane leaves the device); nb_neighbors' count-only
call with its search kernel: it tests the same candidates, twice as many pairs, with no parent[] traffic, so it is the yardstick for
what the union-find costs; and, ONCE (it takes seconds), the host route nb_groups replaces: nb_sync_positions, scipy's
cKDTree.query_pairs (one thread: it has no `workers`), scipy's connected_components.  The host route is skipped at 8 388 608 bodies.
One JSON line per row, appended to FILE (default profiles/groups_bench.log) and printed.  The process ends itself after --limit
seconds (default 900).
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

from neighbors_bench import Pinned  # noqa: E402
from raster_bench import timed_row  # noqa: E402
from tree_bench import settle, stats_of  # noqa: E402

DT = 1e-3
TARGETS = (1.0, 5.0, 30.0)


def open_case(case: str):
    if case.startswith("one"):
        n = int(case[3:])
        side = int(round(n ** 0.5))
        assert side * side == n
        b = nb.bodies_array(n)
        gx, gy = np.meshgrid(np.arange(side, dtype=np.float32) - side / 2, np.arange(side, dtype=np.float32) - side / 2)
        order = np.random.default_rng(1).permutation(n)
        b["pos"][:, 0], b["pos"][:, 1] = gx.ravel()[order], gy.ravel()[order]
        b["mass"] = 1.0 / n
        return nb.Simulation(b, eps=0.01, device=0), n
    n = int(case[1:])
    kw = dict(force="tree", theta=0.5, tree_leaves=True) if case[0] == "t" else {}
    return nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, **kw), n


def find_radius(sim, lib, n: int, target: float) -> tuple:
    """Doubling, then bisection, on nb_neighbors' count-only call: the mean count within 10 % of `target`."""
    count = np.zeros(n, np.uint32)

    def mean(r):
        L.check("nb_neighbors", lib.nb_neighbors(sim._h, r, 0, None, None, count.ctypes.data), lib)
        return float(count.mean(dtype=np.float64))
    r = 1e-5
    m = mean(r)
    while m < target:
        r *= 2
        m = mean(r)
    lo, hi = r / 2, r
    for _ in range(40):
        if 0.9 * target <= m <= 1.1 * target:
            break
        r = (lo * hi) ** 0.5
        m = mean(r)
        if m < target:
            lo = r
        else:
            hi = r
    return r, m


def kernel_ms(sim, call, calls: int, row: dict, name: str) -> None:
    sim.profile(True)                                        # device events around the one bracketed kernel of the call
    sim.profile_read()
    v = []
    for _ in range(5):
        for _ in range(calls):
            call()
        ms, launches = sim.profile_read()
        v.append(ms / launches)
    sim.profile(False)
    stats_of(name, v, row)


def host_route(sim, lib, n: int, radius: float, row: dict) -> None:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    xy = np.zeros((n, 2), np.float32)
    t0 = time.perf_counter()
    L.check("nb_sync_positions", lib.nb_sync_positions(sim._h, xy.ctypes.data), lib)
    t1 = time.perf_counter()
    pairs = cKDTree(xy).query_pairs(radius, output_type="ndarray")
    t2 = time.perf_counter()
    ncomp, _ = connected_components(coo_matrix((np.ones(len(pairs), np.uint8), (pairs[:, 0], pairs[:, 1])), shape=(n, n)), directed=False)
    t3 = time.perf_counter()
    row.update(sync_positions_ms=round((t1 - t0) * 1e3, 2), query_pairs_ms=round((t2 - t1) * 1e3, 1), components_ms=round((t3 - t2) * 1e3, 1),
               total_ms=round((t3 - t0) * 1e3, 1), pairs=int(len(pairs)), ngroups_float64=int(ncomp), threads=1)


def run(case: str, emit, mode: str, host: bool) -> None:
    lib = nb.load()
    sim, n = open_case(case)
    with sim:
        settle(sim, DT)
        one = case.startswith("one")
        radii = [(1.1, 4.0)] if one else [find_radius(sim, lib, n, t) for t in TARGETS]
        pageable = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        count = C.c_uint64(0)
        if mode == "kernels":
            radius = radii[-1][0]
            for _ in range(20):
                L.check("nb_groups", lib.nb_groups(sim._h, radius, pageable[0].ctypes.data, pageable[1].ctypes.data, C.byref(count)), lib)
            emit({"case": case, "n": n, "radius": radius, "ngroups": int(count.value), "largest": int(pageable[1].max()),
                  "kernels": "20 calls with label, size and ngroups"})
            return
        pins = [Pinned(lib, n), Pinned(lib, n)]
        try:
            for radius, mean_count in radii:
                base = {"case": case, "n": n, "radius": radius, "mean_count": round(mean_count, 2)}
                L.check("nb_groups", lib.nb_groups(sim._h, radius, None, pageable[1].ctypes.data, C.byref(count)), lib)
                emit(dict(base, ngroups=int(count.value), largest=int(pageable[1].max()), in_groups_of_2_or_more=round(float((pageable[1] > 1).mean()), 4)))
                for what, dest, args in (("label size ngroups", "nb_host_alloc", (pins[0].ptr, pins[1].ptr, C.byref(count))),
                                         ("label size ngroups", "pageable", (pageable[0].ctypes.data, pageable[1].ctypes.data, C.byref(count))),
                                         ("label", "nb_host_alloc", (pins[0].ptr, None, None)),
                                         ("ngroups", "none", (None, None, C.byref(count)))):
                    def call():
                        L.check("nb_groups", lib.nb_groups(sim._h, radius, *args), lib)
                    row = dict(base, call="nb_groups", outputs=what, dest=dest)
                    sim.profile(False)
                    timed_row(call, row)
                    if what != "label":
                        kernel_ms(sim, call, row["calls_per_stretch"], row, "link_ms")
                    emit(row)

                def yardstick():
                    L.check("nb_neighbors", lib.nb_neighbors(sim._h, radius, 0, None, None, pageable[1].ctypes.data), lib)
                row = dict(base, call="nb_neighbors", outputs="count", dest="pageable")
                timed_row(yardstick, row)
                kernel_ms(sim, yardstick, row["calls_per_stretch"], row, "search_ms")
                emit(row)
                if host and n <= (1 << 20):
                    row = dict(base, call="host route: nb_sync_positions + cKDTree.query_pairs + connected_components", runs=1)
                    host_route(sim, lib, n, radius, row)
                    emit(row)
                elif host:
                    emit(dict(base, call="host route", skipped="minutes per run at this size"))
        finally:
            for p in pins:
                p.close()


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "groups_bench.log", 900
    mode = "kernels" if "--kernels" in args else "all"
    host = "--no-host" not in args
    for flag in ("--kernels", "--no-host"):
        if flag in args:
            args.remove(flag)
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"groups_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "groups_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name), "mode": mode})
        default = {"kernels": ["d1048576", "one1048576"], "all": ["d262144", "d1048576", "t8388608"]}[mode]
        for case in args or default:
            run(case, emit, mode, host)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
