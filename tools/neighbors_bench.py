"""Cost of "who is near every body": nb_neighbors beside nb_sync_positions and nb_sync, on one GPU, from one process.

    python tools/neighbors_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: d262144, d1048576 (Plummer spheres on direct-sum handles, eps 0.01, dt 1e-3), t8388608 (the same on a convergent tree
        handle: leaves, theta 0.5) and cell16384 (16 384 bodies inside ONE cell: the n^2 sweep, reported as a pair rate); all four by
        default

    python tools/neighbors_bench.py --ab [--out FILE] [case ...]
        the search kernel only (default cases d262144 d1048576), for the A/B of DESIGN.md: run alternately, twice each, with the
        product library and with a build of the per-lane form from the same source:
            make -C nbodysim_amd/csrc BUILD=$PWD/build/perlane OUT=$PWD/build/perlane/libnbody_hip.so EXTRA=-DNB_NEIGHBORS_PER_LANE
            NBODY_HIP_LIB=build/perlane/libnbody_hip.so python tools/neighbors_bench.py --ab
        (the Python binding loads $NBODY_HIP_LIB when set; the LIBRARY reads no environment variables)

    python tools/neighbors_bench.py --kernels [case ...]
        twenty calls with k = 5 and nothing else, to be run under a kernel trace (rocprofv3 --kernel-trace --stats -- python ...):
        the sort (rocPRIM's kernels), neighbors_keys, neighbors_gather and neighbors_search each alone

Protocol (that of tools/raster_bench.py): every handle first steps for at least 2 s (settled clocks); the radius is found by doubling
and then bisecting on the count-only call until the mean count lies in 16 .. 32; then, per row, one untimed call (the first call
allocates) and FIVE timed stretches of back-to-back calls under the host clock; a row reports the five per-call figures, their median
and their spread (max - min).  Per handle: the whole call for k = 5 and 16 into pageable numpy arrays and into nb_host_alloc memory
(idx and count), beside each the device time of the search kernel alone (nb_profile_read: events around it); the count-only call;
nb_sync_positions and nb_sync, which a caller pays today before the host pass even starts.  One JSON line per row, appended to FILE
(default profiles/neighbors_bench.log) and printed.  The process ends itself after --limit seconds (default 900).
"""
from __future__ import annotations

import json
import signal
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import nbodysim_amd as nb  # noqa: E402
import numpy as np  # noqa: E402
from nbodysim_amd import _lib as L  # noqa: E402

from raster_bench import timed_row  # noqa: E402
from tree_bench import settle, stats_of  # noqa: E402

DT = 1e-3
KS = (5, 16)


class Pinned:
    """`count` 4-byte elements over an nb_host_alloc block."""

    def __init__(self, lib, count):
        self.lib, self.ptr = lib, lib.nb_host_alloc(count * 4)
        if not self.ptr:
            raise MemoryError("nb_host_alloc")

    def close(self):
        L.check("nb_host_free", self.lib.nb_host_free(self.ptr), self.lib)


def open_case(case: str):
    if case.startswith("cell"):
        n = int(case[4:])
        b = nb.bodies_array(n)
        b["pos"] = np.random.default_rng(1).uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
        b["mass"] = 1.0 / n
        return nb.Simulation(b, eps=0.01, device=0), n
    n = int(case[1:])
    kw = dict(force="tree", theta=0.5, tree_leaves=True) if case[0] == "t" else {}
    return nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, **kw), n


def find_radius(sim, lib, n: int, emit, case: str) -> float:
    """Doubling, then bisection, on the count-only call: the mean count in 16 .. 32."""
    count = np.zeros(n, np.uint32)

    def mean(r):
        L.check("nb_neighbors", lib.nb_neighbors(sim._h, r, 0, None, None, count.ctypes.data), lib)
        return float(count.mean(dtype=np.float64))
    r = 1e-4
    m = mean(r)
    while m < 16:
        r *= 2
        m = mean(r)
    lo, hi = r / 2, r
    for _ in range(40):
        if 16 <= m <= 32:
            break
        r = (lo * hi) ** 0.5
        m = mean(r)
        if m < 16:
            lo = r
        elif m > 32:
            hi = r
    emit({"case": case, "n": n, "radius": r, "mean_count": round(m, 2), "max_count": int(count.max()), "over_5": round(float((count > 5).mean()), 4),
          "over_16": round(float((count > 16).mean()), 4)})
    return r


def search_ms(sim, call, calls: int, row: dict) -> None:
    sim.profile(True)                                        # the search alone: device events around neighbors_search
    sim.profile_read()
    v = []
    for _ in range(5):
        for _ in range(calls):
            call()
        ms, launches = sim.profile_read()
        v.append(ms / launches)
    sim.profile(False)
    stats_of("search_ms", v, row)


def run(case: str, emit, mode: str) -> None:
    lib = nb.load()
    sim, n = open_case(case)
    with sim:
        settle(sim, DT)
        one_cell = case.startswith("cell")
        radius = 10.0 if one_cell else find_radius(sim, lib, n, emit, case)
        kmax = max(KS)
        pageable = np.zeros(n * kmax, np.uint32), np.zeros(n, np.uint32)
        if mode == "kernels":
            for _ in range(20):
                L.check("nb_neighbors", lib.nb_neighbors(sim._h, radius, 5, pageable[0].ctypes.data, None, pageable[1].ctypes.data), lib)
            emit({"case": case, "n": n, "radius": radius, "kernels": "20 calls with k = 5, idx and count"})
            return
        pins = [Pinned(lib, n * kmax), Pinned(lib, n)]
        try:
            for k in KS:
                for dest, (pi, pc) in (("pageable", (pageable[0].ctypes.data, pageable[1].ctypes.data)), ("nb_host_alloc", (pins[0].ptr, pins[1].ptr))):
                    if (mode == "ab" or one_cell) and dest != "pageable":
                        continue

                    def call():
                        L.check("nb_neighbors", lib.nb_neighbors(sim._h, radius, k, pi, None, pc), lib)
                    row = {"case": case, "n": n, "call": "nb_neighbors", "k": k, "radius": radius, "dest": dest, "bytes": n * 4 * (k + 1)}
                    sim.profile(False)
                    timed_row(call, row)
                    search_ms(sim, call, row["calls_per_stretch"], row)
                    if one_cell:
                        row["pairs_per_s"] = round(n * (n - 1.0) / (row["search_ms_median"] * 1e-3), 0)
                    emit(row)
            if mode == "ab" or one_cell:
                return
            row = {"case": case, "n": n, "call": "nb_neighbors", "k": 0, "radius": radius, "dest": "pageable", "bytes": n * 4}
            timed_row(lambda: L.check("nb_neighbors", lib.nb_neighbors(sim._h, radius, 0, None, None, pageable[1].ctypes.data), lib), row)
            emit(row)
            xy = np.zeros((n, 2), np.float32)
            for name, dst, nbytes, fn in (("nb_sync_positions", xy, n * 8, lib.nb_sync_positions), ("nb_sync", sim.bodies, n * 64, lib.nb_sync)):
                row = {"case": case, "n": n, "call": name, "bytes": nbytes}
                timed_row(lambda: L.check(name, fn(sim._h, dst.ctypes.data), lib), row)
                emit(row)
        finally:
            for p in pins:
                p.close()


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "neighbors_bench.log", 900
    mode = "ab" if "--ab" in args else "kernels" if "--kernels" in args else "all"
    for flag in ("--ab", "--kernels"):
        if flag in args:
            args.remove(flag)
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"neighbors_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "neighbors_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name), "mode": mode})
        default = {"ab": ["d262144", "d1048576"], "kernels": ["d1048576"], "all": ["d262144", "d1048576", "t8388608", "cell16384"]}[mode]
        for case in args or default:
            run(case, emit, mode)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
