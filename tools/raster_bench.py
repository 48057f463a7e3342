"""Cost of a frame as an image: nb_raster beside nb_sync_positions and nb_sync, on one GPU, from one process.

    python tools/raster_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: t262144, t1048576, t8388608 (Plummer spheres on convergent tree handles: leaves, theta 0.5, eps 0.01, dt 1e-3) and
        d262144 (the direct sum on the same bodies); all four by default

    python tools/raster_bench.py --ab [--out FILE] [case ...]
        the rows of nb_raster only (default case t1048576): run once with the product library and once with a build of the plainest
        form, one global add per body and no combining, from the same source:
            make -C nbodysim_amd/csrc BUILD=$PWD/build/plain OUT=$PWD/build/plain/libnbody_hip.so EXTRA=-DNB_RASTER_PLAIN
            NBODY_HIP_LIB=build/plain/libnbody_hip.so python tools/raster_bench.py --ab
        (the Python binding loads $NBODY_HIP_LIB when set; the LIBRARY reads no environment variables)

Protocol (that of tools/tree_bench.py): every handle first steps for at least 2 s (settled clocks); then, per row, one untimed call
(the first call allocates) and FIVE timed stretches of back-to-back calls under the host clock, each call into the same pageable,
already touched numpy arrays; a row reports the five per-call figures, their median and their spread (max - min).  Views, all
1024 x 1024 about the origin: `sphere` scale 25.6 (the whole r <= 20 sphere), `core` scale 2048, `one_pixel` scale 1e-3 (every body in
one pixel).  Per view: nb_raster with the counts only and with both planes, and beside each the device time of the bin pass alone
(nb_profile_read: events around raster_bin).  Per handle: nb_sync_positions and nb_sync.  One JSON line per row, appended to FILE
(default profiles/raster_bench.log) and printed; then per handle the bar of DESIGN.md: nb_raster (sphere, both planes) against
nb_sync_positions, medians and the larger spread.  The process ends itself after --limit seconds (default 900).
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

from tree_bench import settle, stats_of  # noqa: E402

W = H = 1024
VIEWS = (("sphere", 25.6), ("core", 2048.0), ("one_pixel", 1e-3))
DT = 1e-3


def stretches(call, est_ms: float, count: int = 5, stretch_s: float = 0.2):
    """`count` stretches of back-to-back calls, about stretch_s each: milliseconds per call of every stretch."""
    k = max(3, min(int(stretch_s * 1e3 / max(est_ms, 1e-3)), 200))
    out = []
    for _ in range(count):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        out.append((time.perf_counter() - t0) / k * 1e3)
    return out, k


def timed_row(call, row: dict, name: str = "call_ms"):
    call()                                                   # allocations, first-touch
    t0 = time.perf_counter()
    call()
    est = (time.perf_counter() - t0) * 1e3
    v, k = stretches(call, est)
    row["calls_per_stretch"] = k
    stats_of(name, v, row)


def open_case(case: str):
    n = int(case[1:])
    kw = dict(force="tree", theta=0.5, tree_leaves=True) if case[0] == "t" else {}
    return nb.Simulation(nb.plummer_2d(n, 42), rsqrt="exact", eps=0.01, device=0, **kw), n


def raster_rows(sim, lib, case: str, n: int, emit) -> dict:
    count, mass = np.zeros((H, W), np.uint32), np.zeros((H, W), np.float32)
    rows = {}
    for view, scale in VIEWS:
        v = L.nb_view()
        v.struct_size, v.width, v.height, v.scale, v.mass_quantum = C.sizeof(L.nb_view), W, H, scale, 1.0 / n / 16
        for planes in ("count", "both"):
            m = mass.ctypes.data if planes == "both" else None

            def call():
                L.check("nb_raster", lib.nb_raster(sim._h, C.byref(v), count.ctypes.data, m), lib)
            row = {"case": case, "n": n, "call": "nb_raster", "view": view, "scale": scale, "planes": planes, "bytes": W * H * (8 if m else 4)}
            sim.profile(False)
            timed_row(call, row)
            sim.profile(True)                                # the bin pass alone: device events around raster_bin
            sim.profile_read()
            bins = []
            for _ in range(5):
                for _ in range(row["calls_per_stretch"]):
                    call()
                ms, launches = sim.profile_read()
                bins.append(ms / launches)
            sim.profile(False)
            stats_of("bin_ms", bins, row)
            row["inside"] = int(count.sum(dtype=np.uint64))
            row["fullest_pixel"] = int(count.max())
            rows[view, planes] = row
            emit(row)
    return rows


def run(case: str, emit, ab: bool) -> None:
    lib = nb.load()
    sim, n = open_case(case)
    with sim:
        settle(sim, DT)
        rows = raster_rows(sim, lib, case, n, emit)
        if ab:
            return
        xy = np.zeros((n, 2), np.float32)
        for name, dst, nbytes, fn in (("nb_sync_positions", xy, n * 8, lib.nb_sync_positions), ("nb_sync", sim.bodies, n * 64, lib.nb_sync)):
            row = {"case": case, "n": n, "call": name, "bytes": nbytes}
            timed_row(lambda: L.check(name, fn(sim._h, dst.ctypes.data), lib), row)
            rows[name] = row
            emit(row)
        r, p = rows["sphere", "both"], rows["nb_sync_positions"]
        margin = max(r["call_ms_spread"], p["call_ms_spread"])
        emit({"case": case, "n": n, "bar": "nb_raster (sphere, both planes) below nb_sync_positions by more than the larger spread",
              "raster_ms": r["call_ms_median"], "sync_positions_ms": p["call_ms_median"], "larger_spread_ms": margin,
              "met": bool(r["call_ms_median"] + margin < p["call_ms_median"])})


def main(argv) -> int:
    args = list(argv)
    out, limit, ab = ROOT / "profiles" / "raster_bench.log", 900, "--ab" in args
    if ab:
        args.remove("--ab")
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"raster_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "raster_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name), "ab": ab,
              "view": f"{W} x {H}"})
        for case in args or (["t1048576"] if ab else ["t262144", "t1048576", "t8388608", "d262144"]):
            run(case, emit, ab)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
