"""Cost of the pair-separation histogram: nb_pair_counts beside nb_neighbors' count-only call at the same radius, on one GPU, from one
process.

    python tools/pair_counts_bench.py [--out FILE] [--limit SECONDS] [case ...]
        cases: d262144, d1048576 (Plummer spheres on direct-sum handles, eps 0.01, dt 1e-3), t8388608 (the same on a convergent tree
        handle: leaves, theta 0.5) and cell16384 (16 384 bodies inside ONE cell: the n^2 sweep, reported as a pair rate); all four by
        default

    python tools/pair_counts_bench.py --ab [--out FILE] [case ...]
        the count kernel only (default cases d262144 d1048576), for the A/B of DESIGN.md: run with the product library and with a
        build of the per-lane form from the same source:
            make -C nbodysim_amd/csrc BUILD=$PWD/build/perlane OUT=$PWD/build/perlane/libnbody_hip.so EXTRA=-DNB_PAIR_COUNTS_PER_LANE
            NBODY_HIP_LIB=build/perlane/libnbody_hip.so python tools/pair_counts_bench.py --ab
        (the Python binding loads $NBODY_HIP_LIB when set; the LIBRARY reads no environment variables)

Protocol (that of tools/groups_bench.py): every handle first steps for at least 2 s (settled clocks); per handle two last edges,
bisected on nb_neighbors' count-only call until the mean count is within 10 % of 5 and of 31; the edges are 0 and then nbins values
spaced geometrically from last / 64 to last, for nbins = 8, 16, 64 (bin capacities 8, 16, 64).  Per row one untimed call (the first
call allocates) and FIVE timed stretches of back-to-back calls under the host clock: the five per-call figures, their median and
their spread (max - min); beside them the device time of the count kernel alone (nb_profile_read: events around it).  THE YARDSTICK
of every last edge is nb_neighbors' count-only call at that radius on the same handle in the same process, the whole call and its
search kernel alone.  One JSON line per row, appended to FILE (default profiles/pair_counts_bench.log) and printed.  The process ends
itself after --limit seconds (default 900).
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

from groups_bench import find_radius, kernel_ms  # noqa: E402
from neighbors_bench import open_case  # noqa: E402
from raster_bench import timed_row  # noqa: E402
from tree_bench import settle  # noqa: E402

DT = 1e-3
TARGETS = (5.0, 31.0)
NBINS = (8, 16, 64)


def edges_of(last: float, nbins: int) -> np.ndarray:
    return np.concatenate([[0.0], np.geomspace(last / 64, last, nbins)]).astype(np.float32)


def run(case: str, emit, mode: str) -> None:
    lib = nb.load()
    sim, n = open_case(case)
    with sim:
        settle(sim, DT)
        one_cell = case.startswith("cell")
        count = np.zeros(n, np.uint32)
        for target in (None,) if one_cell else TARGETS:
            last, mean = (10.0, float(n - 1)) if one_cell else find_radius(sim, lib, n, target)
            base = {"case": case, "n": n, "last_edge": last, "mean_count": round(mean, 2)}
            for nbins in (16,) if one_cell else NBINS:
                edges = edges_of(last, nbins)
                out = np.zeros(nbins, np.uint64)

                def call():
                    L.check("nb_pair_counts", lib.nb_pair_counts(sim._h, edges.ctypes.data, nbins, out.ctypes.data), lib)
                row = dict(base, call="nb_pair_counts", nbins=nbins)
                sim.profile(False)
                if mode == "ab":
                    call()
                    row["calls_per_stretch"] = 20
                else:
                    timed_row(call, row)
                kernel_ms(sim, call, row["calls_per_stretch"], row, "count_kernel_ms")
                row["pairs_in_bins"] = int(out.sum())
                if one_cell:
                    row["pairs_per_s"] = round(n * (n - 1.0) / 2 / (row["count_kernel_ms_median"] * 1e-3), 0)
                emit(row)
            if mode == "ab":
                continue

            def yardstick():
                L.check("nb_neighbors", lib.nb_neighbors(sim._h, last, 0, None, None, count.ctypes.data), lib)
            row = dict(base, call="nb_neighbors, count only (the yardstick)")
            timed_row(yardstick, row)
            kernel_ms(sim, yardstick, row["calls_per_stretch"], row, "search_kernel_ms")
            if one_cell:
                row["pairs_per_s"] = round(n * (n - 1.0) / (row["search_kernel_ms_median"] * 1e-3), 0)
            emit(row)


def main(argv) -> int:
    args = list(argv)
    out, limit = ROOT / "profiles" / "pair_counts_bench.log", 900
    mode = "ab" if "--ab" in args else "all"
    if "--ab" in args:
        args.remove("--ab")
    if "--out" in args:
        out = Path(args.pop(args.index("--out") + 1))
        args.remove("--out")
    if "--limit" in args:
        limit = int(args.pop(args.index("--limit") + 1))
        args.remove("--limit")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"pair_counts_bench: the time limit of {limit} s ran out"))
    signal.alarm(limit)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as log:
        def emit(row: dict) -> None:
            line = json.dumps(row)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        lib_path = Path(nb.load()._name).resolve()
        emit({"tool": "pair_counts_bench", "library": str(lib_path.relative_to(ROOT) if ROOT in lib_path.parents else lib_path.name), "mode": mode})
        default = {"ab": ["d262144", "d1048576"], "all": ["d262144", "d1048576", "t8388608", "cell16384"]}[mode]
        for case in args or default:
            run(case, emit, mode)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
