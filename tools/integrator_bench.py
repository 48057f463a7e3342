"""Cost and energy error of the four integrators (kick-drift, KDK, DKD, FR4) on one GPU, from one process.

    python tools/integrator_bench.py [--rounds R] [--energy-only | --time-only] [handle ...]

    handles: headline (262 144 bodies, fp32, the benchmark's eps and dt), fp64 (its fp64 twin), tree (1 048 576 bodies,
             NB_FORCE_TREE with NB_FLAG_TREE_LEAVES, theta 0.5); all by default

Time.  Per handle the integrators it takes (KDK: the direct handles only) are opened side by side.  Each first steps for at least
2 s (settled clocks, as tools/tree_bench.py), then R rounds (default 5) visit them in turn and time a stretch of about 1 s of steps
between two waits, so that a change of the machine's state reaches all of them alike.  One JSON line per (handle, integrator): the
R figures in ms per step, their median and spread (max - min), and the profiled force launches per step.  Then one line per
handle with the differences the launch counts predict something about: DKD - kick-drift (one pass over positions and velocities),
DKD - KDK, FR4 / kick-drift.

Energy.  |E(T) - E(0)| / |E(0)| after T = 96 h at EQUAL FORCE EVALUATIONS: kick-drift, KDK and DKD take 96 steps of h, FR4 takes
32 steps of 3 h; for h = 1e-3 and 4e-3.  nb_energy is read on the fp64 handle (the fp64 pair sweep) and on the tree handle opened
with NB_FLAG_TREE_ENERGY (its O(n log n) walk).  One JSON line per (handle, integrator, h).

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/integrator_bench.py --trace HANDLE
                                               50 DKD steps alone: the stats file holds the time of the lone `drift` kernel
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import nbodysim_amd as nb  # noqa: E402
from tree_bench import settle  # noqa: E402

EPS, DT, SEED = 0.01, 1e-3, 42
HANDLES = {
    "headline": (262144, dict(eps=EPS), ("kick_drift", "kdk", "dkd", "fr4")),
    "fp64": (262144, dict(eps=EPS, precision="fp64"), ("kick_drift", "kdk", "dkd", "fr4")),
    "tree": (1048576, dict(eps=EPS, force="tree", theta=0.5, tree_leaves=True), ("kick_drift", "dkd", "fr4")),
}


def stats_of(name: str, v, out: dict) -> None:
    out[name] = [round(a, 4) for a in v]
    out[name + "_median"] = round(sorted(v)[len(v) // 2], 4)
    out[name + "_spread"] = round(max(v) - min(v), 4)


def times(handle: str, rounds: int, timed_s: float = 1.0) -> None:
    n, kw, integrators = HANDLES[handle]
    bodies = nb.plummer_2d(n, SEED)
    sims, steps, ms, launches = {}, {}, {k: [] for k in integrators}, {}
    try:
        for k in integrators:
            sims[k] = nb.Simulation(bodies, integrator=k, device=0, **kw)
            est = settle(sims[k], DT)
            steps[k] = max(3, min(int(timed_s / est), 5000))
        for _ in range(rounds):
            for k in integrators:
                t0 = time.perf_counter()
                sims[k].advance(steps[k], DT)
                sims[k].wait()
                ms[k].append((time.perf_counter() - t0) / steps[k] * 1e3)
        for k in integrators:
            sims[k].profile(True)
            sims[k].advance(4, DT)
            launches[k] = sims[k].profile_read()[1] / 4
            sims[k].profile(False)
        rows = {}
        for k in integrators:
            rows[k] = {"handle": handle, "n": n, "integrator": k, "steps_per_stretch": steps[k], "force_launches_per_step": launches[k]}
            stats_of("step_ms", ms[k], rows[k])
            print(json.dumps(rows[k]), flush=True)
        med = {k: rows[k]["step_ms_median"] for k in integrators}
        spread = {k: rows[k]["step_ms_spread"] for k in integrators}
        out = {"handle": handle, "dkd_minus_kick_drift_ms": round(med["dkd"] - med["kick_drift"], 4),
               "fr4_over_kick_drift": round(med["fr4"] / med["kick_drift"], 3), "describe": sims["dkd"].describe()}
        if "kdk" in med:
            out["dkd_minus_kdk_ms"] = round(med["dkd"] - med["kdk"], 4)
            out["spread_of_the_two_ms"] = round(max(spread["dkd"], spread["kdk"]), 4)
            out["dkd_not_slower_than_kdk"] = bool(med["dkd"] - med["kdk"] <= max(spread["dkd"], spread["kdk"]))
        print(json.dumps(out), flush=True)
    finally:
        for s in sims.values():
            s.close()


def energies(handle: str, evaluations: int = 96) -> None:
    n, kw, integrators = HANDLES[handle]
    if handle == "tree":
        kw = dict(kw, tree_energy=True)
    bodies = nb.plummer_2d(n, SEED)
    for h in (1e-3, 4e-3):
        for k in integrators:
            per = 3 if k == "fr4" else 1
            with nb.Simulation(bodies, integrator=k, device=0, **kw) as sim:
                e0 = sum(sim.energy())
                sim.advance(evaluations // per, h * per)
                e1 = sum(sim.energy())
            print(json.dumps({"handle": handle, "n": n, "integrator": k, "h": h * per, "steps": evaluations // per, "T": evaluations * h,
                              "force_evaluations": evaluations, "E0": e0, "E1": e1, "rel_dE": float(f"{abs(e1 - e0) / abs(e0):.3e}")}), flush=True)


def trace(handle: str, steps: int = 50) -> None:
    n, kw, _ = HANDLES[handle]
    with nb.Simulation(nb.plummer_2d(n, SEED), integrator="dkd", device=0, **kw) as sim:
        sim.advance(steps, DT)
        sim.wait()
    print(json.dumps({"handle": handle, "traced_dkd_steps": steps}))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--trace"]:
        trace(args[1])
        sys.exit(0)
    rounds = 5
    if "--rounds" in args:
        rounds = int(args.pop(args.index("--rounds") + 1))
        args.remove("--rounds")
    do_time, do_energy = "--energy-only" not in args, "--time-only" not in args
    names = [a for a in args if not a.startswith("--")] or list(HANDLES)
    for name in names:
        if do_time:
            times(name, rounds)
        if do_energy and name != "headline":
            energies(name)
