"""Cost and energy error of NB_INTEGRATOR_HERMITE4 beside kick-drift, DKD and FR4 on one GPU, from one process.

    python tools/hermite_bench.py [--rounds R] [--energy-only | --time-only] [handle ...]

    handles: headline (262 144 bodies, fp32 2-D, the benchmark's eps and dt), fp64 (its fp64 twin); both by default

Time.  Per handle the four integrators and a one-sided twin (NB_FLAG_NO_SYMMETRY | NB_FLAG_NO_UNIFORM_MASS, kick-drift: the
individual-mass one-sided force launch) are opened side by side on the same bodies.  Each first steps for at least 2 s (settled
clocks, as tools/integrator_bench.py), then R rounds (default 5) visit them in turn and time a stretch of about 1 s of steps between
two waits.  In every round the Hermite handle and the twin also run a stretch with nb_profile_enable: the device events around their
force launches give the time of ONE acc+jerk launch and ONE one-sided force launch.  One JSON line per (handle, integrator): the R
figures in ms per step, their median and spread (max - min); one line per handle with the kernel times and their ratio.

Energy (fp64 handle).  |E(T) - E(0)| / |E(0)| over T = 96 h for h = 1e-3 and 4e-3 at EQUAL WALL TIME: Hermite takes 96 steps of h;
DKD and FR4 take as many equal steps over the same T as fit into the time the 96 Hermite steps took (from the medians measured
above, or --costs HERMITE,DKD,FR4 in ms with --energy-only).  nb_energy is the fp64 pair sweep.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import nbodysim_amd as nb  # noqa: E402
from integrator_bench import stats_of  # noqa: E402
from tree_bench import settle  # noqa: E402

EPS, DT, SEED, N = 0.01, 1e-3, 42, 262144
HANDLES = {"headline": dict(eps=EPS), "fp64": dict(eps=EPS, precision="fp64")}
INTEGRATORS = ("kick_drift", "dkd", "fr4", "hermite4")
TWIN = "one_sided_twin"


def times(handle: str, rounds: int, timed_s: float = 1.0) -> dict:
    kw = HANDLES[handle]
    bodies = nb.plummer_2d(N, SEED)
    sims, steps = {}, {}
    ms = {k: [] for k in INTEGRATORS + (TWIN,)}
    kernel = {"hermite4": [], TWIN: []}
    try:
        for k in INTEGRATORS:
            sims[k] = nb.Simulation(bodies, integrator=k, device=0, **kw)
        sims[TWIN] = nb.Simulation(bodies, device=0, symmetry=False, uniform_mass=False, **kw)
        for k, sim in sims.items():
            est = settle(sim, DT)
            steps[k] = max(3, min(int(timed_s / est), 5000))
        for _ in range(rounds):
            for k, sim in sims.items():
                t0 = time.perf_counter()
                sim.advance(steps[k], DT)
                sim.wait()
                ms[k].append((time.perf_counter() - t0) / steps[k] * 1e3)
            for k in kernel:                                   # device events around the force launches of a short stretch
                sims[k].profile(True)
                sims[k].advance(max(3, steps[k] // 4), DT)
                t, cnt = sims[k].profile_read()
                sims[k].profile(False)
                kernel[k].append(t / cnt)
        med = {}
        for k in sims:
            row = {"handle": handle, "n": N, "integrator": k, "steps_per_stretch": steps[k]}
            stats_of("step_ms", ms[k], row)
            if k in kernel:
                stats_of("force_launch_ms", kernel[k], row)
            med[k] = row["step_ms_median"]
            print(json.dumps(row), flush=True)
        kh, kt = sorted(kernel["hermite4"])[rounds // 2], sorted(kernel[TWIN])[rounds // 2]
        print(json.dumps({"handle": handle, "acc_jerk_launch_ms": round(kh, 4), "one_sided_force_launch_ms": round(kt, 4),
                          "ratio": round(kh / kt, 3), "hermite_over_kick_drift": round(med["hermite4"] / med["kick_drift"], 3),
                          "hermite_over_fr4": round(med["hermite4"] / med["fr4"], 3), "describe": sims["hermite4"].describe()}), flush=True)
        return med
    finally:
        for s in sims.values():
            s.close()


def energies(cost: dict, steps_hermite: int = 96) -> None:
    """cost: ms per step of hermite4, dkd and fr4 on the fp64 handle."""
    bodies = nb.plummer_2d(N, SEED)
    for h in (1e-3, 4e-3):
        total = steps_hermite * h
        for k in ("hermite4", "dkd", "fr4"):
            steps = steps_hermite if k == "hermite4" else max(1, int(steps_hermite * cost["hermite4"] / cost[k]))
            with nb.Simulation(bodies, integrator=k, device=0, **HANDLES["fp64"]) as sim:
                e0 = sum(sim.energy())
                t0 = time.perf_counter()
                sim.advance(steps, total / steps)
                sim.wait()
                wall = time.perf_counter() - t0
                e1 = sum(sim.energy())
            print(json.dumps({"handle": "fp64", "n": N, "integrator": k, "h": total / steps, "steps": steps, "T": total,
                              "wall_ms": round(wall * 1e3, 1), "E0": e0, "E1": e1, "rel_dE": float(f"{abs(e1 - e0) / abs(e0):.3e}")}), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    rounds, cost = 5, None
    if "--rounds" in args:
        rounds = int(args.pop(args.index("--rounds") + 1))
        args.remove("--rounds")
    if "--costs" in args:
        c = [float(v) for v in args.pop(args.index("--costs") + 1).split(",")]
        args.remove("--costs")
        cost = dict(zip(("hermite4", "dkd", "fr4"), c))
    do_time, do_energy = "--energy-only" not in args, "--time-only" not in args
    names = [a for a in args if not a.startswith("--")] or list(HANDLES)
    for name in names:
        if do_time:
            med = times(name, rounds)
            if name == "fp64":
                cost = med
    if do_energy:
        if cost is None:
            sys.exit("the energy table needs the fp64 step costs: run the fp64 handle's timing, or give --costs HERMITE,DKD,FR4")
        energies(cost)
