"""Cost of the collision pass (NB_EXTRA_COLLIDE) per step, on one GPU: the same state stepped with and without the bit.

    python tools/collide_bench.py ref       the reference's start (nb_default_ics(25000), eps 1, dt 0.01, clamp + boundary),
                                            after the first contacts
    python tools/collide_bench.py sparse    262 144 bodies, uniform in a 2000 x 2000 square, radius 0.12, velocities N(0, 50)
                                            per component: a body moves 0.5 per step, more than a disc's diameter, so the
                                            overlaps are new every step and about 1 % of the bodies are in contact in every
                                            step (at rest the first resolution would separate them for good)
Prints one JSON line per case: microseconds per step with and without collisions, pairs and rounds per step, and the
bodies in contact (2 x pairs / n: exact when no body is in two pairs, an upper bound otherwise).  Under
`rocprofv3 --kernel-trace --stats` the collide_* kernels' own times appear in the stats file.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import nbodysim_amd as nb  # noqa: E402


def sparse_bodies(n: int = 262144, side: float = 2000.0, radius: float = 0.12, speed: float = 50.0) -> np.ndarray:
    rng = np.random.default_rng(5)
    b = nb.bodies_array(n)
    b["pos"][:, 0], b["pos"][:, 1] = rng.uniform(-side / 2, side / 2, (2, n)).astype(np.float32)
    b["vel"][:, 0], b["vel"][:, 1] = rng.normal(0, speed, (2, n)).astype(np.float32)
    b["mass"] = 1.0 / n
    b["radius"] = radius
    return b


def timed(sim, steps: int, dt: float) -> float:
    sim.wait()
    t0 = time.perf_counter()
    sim.advance(steps, dt)
    sim.wait()
    return (time.perf_counter() - t0) / steps * 1e6


def run(case: str, steps: int = 200) -> dict:
    if case == "ref":
        bodies, kw, dt, pre = nb.default_ics(25000), dict(eps=1.0, extras=3), 0.01, 100
    else:
        bodies, kw, dt, pre = sparse_bodies(), dict(eps=1.0), 0.01, 2
    with nb.Simulation(bodies, collide=True, device=0, **kw) as on:
        on.advance(pre, dt)                                  # past the first contacts
        state = on.sync().copy()
        with nb.Simulation(state, device=0, **kw) as off:
            timed(off, 20, dt)
            us_off = timed(off, steps, dt)
        timed(on, 20, dt)
        before = on.collision_stats()
        us_on = timed(on, steps, dt)
        after = on.collision_stats()
        rounds = after["rounds_last_step"]
        resolve = on.describe().rsplit("resolve=", 1)[1].split()[0]
    return {"case": case, "n": int(bodies.shape[0]), "steps": steps, "us_per_step_off": round(us_off, 2), "us_per_step_on": round(us_on, 2),
            "added_us_per_step": round(us_on - us_off, 2),
            "pairs_per_step": round((after["pairs_total"] - before["pairs_total"]) / (steps + 0.0), 1),
            "contact_pct": round(200.0 * (after["pairs_total"] - before["pairs_total"]) / steps / bodies.shape[0], 3),
            "pairs_last_step": after["pairs_last_step"], "rounds_last_step": rounds, "resolve": resolve}


if __name__ == "__main__":
    for c in sys.argv[1:] or ["ref", "sparse"]:
        print(json.dumps(run(c)), flush=True)
