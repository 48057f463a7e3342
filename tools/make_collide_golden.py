"""Write the collision fixtures tests/golden/collide_isolated_{ic,s1,s3}.npy from the reference's own step().

About 256 isolated pairs of overlapping discs (approaching, receding and resting, mass ratios 1 ... 1e3), each pair alone in
one of the reference's 600-unit cells, are stepped 1 and 3 times by the compiled reference (oracle/_ref/libnbref.so: its
Simulation::step() = iterate(dt); collide(); ++frame).  Masses are about 1e-20, so every acc * dt is below half an ulp of
the velocity; |v| < 1000 and |p| < 8e4 keep the clamp and the boundary inert; dt = 1/64 makes v * dt exact, so the drift has
the same bits with and without a fused multiply-add.  Arrays are (n, 8) float32: x, y, vx, vy, ax, ay, m, r.

    python tools/make_collide_golden.py      (needs the reference built: `make -C oracle ref`)
"""
from __future__ import annotations

import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))

EPS, DT, PAIRS, CELL = 1.0, 1.0 / 64.0, 256, 600.0


def make_ic(seed: int = 7) -> np.ndarray:
    rng = np.random.default_rng(seed)
    flat = np.zeros((2 * PAIRS, 8), np.float32)
    for k in range(PAIRS):
        cx, cy = CELL * (k % 16) + CELL / 2, CELL * (k // 16) + CELL / 2      # the centre of cell (k % 16, k // 16)
        r1, r2 = rng.uniform(2.0, 30.0, 2)
        ratio = 10.0 ** rng.uniform(0.0, 3.0)
        m1 = 1e-20 * rng.uniform(0.5, 2.0)
        m2 = m1 * ratio
        ang = rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(ang), np.sin(ang)])
        depth = rng.uniform(0.05, 0.6) * (r1 + r2)
        sep = (r1 + r2) - depth                                                 # overlap after the first drift
        kind = k % 3                                                            # 0 approaching, 1 receding, 2 resting
        base = rng.uniform(-200, 200, 2)
        rel = rng.uniform(20, 300)
        v1 = base + (rel * u / 2 if kind == 0 else -rel * u / 2 if kind == 1 else 0)
        v2 = base - (rel * u / 2 if kind == 0 else -rel * u / 2 if kind == 1 else 0)
        for v in (v1, v2):                                                      # no component below 1e-3 in magnitude
            v[np.abs(v) < 1e-3] = 1e-3 + rng.uniform(0, 1)
        q1 = np.array([cx, cy]) - u * sep / 2
        q2 = np.array([cx, cy]) + u * sep / 2
        p1, p2 = q1 - v1 * DT, q2 - v2 * DT                                     # so that the drifted pair overlaps
        if k % 2:                                                               # both index orders of the heavier body
            (p1, v1, m1, r1), (p2, v2, m2, r2) = (p2, v2, m2, r2), (p1, v1, m1, r1)
        flat[2 * k] = [p1[0], p1[1], v1[0], v1[1], 0, 0, m1, r1]
        flat[2 * k + 1] = [p2[0], p2[1], v2[0], v2[1], 0, 0, m2, r2]
    return flat


def main() -> None:
    import nbo

    ic = make_ic()
    assert np.abs(ic[:, 2:4]).max() < 1000 and np.abs(ic[:, 2:4]).min() >= 1e-3 and np.abs(ic[:, :2]).max() < 8e4
    out = ROOT / "tests" / "golden"
    np.save(out / "collide_isolated_ic.npy", ic)
    ref = nbo.ref()
    for steps in (1, 3):
        f = np.ascontiguousarray(ic.copy())
        frame = ref.ref_step(f.reshape(-1), f.shape[0], EPS, DT, steps)
        assert frame == steps
        np.save(out / f"collide_isolated_s{steps}.npy", f)
    for name in ("ic", "s1", "s3"):
        path = out / f"collide_isolated_{name}.npy"
        print(path.name, hashlib.sha256(path.read_bytes()).hexdigest())


if __name__ == "__main__":
    main()
