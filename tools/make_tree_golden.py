"""Write the Barnes-Hut fixtures tests/golden/tree_default_s{1,5}_first4096.npy and tests/golden/tree_manifest.json from the
reference's own step().

The reference's 25 000 default bodies (nb_default_ics, bit-identical to its constructor's) with every radius set to 0 are
stepped 1 and 5 times by the compiled reference (oracle/_ref/libnbref.so: Simulation::step() = Barnes-Hut attract, kick,
velocity clamp, soft boundary, drift, collide(); eps = 1, dt = 0.01).  Radius 0 keeps collide() out: resolve() returns at
once for two bodies at different positions, and no two of the 25 000 coincide at any of the recorded frames (checked here).
A committed file stays small: the first 4 096 rows of (x, y, vx, vy, ax, ay, m, r) are stored, and the sha256 of the full
float32 array goes into the manifest; the tests compare both.

    python tools/make_tree_golden.py      (needs the reference built: `make -C oracle ref`)
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT))

N, ROWS, EPS, DT = 25000, 4096, 1.0, 0.01


def main() -> None:
    import nbo
    import nbodysim_amd as nb

    b = nb.default_ics(N)
    ic = np.zeros((N, 8), np.float32)
    ic[:, 0:2], ic[:, 2:4], ic[:, 6] = b["pos"], b["vel"], b["mass"]          # acc 0, radius 0
    out = ROOT / "tests" / "golden"
    manifest = {"n": N, "rows": ROWS, "eps": EPS, "dt": DT, "ic": "nb_default_ics(25000) with radius = 0", "steps": {}}
    for steps in (1, 5):
        f = np.ascontiguousarray(ic.copy())
        assert nbo.ref().ref_step(f.reshape(-1), N, EPS, DT, steps) == steps
        assert np.unique(f[:, 0:2], axis=0).shape[0] == N, "two bodies coincide: collide() may have acted"
        name = f"tree_default_s{steps}_first{ROWS}.npy"
        np.save(out / name, f[:ROWS])
        manifest["steps"][str(steps)] = {"file": name, "sha256_float32_le": hashlib.sha256(f.astype("<f4").tobytes()).hexdigest()}
    (out / "tree_manifest.json").write_text(json.dumps(manifest, indent=1) + "\n")
    print(json.dumps(manifest, indent=1))


if __name__ == "__main__":
    main()
