"""Write the fixtures of nb_tree_nodes from the compiled reference: tests/golden/node_layout.json (sizeof, alignof and the field
offsets of its `Node`), tests/golden/ref_tree_nodes_random_333.npy (the fields of `quadtree.nodes` after Quadtree::build on
tests/golden/ic_random_333.npy: pos, mass, center, size, children, next, depth) and tests/golden/tree_nodes_manifest.json (the
commands and checksums).

    python tools/make_tree_nodes_golden.py --reference <checkout of 7IBBE77S/nbodysim> [--cxx g++] [--work DIR]

tools/ref_tree_nodes.cpp is compiled against the reference's headers by include path into the work directory (outside the
repository by default: a temporary directory); only the recorded data is written into the repository.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import subprocess
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
FLAGS = ["-std=c++20", "-O2", "-msse4.1", "-ffp-contract=off", "-include", "bit", "-include", "cstdint", "-w"]
ROW = np.dtype([("pos", "<f4", 2), ("mass", "<f4"), ("center", "<f4", 2), ("size", "<f4"), ("children", "<u8"), ("next", "<u8"),
                ("depth", "<u8")])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Nbodysim/)")
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    work = Path(a.work) if a.work else Path(tempfile.mkdtemp(prefix="ref_tree_nodes_"))
    work.mkdir(parents=True, exist_ok=True)
    exe = work / "ref_tree_nodes"
    cmd = [a.cxx, *FLAGS, f"-I{Path(a.reference) / 'Nbodysim' / 'headers'}", str(ROOT / "tools" / "ref_tree_nodes.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    layout = json.loads(subprocess.run([str(exe), "--layout"], check=True, capture_output=True, text=True).stdout)
    (GOLD / "node_layout.json").write_text(json.dumps(layout, indent=1) + "\n")
    ic = np.load(GOLD / "ic_random_333.npy").astype(np.float32)
    np.ascontiguousarray(ic[:, [0, 1, 6]], "<f4").tofile(work / "in.bin")
    subprocess.run([str(exe), str(work / "in.bin"), str(work / "out.bin")], check=True)
    rows = np.fromfile(work / "out.bin", ROW)
    assert rows.dtype.itemsize == 48
    np.save(GOLD / "ref_tree_nodes_random_333.npy", rows)
    version = subprocess.run([a.cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    manifest = {
        "generator": "tools/make_tree_nodes_golden.py (harness: tools/ref_tree_nodes.cpp)",
        "reference": "7IBBE77S/nbodysim (headers included by path, unmodified)",
        "command": " ".join([a.cxx, *FLAGS, "-I<reference>/Nbodysim/headers", "tools/ref_tree_nodes.cpp", "-o", "ref_tree_nodes"]),
        "compiler": version,
        "input": "tests/golden/ic_random_333.npy, columns x, y, mass; Quadtree(1.0f, 1.0f, n).build(bodies)",
        "fields": list(ROW.names),
        "nodes": int(rows.shape[0]),
        "max_depth": int(rows["depth"].max()),
        "sha256": {"node_layout.json": hashlib.sha256((GOLD / "node_layout.json").read_bytes()).hexdigest(),
                   "ref_tree_nodes_random_333.npy": hashlib.sha256((GOLD / "ref_tree_nodes_random_333.npy").read_bytes()).hexdigest()},
    }
    (GOLD / "tree_nodes_manifest.json").write_text(json.dumps(manifest, indent=1) + "\n")
    print(json.dumps(manifest, indent=1))


if __name__ == "__main__":
    main()
