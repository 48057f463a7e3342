"""CPU: the C++ adaptor (nbodysim_amd/host/Simulation.hpp) compiles on its own.

The drop-in claim of SURVEY §8(b) itself — the reference's UNMODIFIED main.cpp passes `g++ -std=c++20 -fsyntax-only`
with nbodysim_amd/host first on the include path — needs the reference tree, which is not part of this repository;
INTEGRATION.md §2 gives the command that checks it where that tree is at hand.  What needs nothing outside the
repository is checked here: without the reference's headers the adaptor declares layout-identical minimal types."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_adaptor_stands_alone_without_the_reference_headers(tmp_path):
    """Without the reference on the include path the adaptor declares layout-identical minimal types."""
    src = ROOT / "nbodysim_amd" / "host" / "sim_thread_example.cpp"
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
