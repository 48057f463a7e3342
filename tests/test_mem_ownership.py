"""CPU: device and page-locked memory has one owner (nbodysim_amd/csrc/nb_mem.h).  The pool itself runs under the sanitizers
(tests/test_sanitizers.py, the pool section of nb_fuzz.cpp); this is the rule that keeps every other allocation out of the sources."""
import re

from conftest import ROOT


def test_only_the_pool_and_the_host_allocator_call_the_hip_allocators():
    """Device and page-locked memory has one owner (nbodysim_amd/csrc/nb_mem.h): under csrc/ the four HIP allocation calls occur in
    the pool's HIP backend (HipMem, nb_sim.hip.h) and in nb_host_alloc / nb_host_free (caller-visible blocks with a registry of their own), nowhere else."""
    tokens = ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(")
    seen = {}
    for p in sorted((ROOT / "nbodysim_amd" / "csrc").iterdir()):
        if not p.is_file():
            continue
        txt = p.read_text(errors="ignore")
        if p.name == "nb_capi.hip":                         # the two entry points' bodies go: `extern "C" ... nb_host_x(...)\n{ ... \n}\n`
            for fn in ("nb_host_alloc", "nb_host_free"):
                m = re.search(r'^extern "C" [^\n]*\b%s\([^\n]*\)\n\{\n.*?^\}\n' % fn, txt, re.S | re.M)
                assert m, fn
                seen[fn] = [tok for tok in tokens if tok in m.group(0)]
                txt = txt.replace(m.group(0), "")
        if p.name == "nb_sim.hip.h":                        # the pool's backend: `struct HipMem {\n ... \n};\n`, one call of each
            m = re.search(r"^struct HipMem \{\n.*?^\};\n", txt, re.S | re.M)
            assert m and all(m.group(0).count(tok) == 1 for tok in tokens), "the pool's HIP backend"
            txt = txt.replace(m.group(0), "")
        hits = [tok for tok in tokens if tok in txt]
        assert not hits, f"{p.name} calls {hits} itself"
    assert seen == {"nb_host_alloc": ["hipHostMalloc("], "nb_host_free": ["hipHostFree("]}
