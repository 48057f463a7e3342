"""CPU: the two flag bits and the entry point of the body order are declared alike in include/nbody.h and the binding, and
tools/body_order_ab.py's host-side Morton order (the model the GPU tests' ceiling measurement used) is a stable permutation."""
import ctypes as C
import importlib.util
import re

import numpy as np

from conftest import ROOT

import nbodysim_amd as nb
from nbodysim_amd import _lib as L

HEADER = (ROOT / "include" / "nbody.h").read_text()


def test_header_and_binding_agree_on_the_body_order_bits():
    assert re.search(r"NB_FLAG_BODY_ORDER\s*=\s*131072\b", HEADER) and L.NB_FLAG_BODY_ORDER == 131072
    assert re.search(r"NB_FLAG_NO_BODY_ORDER\s*=\s*262144\b", HEADER) and L.NB_FLAG_NO_BODY_ORDER == 262144
    known = HEADER.split("enum { NB_FLAGS_KNOWN", 1)[1].split("};", 1)[0]
    assert "NB_FLAG_BODY_ORDER" in known and "NB_FLAG_NO_BODY_ORDER" in known
    assert re.search(r"^int nb_body_order\(nb_sim \*s, uint32_t every, uint32_t \*perm_out, uint32_t \*every_out\);$", HEADER, re.M)
    assert "#define NB_ABI_VERSION 8" in HEADER                       # additive: no ABI bump
    lib = nb.load()
    assert lib.nb_body_order(None, 0, None, None) == L.NB_EINVAL


def test_the_new_bits_pass_the_flag_check_and_unknown_ones_do_not():
    lib = nb.load()
    b = nb.plummer_2d(16, 1)
    for flags, known in ((L.NB_FLAG_BODY_ORDER, True), (L.NB_FLAG_NO_BODY_ORDER, True), (L.NB_FLAG_BODY_ORDER | L.NB_FLAG_NO_BODY_ORDER, True),
                         (524288, False), (65536, False)):
        p = L.default_params()
        p.flags = flags
        h = lib.nb_create(b.ctypes.data, 16, C.byref(p))
        if h:                                                         # a GPU is visible
            lib.nb_destroy(h)
        else:
            assert (b"unknown bits" in lib.nb_last_error()) == (not known), (flags, lib.nb_last_error())


def test_the_measurement_tools_host_order_is_a_stable_permutation():
    spec = importlib.util.spec_from_file_location("body_order_ab", ROOT / "tools" / "body_order_ab.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pos = nb.plummer_2d(5000, 2)["pos"]
    order = mod.morton_order(pos)
    assert np.array_equal(np.sort(order), np.arange(5000))
    same = np.zeros((100, 2), np.float32)
    assert np.array_equal(mod.morton_order(same), np.arange(100))     # a degenerate box: ties by index
    assert np.array_equal(mod.morton_order(pos * np.float32(4.0)), order)   # covariant under a power-of-two scaling
