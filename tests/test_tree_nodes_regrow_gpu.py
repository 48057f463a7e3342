"""GPU: nb_tree_nodes when the tree outgrows the scratch of an earlier export (the helpers are those of tests/test_tree_nodes_gpu.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

from nbodysim_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_tree_nodes_gpu import assert_same_bytes, bodies_of, flat_xym, model_nodes, tree_sim  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_export_scratch_regrows_for_a_larger_tree():
    """The device scratch and the page-locked staging buffer of nb_tree_nodes are sized by the first export (count + count / 8 + 1024
    nodes) and released and allocated anew by an export of a larger tree; a third export of the same state regrows nothing."""
    n = 1024
    two = flat_xym(np.arange(n) % 2, np.arange(n) % 2, np.full(n, 1.0 / n))         # all bodies on (0, 0) and (1, 1), alternately
    rng = np.random.default_rng(2)
    xy = rng.random((n, 2), dtype=np.float32)
    spread = flat_xym(xy[:, 0], xy[:, 1], np.full(n, 1.0 / n))
    want, _ = model_nodes(spread[:, 0], spread[:, 1], spread[:, 6])
    with tree_sim(bodies_of(two), eps=0.05) as sim:
        sim.advance(1, 1e-3)
        first = sim.tree_nodes(out=np.zeros(16, L.NODE_DTYPE))                      # a pageable destination: staged
        count1 = first.shape[0]
        assert count1 == 5
        sim.upload(bodies_of(spread))
        sim.advance(1, 1e-3)                                                        # the tree of the uploaded positions (built before the drift)
        second = sim.tree_nodes(out=np.zeros(want.shape[0] + 8, L.NODE_DTYPE))
        count2 = second.shape[0]
        print(f"export scratch: {count1} nodes, then {count2}")
        assert count2 > count1 + count1 // 8 + 1024                                 # past the scratch of the first export: both buffers regrow
        assert_same_bytes(second, want, "after the scratch grew")
        third = sim.tree_nodes(out=np.zeros(want.shape[0] + 8, L.NODE_DTYPE))
        assert_same_bytes(third, want, "the same state again")
