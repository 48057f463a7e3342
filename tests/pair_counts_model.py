"""The numpy statement of nb_pair_counts' contract (include/nbody.h): brute force over all pairs in float32, one rounding per operation
(numpy does not fuse), every unordered pair once, binned between the float32 squares of the edges, closed below and open above.  No
grid, no sort by cell, no cumulative counters: what the device does to be fast is not repeated here."""
import numpy as np


def pair_counts(x, y, edges, rows=None, chunk=256):
    """counts uint64 (nbins,) of the unordered pairs {i, j} of the bodies (x, y) whose LOWER index is in ``rows`` (default all).
    ``edges`` are rounded to float32 first, as the C argument is, and squared in float32."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    n = x.size
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    e = np.asarray(edges, np.float32)
    e2 = e * e
    assert e2.dtype == np.float32 and e2.size >= 2 and (np.diff(e2) > 0).all() and e2[0] >= 0
    counts = np.zeros(e2.size - 1, np.uint64)
    j = np.arange(n)
    for at in range(0, rows.size, chunk):
        i = rows[at:at + chunk]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            dx = x[None, :] - x[i, None]
            dy = y[None, :] - y[i, None]
            d2 = dx * dx + dy * dy
        assert d2.dtype == np.float32
        mine = j[None, :] > i[:, None]                            # i is the lower index of the pair
        d = d2[mine]
        d = d[d < e2[-1]]                                         # drops NaN and +inf with everything at or beyond r2max
        b = np.searchsorted(e2, d, side="right") - 1              # e2[b] <= d < e2[b + 1]; -1 below e2[0]
        counts += np.bincount(b[b >= 0], minlength=counts.size).astype(np.uint64)
    return counts
