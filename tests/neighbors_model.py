"""The numpy statement of nb_neighbors' contract (include/nbody.h): brute force over all pairs in float32, one rounding per operation
(numpy does not fuse), the strict comparison, the self term left out by index, and the rows in the order of the packed 64-bit integer
``(bits(d2) << 32) | j``.  No grid, no sort by cell: what the device does to be fast is not repeated here."""
import numpy as np

NO_NEIGHBOR = np.uint32(0xFFFFFFFF)
INF_BITS = np.uint64(0x7F800000)
EMPTY = (INF_BITS << np.uint64(32)) | np.uint64(0xFFFFFFFF)        # +inf, NB_NO_NEIGHBOR: above every neighbour's packed key


def neighbors(x, y, radius, k, rows=None, chunk=256):
    """(idx, dist2, count) of the bodies ``rows`` (default all) among all bodies (x, y): idx uint32 (len(rows), k), dist2 float32 of the
    same shape, count uint32 (len(rows),).  ``radius`` is rounded to float32 first, as the C argument is."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    n = x.size
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    r = np.float32(radius)
    r2 = r * r
    assert r2.dtype == np.float32
    idx = np.full((rows.size, k), NO_NEIGHBOR, np.uint32)
    dist2 = np.full((rows.size, k), np.inf, np.float32)
    count = np.zeros(rows.size, np.uint32)
    j = np.arange(n, dtype=np.uint64)
    kk = min(k, n)
    for at in range(0, rows.size, chunk):
        i = rows[at:at + chunk]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            dx = x[None, :] - x[i, None]
            dy = y[None, :] - y[i, None]
            d2 = dx * dx + dy * dy
            near = d2 < r2                                        # false on NaN; an infinite d2 fails it too
        assert d2.dtype == np.float32
        near[np.arange(i.size), i] = False                        # j != i, by index
        count[at:at + chunk] = near.sum(axis=1)
        packed = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j[None, :]
        packed[~near] = EMPTY
        if kk < n:
            packed = np.partition(packed, kk - 1, axis=1)[:, :kk]
        packed = np.sort(packed, axis=1)
        idx[at:at + chunk, :kk] = (packed & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        dist2[at:at + chunk, :kk] = (packed >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, dist2, count


def lattice(lo=-8, hi=8):
    """The integer lattice [lo, hi)^2 as float32 (x, y), row-major in y: every d2 on it is an exact small integer."""
    gx, gy = np.meshgrid(np.arange(lo, hi), np.arange(lo, hi))
    return gx.ravel().astype(np.float32), gy.ravel().astype(np.float32)
