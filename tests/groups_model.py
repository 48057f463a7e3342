"""The numpy statement of nb_groups' contract (include/nbody.h): the link matrix is brute force over all pairs with
tests/neighbors_model.py's arithmetic (the same float32 expressions, one rounding per operation, the strict comparison, the self term
left out by index); the groups are its connected components; a label is the smallest index of its component.  No grid, no sort, no
union-find order: what the device does to be fast is not repeated here."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def links(x, y, radius, chunk=512):
    """(i, j) index arrays of every ordered linked pair, i != j, among the bodies (x, y).  ``radius`` is rounded to float32 first."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    n = x.size
    r = np.float32(radius)
    r2 = r * r
    assert r2.dtype == np.float32
    out_i, out_j = [], []
    for at in range(0, n, chunk):
        i = np.arange(at, min(at + chunk, n))
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            dx = x[None, :] - x[i, None]
            dy = y[None, :] - y[i, None]
            dx *= dx                                              # (in place: the same float32 roundings, fewer temporaries)
            dy *= dy
            dx += dy
            d2 = dx
            near = d2 < r2                                        # false on NaN; an infinite d2 fails it too
        assert d2.dtype == np.float32
        near[np.arange(i.size), i] = False                        # j != i, by index
        a, b = np.nonzero(near)
        out_i.append(a + at)
        out_j.append(b)
    return np.concatenate(out_i), np.concatenate(out_j)


def link_matrix(x, y, radius):
    """The dense boolean link matrix (small n only)."""
    n = len(x)
    i, j = links(x, y, radius)
    m = np.zeros((n, n), bool)
    m[i, j] = True
    return m


def groups(x, y, radius, rows=None):
    """(label, size, ngroups): uint32 label and size of the bodies ``rows`` (default all) and the number of groups among all bodies."""
    n = len(x)
    i, j = links(x, y, radius)
    graph = coo_matrix((np.ones(i.size, np.uint8), (i, j)), shape=(n, n))
    ncomp, comp = connected_components(graph, directed=False)
    smallest = np.full(ncomp, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))                   # canonical: the minimum index per component
    label = smallest[comp].astype(np.uint32)
    size = np.bincount(comp, minlength=ncomp)[comp].astype(np.uint32)
    assert int((label == np.arange(n)).sum()) == ncomp
    if rows is not None:
        label, size = label[rows], size[rows]
    return label, size, int(ncomp)
