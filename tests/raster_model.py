"""numpy restatement of nb_raster's contract (include/nbody.h): the pixel arithmetic in float32 with one rounding per operation,
np.bincount for the counts, the mass in whole quanta (np.rint on float32, ties to even, saturated) summed as integers, and the final
float32(float64(U) * float64(q)).  Nothing here depends on the order of the bodies."""
import numpy as np

F = np.float32


def pixels(x, y, width: int, height: int, center=(0.0, 0.0), scale=1.0):
    """(inside, pixel index) per body: sx = (x - cx) * scale + width * 0.5f, inside tested before any conversion."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (x - F(center[0])) * F(scale) + F(width) * F(0.5)
        sy = (y - F(center[1])) * F(scale) + F(height) * F(0.5)
        assert sx.dtype == F and sy.dtype == F
        inside = (sx >= F(0)) & (sx < F(width)) & (sy >= F(0)) & (sy < F(height))       # NaN fails every comparison
    px = np.zeros(x.shape, np.int64)
    px[inside] = sy[inside].astype(np.int64) * width + sx[inside].astype(np.int64)          # truncation of values in [0, 16384)
    return inside, px


def units(m, quantum) -> np.ndarray:
    """Whole quanta per body as uint64: 0 for !(m > 0), else rint(m / q) in float32, 2^32 - 1 from 2^32 up."""
    m = np.asarray(m, F)
    u = np.zeros(m.shape, np.uint64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pos = m > F(0)                                                                   # False for NaN
        r = m[pos] / F(quantum)
        assert r.dtype == F
        big = r >= F(4294967296.0)
        ur = np.full(r.shape, 4294967295, np.uint64)
        ur[~big] = np.rint(r[~big]).astype(np.uint64)
    u[pos] = ur
    return u


def unit_sums(x, y, m, width, height, center=(0.0, 0.0), scale=1.0, quantum=1.0) -> np.ndarray:
    """U_p: the integer unit sum of every pixel, (height, width) uint64 (exact: Python-int free, n * 2^32 < 2^64)."""
    inside, px = pixels(x, y, width, height, center, scale)
    out = np.zeros(width * height, np.uint64)
    np.add.at(out, px[inside], units(np.asarray(m, F)[inside], quantum))
    return out.reshape(height, width)


def raster(x, y, m, width, height, center=(0.0, 0.0), scale=1.0, quantum=None):
    """(count, mass): the uint32 (height, width) count plane and, with a quantum, the float32 mass plane (else None)."""
    inside, px = pixels(x, y, width, height, center, scale)
    count = np.bincount(px[inside], minlength=width * height).astype(np.uint32).reshape(height, width)
    if quantum is None:
        return count, None
    U = unit_sums(x, y, m, width, height, center, scale, quantum)
    with np.errstate(over="ignore"):
        mass = (U.astype(np.float64) * np.float64(F(quantum))).astype(F)
    return count, mass
