"""Inputs of the device text formatter tests (TEST ONLY): the cell values of
the {v:F3} rule's edges and the block shapes at the seams of the kernels' work split."""
import math
import struct

import numpy as np

THRESHOLD_BITS = 0x3F40624DD2F1A9F8  # the smallest double that prints 0.001
DBL_MAX = 1.7976931348623157e308


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _to_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def around(v, ulps):
    b = _to_bits(abs(v))
    s = -1.0 if math.copysign(1.0, v) < 0 else 1.0
    return [s * _from_bits(b + d) for d in range(-ulps, ulps + 1) if b + d >= 0]


_CELLS = None


def cell_values():
    """Every value the issue lists, in a fixed order (computed once, left unchanged)."""
    global _CELLS
    if _CELLS is not None:
        return _CELLS
    v = [_from_bits(THRESHOLD_BITS), _from_bits(THRESHOLD_BITS - 1)]
    for k in range(-4, 16):
        v += around(float("1e%d" % k), 3)
    for text in ("0.0015", "0.0025", "0.0125", "0.1235"):
        v += around(float(text), 2)
    for m in range(0, 10):
        for frac in (".2345", ".0005", ".9995"):
            v += around(float(str(12 * 10 ** m // 10) + frac), 2)
    v += [999.9995, -999.9995, 9.9995e14, 1e15 - 0.5, 1e14 + 0.5, 1e14 + 1.5]
    v += [-0.0004, -0.0, 0.0, 5e-324, 2.2250738585072014e-308]
    big = [1e15, 1e22, 1e23, 1.2345678901234568e17, 2.0 ** 63, 2.0 ** 64, 1e300, DBL_MAX]
    v += big + [-x for x in big]
    v += [float("nan"), float("inf"), float("-inf")]
    _CELLS = v
    return v


def cell_tableaux():
    """cell_values() as 1 x 1 .. 1 x 8 tableaux, widths in turn."""
    vals, out, at, w = cell_values(), [], 0, 1
    while at < len(vals):
        out.append(np.array([vals[at:at + w]], dtype=np.float64))
        at += w
        w = w % 8 + 1
    return out


def random_bits_tableau(seed=20, rows=400, cols=500):
    """rows x cols random 64-bit patterns: all exponents, both signs."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 64, size=(rows, cols), dtype=np.uint64).view(np.float64)


def _mixed(rng, rows, cols):
    """Cells of varied lengths: magnitudes 1e-4 .. 1e7, some zeros, both signs."""
    T = rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-4, 8, size=(rows, cols))
    T[rng.random((rows, cols)) < 0.2] = 0.0
    return T


_SEAMS = None


def seam_blocks():
    """(tableau, nvars) pairs; 1 x 1 blocks in between so that offsets cross every boundary."""
    global _SEAMS
    if _SEAMS is not None:
        return _SEAMS
    rng = np.random.default_rng(25)
    out = []
    one = lambda: (np.array([[rng.standard_normal()]]), int(rng.integers(0, 3)))
    for cols in (1, 2, 63, 64, 65, 255, 256, 257, 1025):
        out += [(_mixed(rng, 3, cols), max(cols - 2, 0)), one()]
    for rows in (1, 2, 10, 11, 100, 101):
        out += [(_mixed(rng, rows, 5), 2), one()]
    cols = 12
    for nv in (0, 1, 9, 10, 99, 100, cols - 1, cols, cols + 3):
        out += [(_mixed(rng, 2, cols), nv), one()]
    for at in (0, 65, 129, 63, 64):  # one 314-byte cell in a row of short ones
        T = np.round(_mixed(rng, 3, 130), 0) % 10
        T[1, at] = -DBL_MAX
        out += [(T, 100), one()]
    T = np.zeros((5, 9))  # 4 rows per wave at 16 lanes: rows on both sides of a wave
    T[:, 8] = [DBL_MAX, -1e15, 1e22, float("nan"), float("-inf")]
    out.append((T, 3))
    _SEAMS = out
    return out
