"""Host-side mirror of Utilities/TableIterationFormater.cs:19-48 and of the .NET Framework
number formatting it relies on (``{v:F3}``), plus ``NumFormat.N3``
(Simplex/RevisedPrimalSimplexSolver.cs:451-466).

.NET Framework 4.7.2 formats a double with a fixed-point specifier in two steps: the value is
first converted to 15 significant decimal digits (correctly rounded), then that decimal string is
rounded half-away-from-zero to the requested number of decimals; a result that rounds to zero is
printed without a sign.  ``'%.3f'`` differs (it rounds the exact binary value half-even: 2.0005 ->
'2.000' where .NET prints '2.001'), so the two steps are restated with ``decimal``.
PARITY UNPINNED: the reference holds no formatted output to check these strings against.
"""
from __future__ import annotations

import ctypes as C
import math
from decimal import ROUND_HALF_UP, Context, Decimal
from typing import Optional, Sequence

import numpy as np

NEWLINE = "\r\n"  # Environment.NewLine on the reference's platform (Windows / .NET Framework)


def _dec15(v: float) -> Decimal:
    return Decimal("%.14e" % v)  # 15 significant digits, correctly rounded


def format_fixed(v: float, decimals: int) -> str:
    """double.ToString("F<decimals>", InvariantCulture) on .NET Framework."""
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "Infinity" if v > 0 else "-Infinity"
    q = Decimal(1).scaleb(-decimals)
    # (a context of its own: the default 28 digits cannot hold 1e300 at three decimals)
    d = _dec15(v).quantize(q, rounding=ROUND_HALF_UP, context=Context(prec=700))
    if d == 0:
        d = abs(d)  # "-0.000" never appears on .NET Framework
    return format(d, "f")


def F3(v: float) -> str:
    return format_fixed(v, 3)


def F6(v: float) -> str:
    return format_fixed(v, 6)


def dotnet_double_to_string(v: float) -> str:
    """double.ToString() on .NET Framework ("G", 15 significant digits)."""
    if v != v:
        return "NaN"
    if v in (float("inf"), float("-inf")):
        return "Infinity" if v > 0 else "-Infinity"
    s = format(v, ".15g")
    if "e" in s:
        mant, exp = s.split("e")
        sign = "+" if int(exp) >= 0 else "-"
        s = f"{mant}E{sign}{abs(int(exp)):02d}"
    return "0" if s in ("-0", "0") else s


def dotnet_round_half_even(x: float) -> float:
    """Math.Round(double) on .NET Framework (classlibnative COMDouble::Round)."""
    if math.isnan(x) or math.isinf(x):
        return x
    if abs(x) < 9.2e18 and x == float(int(x)):
        return x
    t = x + 0.5
    f = math.floor(t)
    if f == t and math.fmod(t, 2.0) != 0:
        f -= 1.0
    return math.copysign(f, x)


def dotnet_round_digits(x: float, digits: int, away_from_zero: bool = False) -> float:
    """Math.Round(double, int[, MidpointRounding]) on .NET Framework (Math.InternalRound)."""
    if math.isnan(x) or math.isinf(x):
        return x
    if abs(x) < 1e16:
        p = float(10 ** digits)
        x = x * p
        if away_from_zero:
            frac, whole = math.modf(x)
            x = whole
            if abs(frac) >= 0.5:
                x += math.copysign(1.0, frac)
        else:
            x = dotnet_round_half_even(x)
        x = x / p
    return x


def _custom_0_hashes(r: float, digits: int = 3) -> str:
    """double.ToString("0.###", InvariantCulture), or "0.####" with ``digits`` = 4: the
    15-significant-digit decimal image first, rounded half away from zero to ``digits``
    decimals, trailing zeros dropped, no "-0"; NaN and the infinities as words."""
    if math.isnan(r):
        return "NaN"
    if math.isinf(r):
        return "Infinity" if r > 0 else "-Infinity"
    d = _dec15(r).quantize(Decimal(1).scaleb(-digits), rounding=ROUND_HALF_UP,
                           context=Context(prec=700))
    neg = d < 0
    s = format(abs(d), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    if s == "":
        s = "0"
    if s == "0":
        neg = False
    return ("-" if neg else "") + s


def H3(v: float) -> str:
    """v.ToString("0.###")"""
    return _custom_0_hashes(v, 3)


def H4(v: float) -> str:
    """v.ToString("0.####") (CuttingPlaneSolver.cs:50-52, PrimalSimplexSolver2.cs:186-188)"""
    return _custom_0_hashes(v, 4)


def N3(x: float) -> str:
    """NumFormat.N3, Simplex/RevisedPrimalSimplexSolver.cs:455-465."""
    if math.isnan(x):
        return "NaN"
    if abs(x) < 1e-12:
        x = 0.0
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    r = dotnet_round_digits(x, 3, away_from_zero=True)
    rr = dotnet_round_half_even(r)
    if abs(r - rr) < 1e-12:
        # double.ToString() of an integral value ("R"-less general format, 15 digits)
        if rr == 0:
            return "0"
        if abs(rr) < 1e15:
            return str(int(rr))
        return _dotnet_g15_scientific(rr)
    return _custom_0_hashes(r)


def _dotnet_g15_scientific(v: float) -> str:
    """double.ToString() on .NET Framework for |v| >= 1e15: "G" with 15 significant digits falls
    back to scientific notation, mantissa without trailing zeros, exponent sign and at least two
    digits ("1E+15", "1.23456789012346E+17")."""
    mant, exp = f"{abs(v):.14e}".split("e")
    mant = mant.rstrip("0").rstrip(".")
    e = int(exp)
    return ("-" if v < 0 else "") + f"{mant}E{'+' if e >= 0 else '-'}{abs(e):02d}"


def Format(tab: np.ndarray, numOriginalVars: int, title: str,
           rowLabels: Optional[Sequence[str]] = None) -> str:
    """TableIterationFormater.Format, Utilities/TableIterationFormater.cs:22-48."""
    rows, cols = tab.shape
    nl = NEWLINE
    out = ["\n" + title + ":" + nl, "-" * 80 + nl, "Table\t"]
    for j in range(numOriginalVars):
        out.append(f"x{j + 1}\t")
    for j in range(numOriginalVars, cols - 1):
        out.append(f"t{j - numOriginalVars + 1}\t")
    out.append("RHS" + nl)
    out.append("Z\t")
    for j in range(cols):
        out.append(F3(float(tab[0, j])) + "\t")
    out.append(nl)
    for i in range(1, rows):
        label = rowLabels[i - 1] if (rowLabels is not None and len(rowLabels) >= i) else f"{i}"
        out.append(label + "\t")
        for j in range(cols):
            out.append(F3(float(tab[i, j])) + "\t")
        out.append(nl)
    return "".join(out)


# -- device text: the body of Format, written on the MI355X -------------

def title_line(title: str) -> str:
    """The first line of Format (:24), the part of a block that stays on the host."""
    return "\n" + title + ":" + NEWLINE


class DeviceText:
    """Blocks formatted on the device (lpr_text_*): ``block(i)`` is Format(tab, numOriginalVars,
    title) without its title line.  Owns the handle; offsets and bytes are read once."""

    def __init__(self, handle):
        from . import _native as N
        self._N = N
        self._h = handle
        blocks, nbytes, ms = C.c_int64(), C.c_int64(), C.c_double()
        N.check(N.lib.lpr_text_info(self._h, C.byref(blocks), C.byref(nbytes), C.byref(ms)),
                "lpr_text_info")
        self.Count = int(blocks.value)
        self.Bytes = int(nbytes.value)
        self.KernelMs = float(ms.value)
        self._offsets = None
        self._data = None

    def _read(self) -> None:
        N = self._N
        off = np.zeros(self.Count + 1, dtype=np.int64)
        N.check(N.lib.lpr_text_offsets_read(self._h, N._ptr(off, C.c_int64)),
                "lpr_text_offsets_read")
        data = np.zeros(max(self.Bytes, 1), dtype=np.uint8)
        N.check(N.lib.lpr_text_read(self._h, 0, self.Bytes, N._ptr(data, C.c_uint8)),
                "lpr_text_read")
        self._offsets = off
        self._data = data[:self.Bytes].tobytes()

    @property
    def offsets(self) -> np.ndarray:
        if self._offsets is None:
            self._read()
        return self._offsets

    def block(self, i: int) -> str:
        if self._data is None:
            self._read()
        if not 0 <= i < self.Count:
            raise IndexError(f"block {i} of {self.Count}")
        return self._data[int(self._offsets[i]):int(self._offsets[i + 1])].decode("ascii")

    def blocks(self):
        return [self.block(i) for i in range(self.Count)]

    def destroy(self) -> None:
        if self._h:
            self._N.lib.lpr_text_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def format_device(tableaux, nvars, engine=None, round4=0) -> DeviceText:
    """lpr_text_format_tableaux: one block per tableau (2-D arrays of any shapes), ``nvars`` an
    int for all or one per tableau.  ``round4`` (an int for all, or one per tableau; 0, 1 or 2)
    is how many times Math.Round(v, 4) is applied to every cell on the device before it is
    formatted -- DisplayTableau (BranchBoundSimplexSolver.cs:623-640) is 1, a tableau that went
    through RoundAllTableaux first is 2; with any entry non-zero the call is
    lpr_text_format_tableaux_rounded."""
    from . import _native as N
    from .engine import default_engine
    T = [np.ascontiguousarray(t, dtype=np.float64) for t in tableaux]
    if not T or any(t.ndim != 2 for t in T):
        raise ValueError("tableaux must be a non-empty list of 2-D arrays")
    nv = [int(nvars)] * len(T) if np.isscalar(nvars) else [int(v) for v in nvars]
    if len(nv) != len(T):
        raise ValueError("nvars must be an int or hold one entry per tableau")
    rows = np.asarray([t.shape[0] for t in T], dtype=np.int32)
    cols = np.asarray([t.shape[1] for t in T], dtype=np.int32)
    nva = np.asarray(nv, dtype=np.int32)
    flat = np.concatenate([t.reshape(-1) for t in T])
    eng = engine or default_engine()
    h = C.c_void_p()
    r4 = [int(round4)] * len(T) if np.isscalar(round4) else [int(v) for v in round4]
    if len(r4) != len(T):
        raise ValueError("round4 must be an int or hold one entry per tableau")
    if any(r4):
        r4a = np.asarray(r4, dtype=np.int32)
        N.check(N.lib.lpr_text_format_tableaux_rounded(
            eng._h, len(T), N._ptr(rows, C.c_int32), N._ptr(cols, C.c_int32),
            N._ptr(nva, C.c_int32), N._ptr(r4a, C.c_int32), N._ptr(flat, C.c_double),
            C.byref(h)), "lpr_text_format_tableaux_rounded")
        return DeviceText(h)
    N.check(N.lib.lpr_text_format_tableaux(eng._h, len(T), N._ptr(rows, C.c_int32),
                                           N._ptr(cols, C.c_int32), N._ptr(nva, C.c_int32),
                                           N._ptr(flat, C.c_double), C.byref(h)),
            "lpr_text_format_tableaux")
    return DeviceText(h)


def format_bodies(tableaux, nvars, engine=None, round4=0):
    """Format(tab, nvars, title) without its title line for every tableau, on the device;
    ``round4`` as format_device takes it."""
    text = format_device(tableaux, nvars, engine, round4)
    try:
        return text.blocks()
    finally:
        text.destroy()


def FormatMany(tableaux, nvars, titles, engine=None, round4=0):
    """[Format(tab, nvars, title)] for every (tableau, title) pair: bodies from the device, the
    title lines from the host; ``round4`` as format_device takes it."""
    titles = list(titles)
    bodies = format_bodies(tableaux, nvars, engine, round4)
    if len(titles) != len(bodies):
        raise ValueError("one title per tableau")
    return [title_line(t) + b for t, b in zip(titles, bodies)]
