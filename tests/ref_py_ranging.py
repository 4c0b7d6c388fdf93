"""Restatement of the sensitivity report (TEST ONLY): what lpr_sens_ranging must return, written
twice.

``report_literal`` restates SensitivityAnalysis/SensitivityAnalyzer.cs index by index, with the
C#'s sequential loops: DisplayRangeNonBasic :276-297, DisplayRangeBasic :324-359, DisplayRangeRHS
:396-424, ShadowPrices :212-222, GetBasicRow / IsPivotColumn :69-84.  Math.Max / Math.Min are the
.NET Framework forms, written out as dotnet_max / dotnet_min.

``report_numpy`` is a second, vectorised formulation for shapes the loops are too slow for.  It
does not scan: a fold is NaN when any candidate is, else the largest (smallest) candidate, and of
equal candidates the one with the largest index -- form (b) of DESIGN.md section 18.
test_ranging_cpu.py holds the two against each other.

Both take the analyzer's state (tableau rows x cols with row 0 = Z row, basicVars) and return
{field: array} with the fields of engine.RangingReport."""
from __future__ import annotations

import math

import numpy as np

EPS = 1e-9  # :20
INF = math.inf

NONBASIC_RANGE, NONBASIC_BOUNDARY, NONBASIC_NOT_OPTIMAL, BASIC, BASIC_ROW_NOT_FOUND = range(5)
FIELDS = ("kind", "var_row", "reduced_cost", "cost_lo", "cost_hi", "shadow", "rhs_lo", "rhs_hi",
          "rhs_now")
INT_FIELDS = ("kind", "var_row")


def dotnet_max(a: float, b: float) -> float:
    """.NET Framework Math.Max(double, double)."""
    if a > b:
        return a
    if a != a:  # double.IsNaN(a)
        return a
    return b


def dotnet_min(a: float, b: float) -> float:
    """.NET Framework Math.Min(double, double)."""
    if a < b:
        return a
    if a != a:
        return a
    return b


# ---- the literal restatement -------------------------------------------------------------------
def is_pivot_column(T, pivot_row: int, col: int) -> bool:  # :79-84
    for i in range(1, len(T)):
        if i != pivot_row and abs(T[i][col]) > EPS:
            return False
    return True


def get_basic_row(T, col: int) -> int:  # :69-77
    for i in range(1, len(T)):
        if abs(T[i][col] - 1.0) < EPS and is_pivot_column(T, i, col):
            return i
    return -1


def basic_range(T, basic, index: int, r: int):  # :340-355
    lo, hi = -INF, INF
    for j in range(len(T[0]) - 1):
        if j == index or j in basic:
            continue
        a_rj = T[r][j]
        cbar_j = T[0][j]
        if a_rj > EPS:
            lo = dotnet_max(lo, -cbar_j / a_rj)
        elif a_rj < -EPS:
            hi = dotnet_min(hi, -cbar_j / a_rj)
    return lo, hi


def rhs_range(T, s_col: int):  # :406-418
    lo, hi = -INF, INF
    last = len(T[0]) - 1
    for i in range(1, len(T)):
        coeff = T[i][s_col]
        bi = T[i][last]
        if coeff > EPS:
            lo = dotnet_max(lo, -bi / coeff)
        elif coeff < -EPS:
            hi = dotnet_min(hi, -bi / coeff)
    return lo, hi


def _as_lists(T):
    A = np.ascontiguousarray(T, dtype=np.float64)
    return [[float(v) for v in row] for row in A]   # Python floats: plain IEEE, no numpy warnings


def report_literal(T, basic):
    T = _as_lists(T)
    basic = [int(b) for b in basic]
    R, C = len(T), len(T[0])
    m = R - 1
    n = C - m - 1
    assert n >= 0, "the C# indexes tableau[0, n + k - 1] out of range"
    kind, var_row, rc, clo, chi = [], [], [], [], []
    for j in range(C - 1):
        cbar = T[0][j]
        lo, hi, r = -INF, INF, -1
        if j in basic:                              # :330
            r = get_basic_row(T, j)
            if r == -1:
                k = BASIC_ROW_NOT_FOUND             # :337
            else:
                k = BASIC
                lo, hi = basic_range(T, basic, j, r)
        elif cbar > EPS:                            # :291
            k = NONBASIC_RANGE
        elif abs(cbar) <= EPS:                      # :293
            k = NONBASIC_BOUNDARY
        else:                                       # :295, a NaN cbar too
            k = NONBASIC_NOT_OPTIMAL
        kind.append(k)
        var_row.append(r)
        rc.append(cbar)
        clo.append(lo)
        chi.append(hi)
    shadow, rlo, rhi, now = [], [], [], []
    for k in range(1, R):
        s = n + (k - 1)                             # SlackColForConstraint :62-67
        lo, hi = rhs_range(T, s)
        shadow.append(T[0][s])
        rlo.append(lo)
        rhi.append(hi)
        now.append(T[k][C - 1])
    f8 = lambda v: np.array(v, dtype=np.float64)
    i4 = lambda v: np.array(v, dtype=np.int32)
    return dict(kind=i4(kind), var_row=i4(var_row), reduced_cost=f8(rc), cost_lo=f8(clo),
                cost_hi=f8(chi), shadow=f8(shadow), rhs_lo=f8(rlo), rhs_hi=f8(rhi), rhs_now=f8(now))


# ---- the vectorised formulation ----------------------------------------------------------------
def _fold_last_extreme(Q, mask, largest: bool):
    """Along axis 1 of Q, over the entries where mask holds: NaN if any is NaN; else the largest
    (smallest) value, taken from the LAST position that holds it; the identity where none."""
    ident = -INF if largest else INF
    nan = (mask & np.isnan(Q)).any(axis=1)
    V = np.where(mask & ~np.isnan(Q), Q, ident)
    ext = V.max(axis=1) if largest else V.min(axis=1)
    eq = mask & (V == ext[:, None])                  # +0 == -0: both zeros are positions of a tie
    ncol = Q.shape[1]
    last = ncol - 1 - np.argmax(eq[:, ::-1], axis=1)
    out = np.where(eq.any(axis=1), V[np.arange(Q.shape[0]), last], ident)
    return np.where(nan, np.nan, out)


def report_numpy(T, basic):
    T = np.ascontiguousarray(T, dtype=np.float64)
    R, C = T.shape
    m = R - 1
    n = C - m - 1
    assert n >= 0
    nc = C - 1
    in_basis = np.zeros(nc, dtype=bool)
    for b in basic:
        if 0 <= int(b) < nc:
            in_basis[int(b)] = True
    body = T[1:, :nc]
    # GetBasicRow for every column: exactly one row with |v| > EPS, and that row within EPS of 1
    big = np.abs(body) > EPS
    cnt = big.sum(axis=0)
    row = 1 + np.argmax(big, axis=0)
    unit = (cnt == 1) & (np.abs(T[row, np.arange(nc)] - 1.0) < EPS)
    gbr = np.where(unit, row, -1)
    cbar = T[0, :nc]
    with np.errstate(all="ignore"):
        Qr = -cbar[None, :] / body                   # -cbar_j / a_rj for every row and column
        free = ~in_basis[None, :]
        row_lo = _fold_last_extreme(Qr, free & (body > EPS), True)
        row_hi = _fold_last_extreme(Qr, free & (body < -EPS), False)
        S = T[1:, n:n + m]                           # the slack block, constraint k in column k - 1
        Qc = (-T[1:, C - 1][:, None] / S).T          # transposed: fold along the rows
        rhs_lo = _fold_last_extreme(Qc, (S > EPS).T, True)
        rhs_hi = _fold_last_extreme(Qc, (S < -EPS).T, False)
    kind = np.full(nc, NONBASIC_NOT_OPTIMAL, dtype=np.int32)
    kind[np.abs(cbar) <= EPS] = NONBASIC_BOUNDARY
    kind[cbar > EPS] = NONBASIC_RANGE
    kind[in_basis] = BASIC_ROW_NOT_FOUND
    found = in_basis & (gbr >= 1)
    kind[found] = BASIC
    var_row = np.where(found, gbr, -1).astype(np.int32)
    clo = np.full(nc, -INF)
    chi = np.full(nc, INF)
    clo[found] = row_lo[gbr[found] - 1]
    chi[found] = row_hi[gbr[found] - 1]
    return dict(kind=kind, var_row=var_row, reduced_cost=cbar.copy(), cost_lo=clo, cost_hi=chi,
                shadow=T[0, n:n + m].copy(), rhs_lo=rhs_lo, rhs_hi=rhs_hi,
                rhs_now=T[1:, C - 1].copy())
