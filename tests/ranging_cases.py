"""Analyzer states for the sensitivity-report tests (TEST ONLY), on top of sens_cases.identity_basis
and sens_cases.solved_lp.  A case is (name, T, x, z): what SensState.create takes.  The planted
cases return what they plant as well, and test_ranging_cpu.py asserts it on the restatement, so
that a case cannot decay into an easy one.

The sweep kernel's geometry (csrc/sens_ranging_common.hpp): a tile is TILE_ROWS x TILE_COLS, its
rows are taken SUB_ROWS at a time, lane l of 256 owns columns (2l, 2l + 1) of the tile, 8 lanes
make a segment and 64 a wave."""
from __future__ import annotations

import math

import numpy as np

import sens_cases
import special_values as sv

TILE_ROWS, SUB_ROWS, TILE_COLS = 32, 8, 512
EPS = 1e-9


def dense(m, n_extra, seed, zero_costs=True):
    """identity_basis with a dense slack block in [-1, 1), reduced costs of both signs (a few
    exact zeros of both signs: zero quotients) and right-hand sides of both signs: every row and
    every slack column has many candidates on both sides."""
    T, x, z, _ = sens_cases.identity_basis(m, n_extra, seed)
    rng = np.random.RandomState(1000 + seed)
    n = m + n_extra
    T[1:, n:n + m] = rng.uniform(-1.0, 1.0, size=(m, m))
    T[0, m:n + m] = rng.uniform(-1.0, 2.0, size=n_extra + m)
    if zero_costs and n_extra + m >= 4:
        zs = m + rng.choice(n_extra + m, size=max(2, (n_extra + m) // 16), replace=False)
        T[0, zs] = np.where(rng.randint(2, size=zs.size) == 1, 0.0, -0.0)
    T[1:, -1] = rng.uniform(-3.0, 10.0, size=m)
    if m >= 3:
        T[2, -1] = -0.0
    return T, x, z


def shape_cases():
    """(name, T, x, z, use_numpy_reference): tiny and edge shapes, C - 1 around 16 / 64 / 128, m
    across the tile height and the sub-pass height, one shape with several tiles each way and one
    past 1024 rows and 2048 columns."""
    out = []
    for (m, ne) in [(1, 0), (1, 1), (3, 2)]:
        out.append(("tiny_m%d_ne%d" % (m, ne),) + dense(m, ne, 40 + m + ne) + (False,))
    for m in (1, 2, 7):                       # n = 0: every column is a slack column
        T, x, z = dense(m, 0, 50 + m)
        T = np.ascontiguousarray(T[:, m:])    # drop the structural block: C = m + 1
        out.append(("n0_m%d" % m, T, np.zeros(0), z, False))
    for w in (15, 16, 17, 63, 64, 65, 127, 129):
        m = 5
        out.append(("width_%d" % w,) + dense(m, w - 2 * m, 60 + w) + (False,))
    for m in (SUB_ROWS - 1, SUB_ROWS, SUB_ROWS + 1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1,
              2 * TILE_ROWS + 1):
        out.append(("height_%d" % m,) + dense(m, 3, 70 + m) + (True,))
    # several tile rows and several tile columns (a tile is 512 columns wide, so 1300 of them)
    out.append(("tiles_200x1300",) + dense(199, 1300 - 1 - 2 * 199, 81) + (True,))
    out.append(("tiles_1030x2100",) + dense(1029, 2100 - 1 - 2 * 1029, 82) + (True,))
    return out


# ---- planted order cases -------------------------------------------------------------------------
# column pairs by what separates them in the sweep, each class in both sign orders
ROW_PAIRS = [(32, 33), (36, 37),           # the two columns of one lane
             (40, 44), (42, 46),           # two lanes of one 8-lane segment
             (64, 120), (66, 122),         # two segments of one wave
             (48, 300), (50, 302),         # two waves of one workgroup
             (52, 700), (54, 702),         # two tile columns: two workgroups
             (600, 1290), (602, 1292)]
COL_PAIRS = [(1, 2), (3, 4),               # one sub-pass
             (5, 14), (6, 15),             # two sub-passes of one tile
             (7, 40), (9, 41),             # two tile rows: two workgroups
             (33, 70), (34, 71)]


def row_zero_ties():
    """Per pair (p1, p2) two rows: in the first the only non-negative `lo` candidates are the
    zeros -cbar / 1 at p1 and p2 (all other candidates negative), in the second the only
    non-positive `hi` candidates are the zeros -cbar / -1 (all others positive).  Pair k holds
    (-0, +0) in the Z row when k is even and (+0, -0) when odd.  Returns (T, x, z, plants) with
    plants = [(row, "lo" | "hi", p1, p2)]; the basic column of row r is r - 1."""
    m, ne = 2 * len(ROW_PAIRS), 1300
    T, x, z, _ = sens_cases.identity_basis(m, ne, 91)
    n = m + ne
    T[0, m:n + m] = np.abs(T[0, m:n + m]) + 0.25            # cbar > 0 off the basis
    T[1:, n:n + m] = 0.0                                     # slack block: the diagonal only
    T[1:, n:n + m] += np.diag(np.full(m, 0.75))
    planted_cols = sorted(c for pr in ROW_PAIRS for c in pr)
    assert planted_cols[0] >= m and planted_cols[-1] < n
    plants = []
    for k, (p1, p2) in enumerate(ROW_PAIRS):
        T[0, p1], T[0, p2] = (-0.0, 0.0) if k % 2 == 0 else (0.0, -0.0)
        for which, sign in (("lo", 1.0), ("hi", -1.0)):
            r = 1 + 2 * k + (which == "hi")
            T[r, m:n] = sign * np.abs(T[r, m:n])             # one-sided: -cbar / a has sign -sign
            T[r, planted_cols] = 0.0
            T[r, p1] = T[r, p2] = sign
            T[r, n + r - 1] = sign * 0.75
            plants.append((r, which, p1, p2))
    return T, x, z, plants


def col_zero_ties():
    """The same down slack columns: pair k owns the slack columns of constraints 2k + 1 (`lo`:
    coefficient 1 in rows r1, r2 whose right-hand sides are the zeros, positive elsewhere over
    positive right-hand sides) and 2k + 2 (`hi`).  plants = [(constraint, "lo" | "hi", r1, r2)]."""
    m, ne = 72, 3
    T, x, z, _ = sens_cases.identity_basis(m, ne, 92)
    n = m + ne
    rng = np.random.RandomState(93)
    planted_rows = sorted(r for pr in COL_PAIRS for r in pr)
    assert planted_rows[-1] <= m
    T[1:, n:n + m] = 0.0
    plants = []
    for k, (r1, r2) in enumerate(COL_PAIRS):
        T[r1, -1], T[r2, -1] = (-0.0, 0.0) if k % 2 == 0 else (0.0, -0.0)
        for which, sign in (("lo", 1.0), ("hi", -1.0)):
            c = 2 * k + 1 + (which == "hi")
            s = n + c - 1
            T[1:, s] = sign * rng.uniform(0.25, 1.0, size=m)
            T[planted_rows, s] = 0.0
            T[r1, s] = T[r2, s] = sign
            plants.append((c, which, r1, r2))
    x = x.copy()
    x[:m] = T[1:, -1]
    return T, x, z, plants


def equal_maxima(m=6, ne=40, seed=94):
    """Two N columns that are copies of each other and hold every row's largest `lo` candidate
    (-(-50) / 0.5 = 100), and two rows that agree on the slack block and the RHS (candidate
    40 / 0.5 = 80 in every slack column): equal non-zero candidates at two indices."""
    T, x, z = dense(m, ne, seed, zero_costs=False)
    n = m + ne
    T[0, m + 2] = -50.0
    T[1:, m + 2] = 0.5
    T[:, m + 9] = T[:, m + 2]
    T[1, n:n + m] = 0.5
    T[1, -1] = -40.0
    T[2, n:] = T[1, n:]
    return T, x, z


def eps_boundary():
    """Row 1 holds +-1e-9 exactly and one ulp either side in six N columns and nothing else off the
    basis: only eps+ulp is a `lo` candidate and only -eps-ulp a `hi` candidate.  Row 7 has no
    qualifying entry.  Slack column of constraint 3 holds the same six values down rows 1..6, the
    slack column of constraint 4 nothing.  Returns (T, x, z, vals)."""
    vals = [sv.CLASSES[k] for k in ("eps", "eps+ulp", "eps-ulp", "-eps", "-eps-ulp", "-eps+ulp")]
    m, ne = 7, 8
    T, x, z, _ = sens_cases.identity_basis(m, ne, 95)
    n = m + ne
    T[1:, m:n + m] = 0.0
    for q, v in enumerate(vals):
        T[1, m + q] = v
        T[1 + q, n + 2] = v
    T[3:7, m + 7] = 0.5                       # rows 3..6 keep one ordinary candidate each
    return T, x, z, vals


SPECIALS = (math.nan, math.inf, -math.inf, 1e308)
PLACES = ("z_row", "basic_row", "rhs", "slack_col")


def nonfinite_cases(m, ne, seed=96):
    """[(name, T, x, z)]: dense(m, ne) with one special value in the Z row, in a row of the body,
    in the RHS column or in a slack column, near the start and near the end of that row / column
    (first and last tile at the GPU's shape), finite candidates on both sides of it; then the
    constructed ones: a NaN entry `a` (skipped), a NaN reduced cost under a qualifying entry (the
    NaN quotient sticks) and inf / inf."""
    base = dense(m, ne, seed)
    n = m + ne
    out = []
    for v in SPECIALS:
        tag = "nan" if v != v else repr(v)
        for place in PLACES:
            for end in (0, 1):
                T = base[0].copy()
                jn = m + 2 if end == 0 else n - 2           # an N column
                js = n + 1 if end == 0 else n + m - 2       # a slack column
                i = 2 if end == 0 else m - 1
                if place == "z_row":
                    T[0, jn] = v
                    T[0, js] = v
                elif place == "basic_row":
                    T[i, jn] = v
                elif place == "rhs":
                    T[i, -1] = v
                else:
                    T[i, js] = v
                out.append(("%s_%s_%d" % (tag, place, end), T, base[1], base[2]))
    T = base[0].copy()
    T[2, m + 1] = math.nan                                   # a NaN `a`: neither > EPS nor < -EPS
    T[3, n + 2] = math.nan
    out.append(("nan_entry_skipped", T, base[1], base[2]))
    T = base[0].copy()
    T[0, m + 1] = math.nan
    T[1:, m + 1] = 0.5                                       # qualifies in every row
    T[3, -1] = math.nan
    T[3, n:n + m] = -0.5                                     # row 3 qualifies in every slack column
    out.append(("nan_quotient_sticks", T, base[1], base[2]))
    T = base[0].copy()
    T[0, m + 3] = math.inf
    T[2, m + 3] = math.inf                                   # -inf / inf
    T[4, -1] = -math.inf
    T[4, n + 1] = math.inf                                   # inf / inf
    out.append(("inf_over_inf", T, base[1], base[2]))
    return out


def degenerate_created():
    """States whose rebuilt basicVars (the ctor's RebuildBasicsFromTableau, :35) is degenerate:
    a row without a unit column (a -1 entry), two identical unit columns (only the first is in
    basicVars; the second is non-basic although GetBasicRow finds its row)."""
    out = []
    T, x, z = dense(6, 9, 97)
    T[3, 2] = 0.5                              # column 2 is no unit column: row 3 has none
    out.append(("row_without_unit_column", T, x, z))
    T, x, z = dense(6, 9, 98)
    T[:, 6 + 4] = T[:, 1]                      # N column 10 is a copy of basic column 1
    out.append(("identical_unit_columns", T, x, z))
    return out


def row_not_found_script():
    """(T, x, z, (k, new_b)): after change_rhs(k, new_b) column 0 is still in basicVars but is no
    unit column any more, so GetBasicRow(0) is -1 (kind BASIC_ROW_NOT_FOUND).  Column 0 holds
    0.9e-9 (counted as zero) in rows 2 and 3; the edit's one dual pivot (row 3 leaves, column m
    enters, pivot -1) adds 1.5 * 0.9e-9 to row 2's entry, which passes EPS.  ChangeRHS does not
    rebuild basicVars (:455-456)."""
    m, ne = 5, 3
    T, x, z, _ = sens_cases.identity_basis(m, ne, 99)
    n = m + ne
    T[2, 0] = T[3, 0] = 0.9e-9
    T[1:, m] = 0.0
    T[3, m:n] = np.abs(T[3, m:n])
    T[3, m] = -1.0
    T[2, m] = 1.5
    s3 = T[3, n + 2]
    new_b = float(T[3, -1] + (-1.0 - T[3, -1]) / s3)        # right-hand side of row 3 becomes -1
    return T, x, z, (3, new_b)


def raw_bases():
    """[(name, T, basicVars)] for the restatement alone: bases that no call can hand to the device
    (lpr_sens_create rebuilds basicVars from the tableau) -- an entry whose column is no unit
    column, a duplicate entry, a -1 entry."""
    T, _, _ = dense(6, 9, 100)
    return [("non_unit_entry", T, [0, 1, 2, 3, 4, 8]),
            ("duplicate_entry", T, [0, 1, 1, 3, 4, 5]),
            ("minus_one_entry", T, [0, -1, 2, 3, -1, 5])]


def coverage():
    """dense(12, 20) with two rows and two slack columns one-sided: finite, -inf and +inf bounds all
    occur in the cost ranges and in the RHS ranges."""
    m, ne = 12, 20
    T, x, z = dense(m, ne, 101)
    n = m + ne
    T[4, m:n + m] = np.abs(T[4, m:n + m])      # row 4: no `hi` candidate
    T[5, m:n + m] = -np.abs(T[5, m:n + m])     # row 5: no `lo` candidate
    T[1:, n + 6] = -np.abs(T[1:, n + 6])       # slack column of constraint 7: no `lo` candidate
    T[1:, n + 8] = np.abs(T[1:, n + 8])        # slack column of constraint 9: no `hi` candidate
    T[4:6, [n + 6, n + 8]] = 0.0               # the one-sided rows and columns do not cross
    return T, x, z


def hand_worked():
    """max 3 x1 + 2 x2, x1 + x2 <= 4, x1 + 3 x2 <= 6, optimal at (4, 0):
         Z row  [0  1  3  0 | 12], row 1 [1 1 1 0 | 4] (x1 basic), row 2 [0 2 -1 1 | 2] (s2 basic).
    x1: a = (1, 1) at x2, s1 with cbar (1, 3): lo = max(-1, -3) = -1, hi = +inf.
    s2: a = (2, -1): lo = -1 / 2, hi = -3 / -1 = 3.
    Constraint 1 (column s1 = (1, -1), b = (4, 2)): lo = -4, hi = 2.  Constraint 2 (column s2 =
    (0, 1)): lo = -2, hi = +inf."""
    T = np.array([[0.0, 1.0, 3.0, 0.0, 12.0],
                  [1.0, 1.0, 1.0, 0.0, 4.0],
                  [0.0, 2.0, -1.0, 1.0, 2.0]])
    want = dict(kind=[3, 0, 0, 3], var_row=[1, -1, -1, 2], reduced_cost=[0.0, 1.0, 3.0, 0.0],
                cost_lo=[-1.0, -math.inf, -math.inf, -0.5],
                cost_hi=[math.inf, math.inf, math.inf, 3.0],
                shadow=[3.0, 0.0], rhs_lo=[-4.0, -2.0], rhs_hi=[2.0, math.inf], rhs_now=[4.0, 2.0])
    return T, [4.0, 0.0], 12.0, [0, 3], want


def rebuilt_basis(T):
    """RebuildBasicsFromTableau (:706-723): per row the first column whose GetBasicRow is that
    row, else -1 -- what the device holds after lpr_sens_create."""
    import ref_py_ranging as ref
    T = np.ascontiguousarray(T, dtype=np.float64)
    R, C = T.shape
    gbr = ref.report_numpy(T, range(C - 1))["var_row"]      # every column asked: GetBasicRow
    basic = [-1] * (R - 1)
    for j in range(C - 2, -1, -1):
        if gbr[j] >= 1:
            basic[gbr[j] - 1] = j
    return basic


def cpu_cases():
    """[(name, T, basicVars)] for test_ranging_cpu.py: every builder at shapes up to 70 x 200."""
    out = []
    for name, T, x, z, _ in shape_cases():
        if T.shape[0] <= 70 and T.shape[1] <= 200:
            out.append((name, T, rebuilt_basis(T)))
    out.append(("equal_maxima", equal_maxima()[0], None))
    out.append(("eps_boundary", eps_boundary()[0], None))
    out.append(("coverage", coverage()[0], None))
    for name, T, x, z in nonfinite_cases(12, 30):
        out.append((name, T, None))
    for name, T, x, z in degenerate_created():
        out.append((name, T, None))
    out.append(("row_not_found_start", row_not_found_script()[0], None))
    out = [(name, T, rebuilt_basis(T) if b is None else b) for name, T, b in out]
    return out + raw_bases()
