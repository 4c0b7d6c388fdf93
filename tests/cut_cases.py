"""Instances for the cutting-plane side path (TEST ONLY): tableaux (row 0 = objective row)."""
from __future__ import annotations

import numpy as np

import bb_cases
import lp_cases


def primal2_tableaux(oracle):
    """Initial tableaux of LPs with b >= 0 (PrimalSimplexSolver2 assumes a feasible basis)."""
    out = []
    for (m, n, seed) in [(4, 8, 0), (16, 32, 1), (40, 17, 4)]:
        obj, cons, _ = lp_cases.random_dense(m, n, seed)
        o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
        T, _ = oracle.primal_build(o, A, rel, rhs, True, ncoef)
        out.append((f"dense_{m}x{n}_s{seed}", T))
    for (m, n, seed) in [(6, 6, 0), (12, 9, 1), (24, 30, 2)]:
        obj, cons, _ = lp_cases.tie_heavy(m, n, seed)
        cons = [type(c)(c.Coefficients, "<=", abs(c.RHS)) for c in cons]
        o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
        T, _ = oracle.primal_build(o, A, rel, rhs, True, ncoef)
        out.append((f"ties_{m}x{n}_s{seed}", T))
    obj, cons, _ = lp_cases.unbounded_lp()
    o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
    T, _ = oracle.primal_build(o, A, rel, rhs, True, ncoef)
    out.append(("unbounded", T))
    return out


def dual_tableaux(oracle):
    """Dual-feasible tableaux with negative right-hand sides: an optimal tableau plus a violated
    branching row (what AddConstraint hands to a dual simplex), and >= rows negated by the ctor."""
    out = []
    for name, (obj, cons) in bb_cases.all_bb_cases()[:8]:
        st, T, n = bb_cases.primal_final_tableau(oracle, obj, cons)
        vals = [0.0] * n
        for k in range(n):
            for j in range(T.shape[0]):
                if abs(T[j, k] - 1.0) <= 1e-6:
                    vals[k] = T[j, -1]
                    break
        frac = [k for k in range(n) if abs(vals[k] - round(vals[k])) > 1e-6]
        if not frac:
            continue
        k = frac[0]
        for side, bound in ((0, np.floor(vals[k])), (1, np.ceil(vals[k]))):
            con = np.zeros(n + 2)
            con[k] = 1.0
            con[n] = bound
            con[n + 1] = float(side)
            out.append((f"{name}_side{side}", oracle.bb_add_constraint(T, con)))
    # >= rows: the PrimalSimplexSolver ctor negates them, leaving negative RHS with a dual
    # feasible Z row when the objective is a minimisation-style (all reduced costs >= 0)
    rng = np.random.RandomState(5)
    for (m, n) in [(5, 7), (12, 9)]:
        A = rng.randint(1, 9, size=(m, n)).astype(float)
        b = rng.randint(5, 40, size=m).astype(float)
        c = rng.randint(1, 9, size=n).astype(float)
        T = np.zeros((m + 1, n + m + 1))
        T[0, :n] = c
        T[1:, :n] = -A
        T[1:, n:n + m] = np.eye(m)
        T[1:, -1] = -b
        out.append((f"cover_{m}x{n}", T))
    return out


def cutting_plane_tableaux(oracle):
    """Optimal LP tableaux with fractional right-hand sides (what CuttingPlaneSolution expects)."""
    out = []
    for name, (obj, cons) in bb_cases.all_bb_cases():
        st, T, n = bb_cases.primal_final_tableau(oracle, obj, cons)
        out.append((name, T))
    return out


# ---- instances past one workgroup stride --------------------------------------------------------
# The device folds of this path run 1024 lanes in strided loops over rows or columns: index i sits
# on lane i % 1024, wave (i % 1024) // 64.  The generators below build tableaux directly (identity
# slack block, chosen Z row and RHS) and plant the candidates that decide the first selection two
# or three strides apart: an exact tie, a near tie inside the 1e-9 band in either order, and a
# near tie just outside it.  Each returns the planted index the oracle must pick first; the CPU
# tests (test_oracle_cut.py) check that it does, so a case cannot decay into an easy one.

EPS = 1e-9
STRIDE = 1024
# value offsets of the later candidate against the earlier one, and which of the two must win:
# inside the band the earlier index keeps it whichever side the later one lies on
TIE_MODES = {
    "exact": (0.0, 0),
    "later_better_in_band": (-2.0 ** -31, 0),   # ~4.7e-10 better: still the earlier one
    "earlier_better_in_band": (2.0 ** -31, 0),  # the earlier one is the better one
    "later_better_out_of_band": (-2.0 ** -26, 1),  # ~1.5e-8 better: the later one
}


def side_base(m, n, seed):
    """(m + 1) x (n + m + 1) tableau [A | I | b]: Z row >= 0 on the structurals, 0 on the slacks;
    A in [0.05, 1); b in [5, 10) with fractional parts kept away from 0.5 (keys >= 0.1)."""
    rng = np.random.RandomState(seed)
    T = np.zeros((m + 1, n + m + 1))
    T[0, :n] = rng.uniform(1.0, 2.0, size=n)
    T[1:, :n] = rng.uniform(0.05, 1.0, size=(m, n))
    T[1:, n:n + m] = np.eye(m)
    f = rng.uniform(0.1, 0.4, size=m)
    f[rng.rand(m) < 0.5] += 0.5
    T[1:, -1] = rng.randint(5, 10, size=m) + f
    return T


def _pair(lo, gap):
    return lo, lo + gap


def dual_rows_case(m, n, mode, gap, seed=0):
    """Dual simplex: two constraint rows `gap` apart hold the most negative RHS (tie `mode`); every
    other RHS is positive.  Returns (T, planted constraint row)."""
    d, win = TIE_MODES[mode]
    T = side_base(m, n, seed)
    r1, r2 = _pair(37, gap)
    assert r2 < m
    for r, v in ((r1, -1.0), (r2, -1.0 + d)):
        T[r + 1, :n] = np.abs(T[r + 1, :n])
        T[r + 1, 3:n:7] *= -1.0          # a few negative entries: dual ratios >= 1
        T[r + 1, -1] = v
    return T, (r1, r2)[win]


def dual_cols_case(m, n, mode, gap, seed=0):
    """Dual ratio column (fold_dual_column): one negative row whose two cheapest ratios |z / a| sit
    in structural columns `gap` apart.  Returns (T, planted column)."""
    d, win = TIE_MODES[mode]
    T = side_base(m, n, seed)
    c1, c2 = _pair(53, gap)
    assert c2 < n
    r = m // 2
    T[r + 1, :n] = np.abs(T[r + 1, :n])
    T[r + 1, 5:n:11] *= -1.0             # other candidates: ratio >= 1
    T[r + 1, -1] = -1.0
    T[r + 1, c1] = T[r + 1, c2] = -4.0
    T[0, c1] = 1.0                       # ratio 0.25
    T[0, c2] = 1.0 + 4.0 * d             # ratio 0.25 + d
    return T, (c1, c2)[win]


def primal2_cols_case(m, n, mode, gap, seed=0):
    """PrimalSimplexSolver2 entering column: two negative reduced costs `gap` apart, every other
    entry of the Z row >= 0.  Returns (T, planted column)."""
    d, win = TIE_MODES[mode]
    T = side_base(m, n, seed)
    c1, c2 = _pair(53, gap)
    assert c2 < n
    T[0, c1] = -1.0
    T[0, c2] = -1.0 + d
    return T, (c1, c2)[win]


def primal2_rows_case(m, n, mode, gap, seed=0):
    """PrimalSimplexSolver2 leaving row: in the (single) entering column two rows `gap` apart have
    the smallest ratio b / a.  Returns (T, planted tableau row)."""
    d, win = TIE_MODES[mode]
    T = side_base(m, n, seed)
    c = n // 3
    T[0, c] = -1.0
    r1, r2 = _pair(37, gap)
    assert r2 < m
    T[r1 + 1, c] = T[r2 + 1, c] = 4.0    # every other ratio >= 5
    T[r1 + 1, -1] = 4.0                  # ratio 1
    T[r2 + 1, -1] = 4.0 * (1.0 + d)      # ratio 1 + d
    return T, (r1 + 1, r2 + 1)[win]


def cut_rows_case(m, n, mode, gap, seed=0):
    """Cutting plane source row (k_cut_add): two rows `gap` apart have |frac - 0.5| keys 0 and d
    (no EPS band here: a strictly smaller key wins, an exact tie goes to the lower index).  The
    log names the cut row, not its source, so each of the two rows carries a cheap ratio in a
    column of its own (11 / 17): the cut's pivot column tells which row it came from.  Returns
    (T, pivot column of the planted row)."""
    d = {"exact": 0.0, "later_better": -2.0 ** -30, "earlier_better": 2.0 ** -30}[mode]
    T = side_base(m, n, seed)
    r1, r2 = _pair(37, gap)
    assert r2 < m
    T[r1 + 1, -1] = 7.5 + (2.0 ** -30 if d < 0 else 0.0)
    T[r2 + 1, -1] = 9.5 + (2.0 ** -30 if d > 0 else 0.0)
    for r, mine, other in ((r1, 11, 17), (r2, 17, 11)):
        T[r + 1, mine] = 2.25            # cut entry -0.25, ratio 0.125 / 0.25 = 0.5 < 1
        T[r + 1, other] = 1.0            # frac 0: no candidate
    T[0, 11] = T[0, 17] = 0.125
    return T, (17 if d < 0 else 11)


def cut_cols_case(m, n, mode, gap, seed=0):
    """Pivot column on the cut row: the chosen source row's two cheapest ratios sit in columns
    `gap` apart.  Returns (T, planted column)."""
    d, win = TIE_MODES[mode]
    T = side_base(m, n, seed)
    r = m // 2
    T[r + 1, -1] = 6.5                   # the only key 0: the cut comes from this row
    c1, c2 = _pair(53, gap)
    assert c2 < n
    T[r + 1, c1] = T[r + 1, c2] = 2.25   # frac 0.25 -> cut entry -0.25
    T[0, c1] = 0.125                     # ratio 0.5; every other one >= 1 (z >= 1, frac < 1)
    T[0, c2] = 0.125 + 0.25 * d
    return T, (c1, c2)[win]


# (name, solver, T, log field, planted): the first log triple's field (1 row, 2 column) must be
# `planted`.  Tall: 1300 constraint rows; wide: 1250 structural columns; cols % 16 != 0 in both,
# so the rows carry padding.  Gap 1124 puts the later candidate on another wave (lane + 100), gap
# 1024 on the same lane one stride later.
def stride_cases():
    tall, wide = (1300, 24), (40, 1250)
    gens = [("dual_rows", "dual", dual_rows_case, tall, 1),
            ("dual_cols", "dual", dual_cols_case, wide, 2),
            ("primal2_cols", "primal2", primal2_cols_case, wide, 2),
            ("primal2_rows", "primal2", primal2_rows_case, tall, 1),
            ("cut_cols", "cut", cut_cols_case, wide, 2)]
    out = []
    for name, solver, gen, (m, n), field in gens:
        assert (n + m + 1) % 16 != 0
        plan = [(mode, 1124) for mode in TIE_MODES]
        plan += [("exact", 1024), ("later_better_out_of_band", 1024)]
        for mode, gap in plan:
            T, p = gen(m, n, mode, gap)
            out.append((f"{name}_{mode}_gap{gap}", solver, T, field, p))
    for mode, gap in [("exact", 1124), ("later_better", 1124), ("earlier_better", 1124),
                      ("exact", 1024)]:
        T, p = cut_rows_case(1300, 24, mode, gap)
        out.append((f"cut_rows_{mode}_gap{gap}", "cut", T, 2, p))
    T, p = dual_rows_case(2400, 24, "later_better_in_band", 2 * STRIDE + 300)
    out.append(("dual_rows_three_strides", "dual", T, 1, p))
    return out


def run_oracle(oracle, solver, T, hard_cap, max_cuts=1):
    """(status or exit code, pivots or cuts, final tableau, log) of one side-path call."""
    if solver == "cut":
        return oracle.cutting_plane(T, max_cuts=max_cuts, hard_cap=hard_cap)
    T = T.copy()
    fn = oracle.dual_solve if solver == "dual" else oracle.primal2_solve
    rc, piv, log = fn(T, print_steps=(solver == "dual"), hard_cap=hard_cap)
    return rc, piv, T, log


def many_cuts_tall():
    """An optimal tableau with 1100 constraint rows, every RHS fractional: a cutting-plane run
    that is stopped by max_cuts only."""
    return side_base(1100, 60, 3)
