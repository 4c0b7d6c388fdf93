"""Instances and oracle references for the cutting-plane batch (TEST ONLY).

A reference is what the oracle gives for ONE item alone; the batch must give every item those
bits.  test_cut_batch_cpu.py checks on the oracle and on ref_py_cut that every fixture still
reaches the branch it is named for, so a case cannot decay."""
from __future__ import annotations

import numpy as np

import cut_cases

MODE_CUT, MODE_DUAL, MODE_PRIMAL2 = 0, 1, 2
DUAL_STATUS = {0: 0, 1: 2, 3: 3, 5: 5}    # oracle rc -> lpr_status (false = INFEASIBLE_BASIS)
PRIM_STATUS = {0: 0, 1: 1, 3: 3, 5: 5}    # false = UNBOUNDED
MAX_LDS_G = 160 * 1024 - 1024


def exit2_tableau():
    """Integer coefficients and one fractional RHS: the cut row is all zeros but its RHS, so the
    dual ratio fold finds no column (exit 2, :134-138)."""
    return np.array([[2.0, 3.0, 0.0, 0.0, 12.0],
                     [1.0, 2.0, 1.0, 0.0, 4.5],
                     [3.0, 1.0, 0.0, 1.0, 6.0]])


def textbook_items(oracle):
    """(name, tableau): cut_cases.cutting_plane_tableaux plus the exit-2 construction."""
    return list(cut_cases.cutting_plane_tableaux(oracle)) + [("exit2_integer_rows",
                                                               exit2_tableau())]


# the two larger items of the mixed / launch-bound / bench workloads: (tableau, max_cuts) and what
# the oracle gives for them (exit, cuts, pivots)
def g_item(seed=7):
    return cut_cases.side_base(40, 60, seed), 8


def h_item(seed=3):
    return cut_cases.side_base(200, 40, seed), 12


G_ITEM_OUTCOME = (6, 8, 23)
H_ITEM_OUTCOME = (6, 12, 60)


def footprint_g(rows, cols, max_cuts):
    rcap = rows + max_cuts
    return 8 * (rcap * cols + rcap + cols)


def boundary_shapes(m=40, max_cuts=8):
    """(n_fit, n_over): side_base(m, n, .) whose footprint at capacity is the largest that fits
    form G's budget, and the next one."""
    n = 1
    while footprint_g(m + 1, (n + 1) + m + 1, max_cuts) <= MAX_LDS_G:
        n += 1
    return n, n + 1


def cut_limit(rows, rcap, requested):
    left = rcap - rows
    return min(requested, left) if requested > 0 else left


def reference(oracle, mode, T, max_cuts=0, hard_cap=0, max_iters=10000, print_steps=None,
              rcap=None):
    """One call on one item alone: dict(code, cuts, pivots, T, log).  mode 0: max_cuts is what
    the call may add (0 with rcap given: the capacity left)."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    if mode == MODE_CUT:
        mc = max_cuts if rcap is None else cut_limit(T.shape[0], rcap, max_cuts)
        rc, cuts, out, log = oracle.cutting_plane(T, max_cuts=mc, hard_cap=hard_cap)
        return dict(code=rc, cuts=cuts, pivots=len(log), T=out, log=log)
    out = T.copy()
    if print_steps is None:
        print_steps = mode == MODE_DUAL
    fn = oracle.dual_solve if mode == MODE_DUAL else oracle.primal2_solve
    rc, piv, log = fn(out, max_iters=max_iters, print_steps=print_steps, hard_cap=hard_cap)
    code = (DUAL_STATUS if mode == MODE_DUAL else PRIM_STATUS)[rc]
    return dict(code=code, cuts=0, pivots=piv, T=out, log=log)


# ---- lane and walk strides ------------------------------------------------------------------------
# The batch's folds stage their candidates in LDS and one wave walks them 64 at a time; the
# staging loops and the update run 256 lanes apart.  Gap 64 puts the later candidate on the same
# lane one walk step later, 50 and 100 on another lane of the next step(s), 256 on the same
# staging lane one stride later, 320 and 512 further strides.
G_TALL, G_WIDE, G_GAPS = (110, 20), (10, 200), (50, 64)
H_TALL, H_WIDE, H_GAPS = (700, 24), (40, 900), (64, 100, 256, 320, 512)
CUT_ROWS_MODES = ("exact", "later_better", "earlier_better")
STRIDE_HARD_CAP = 3   # the first selection decides the case; the reference stays cheap

# generator name -> (generator, mode, tall?, log field that names the planted index, tie modes)
STRIDE_GENS = {
    "dual_rows": (cut_cases.dual_rows_case, MODE_DUAL, True, 1, tuple(cut_cases.TIE_MODES)),
    "dual_cols": (cut_cases.dual_cols_case, MODE_DUAL, False, 2, tuple(cut_cases.TIE_MODES)),
    "primal2_cols": (cut_cases.primal2_cols_case, MODE_PRIMAL2, False, 2,
                     tuple(cut_cases.TIE_MODES)),
    "primal2_rows": (cut_cases.primal2_rows_case, MODE_PRIMAL2, True, 1,
                     tuple(cut_cases.TIE_MODES)),
    "cut_cols": (cut_cases.cut_cols_case, MODE_CUT, False, 2, tuple(cut_cases.TIE_MODES)),
    "cut_rows": (cut_cases.cut_rows_case, MODE_CUT, True, 2, CUT_ROWS_MODES),
}


def stride_group(gen_name, form):
    """(mode, field, [(name, T, planted)]) of one generator at the shapes of one form ("G" / "H"):
    every tie mode at every gap."""
    gen, mode, tall, field, ties = STRIDE_GENS[gen_name]
    if form == "G":
        (m, n), gaps = (G_TALL if tall else G_WIDE), G_GAPS
    else:
        (m, n), gaps = (H_TALL if tall else H_WIDE), H_GAPS
    items = []
    for tie in ties:
        for gap in gaps:
            T, planted = gen(m, n, tie, gap)
            items.append((f"{gen_name}_{form}_{tie}_gap{gap}", T, planted))
    return mode, field, items


def stride_reference(oracle, mode, T):
    if mode == MODE_CUT:
        return reference(oracle, MODE_CUT, T, max_cuts=1, hard_cap=STRIDE_HARD_CAP)
    return reference(oracle, mode, T, hard_cap=STRIDE_HARD_CAP)


# ---- a NaN factor ---------------------------------------------------------------------------------
def nan_factor_cases(oracle):
    """[(mode, T)]: a primal2 tableau with one NaN in its first entering column and a dual tableau
    with one NaN in its first pivot column, each in a row that is not the pivot row."""
    out = []
    for mode, tabs in ((MODE_PRIMAL2, cut_cases.primal2_tableaux(oracle)),
                       (MODE_DUAL, cut_cases.dual_tableaux(oracle))):
        name, T0 = tabs[0]
        ref = reference(oracle, mode, T0, hard_cap=50)
        kind, row, col = ref["log"][0]
        pr = row if mode == MODE_PRIMAL2 else row + 1
        victim = next(i for i in range(1, T0.shape[0]) if i != pr)
        T = T0.copy()
        T[victim, col] = np.nan
        out.append((mode, T, victim, col))
    return out
