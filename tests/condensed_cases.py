"""Cases for the condensed working layout of the two-stream K-pivot path (TEST ONLY;
csrc/overlap_kernels.hip, solve_condensed in csrc/overlap_driver.hip).  For the length of a solve call
the kernels work on [columns not basic at the start | S spare columns | RHS]; a variable that was
basic at the start ("omitted") gets a spare slot when it leaves.  What the layout can get wrong
depends on WHEN variables leave and enter relative to the blocks of 16 pivots, so the cases are
picked by classifying the oracle's pivot logs (classify), and test_condensed_cpu.py asserts that
every class is met."""
from __future__ import annotations

import numpy as np

import lp_cases
import ov_step_cases as cs
from lp_cases import PyConstraint

OV2 = cs.OV2
FORCE = 1 << 26     # opts.variant bit 26: the condensed layout whatever the size / call length
BEFORE = 1 << 25    # opts.variant bit 25: never condensed (the form before)
SPARES_HOOK = "LPR_TEST_OV_SPARES"

CLASSES = ("omitted-first", "omitted-last", "omitted-consecutive", "reenter-leave-same-block",
           "enter-leave-across-blocks", "row-repeat-in-block", "row-repeat-prev-block")

# (m, n, seed): odd widths, so the physical width is padded; fewer / more rows than columns
SMALL = ((3, 3, 0), (5, 7, 1), (7, 4, 2), (13, 37, 3), (37, 13, 4), (39, 40, 5), (23, 31, 6))
# shapes of ov_step_cases: one / two / six head workgroups, the heads' further-rows path
STEP_SHAPES = ((40, 60, "optimal"), (40, 60, "unbounded"), (300, 700, "optimal"),
               (8, 3000, "optimal"), (8, 3000, "unbounded"), (600, 50, "optimal"))
# integer data, equal reduced costs: (m, n, seed) -> the tie class the oracle shows (ties_of)
INT_TIES = {(30, 8, 58): "sharp", (30, 8, 3): "spare-wins"}


def classify(b0, log, block=16):
    """Classes of events in a pivot log [(row, col)] from start basis b0, with blocks of `block`
    pivots counted from the start of the log (one call, no re-condensing)."""
    basis, omitted, entered_at, out, prev_om, rows = list(b0), set(b0), {}, set(), None, []
    for q, (r, e) in enumerate(log):
        lv, pos = basis[r - 1], q % block
        if lv in omitted:
            omitted.discard(lv)
            if pos == 0:
                out.add("omitted-first")
            if pos == block - 1:
                out.add("omitted-last")
            if prev_om == q - 1:
                out.add("omitted-consecutive")
            prev_om = q
        if lv in entered_at:
            q0 = entered_at.pop(lv)
            out.add("reenter-leave-same-block" if q0 // block == q // block
                    else "enter-leave-across-blocks")
        entered_at[e] = q
        if r in rows[(q // block) * block:q]:
            out.add("row-repeat-in-block")
        if q >= block and r in rows[(q // block - 1) * block:(q // block) * block]:
            out.add("row-repeat-prev-block")
        rows.append(r)
        basis[r - 1] = e
    return out


def build(oracle, case):
    obj, cons, is_max = case
    o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
    T, basis = oracle.primal_build(o, A, rel, rhs, is_max, ncoef)
    return T, basis


def small_case(m, n, seed):
    return cs._negated(lp_cases.random_dense(m, n, seed), False)


def int_lp(m, n, seed):
    """<= rows only (the start basis is the slack columns, exact unit columns), small integers."""
    rng = np.random.RandomState(seed)
    A = rng.randint(0, 3, size=(m, n)).astype(float)
    b = rng.randint(1, 5, size=m).astype(float)
    c = rng.randint(1, 3, size=n).astype(float)
    return c.tolist(), [PyConstraint(A[i].tolist(), "<=", float(b[i])) for i in range(m)], True


def ties_of(oracle, T0, b0, cap=200):
    """Tie classes met when the oracle solves (T0, b0) pivot by pivot.  A column that was basic
    at the start and has left sits in a spare slot, in the order of leaving: "spare-tied" = such a
    column ties for the most negative reduced cost, "spare-wins" = and it is the lowest original
    index among the tied, "sharp" = and another tied spare column left BEFORE it (lower slot,
    higher original index: slot order would pick the wrong one)."""
    T, b = T0.copy(), b0.copy()
    omitted, spare, out = set(b0.tolist()), {}, set()
    for _ in range(cap):
        z = T[0, :-1]
        zmin = z.min()
        tied = [j for j in range(len(z)) if z[j] == zmin] if zmin < 0 else []
        before = b.tolist()
        _, p, log = oracle.primal_solve(T, b, 1)
        if p == 0:
            break
        r, _ = log.tolist()[0]
        sp = [j for j in tied if j in spare]
        if sp and len(tied) >= 2:
            out.add("spare-tied")
            if min(tied) in spare:
                out.add("spare-wins")
                if min(sp, key=lambda j: spare[j]) != min(tied):
                    out.add("sharp")
        lv = before[r - 1]
        if lv in omitted:
            omitted.discard(lv)
            spare[lv] = len(spare)
    return out


_REF = {}


def legs_reference(oracle, key, T0, b0, legs):
    """(T0, b0, [(status, pivots, log, basis, tableau bytes) after each leg]) on the oracle, once
    per key; a leg of 0 has no pivot limit."""
    key = (key, legs)
    if key not in _REF:
        T, basis = T0.copy(), b0.copy()
        states = []
        for leg in legs:
            st, piv, log = oracle.primal_solve(T, basis, leg if leg else 100000)
            states.append((st, piv, log.tolist(), basis.tolist(), T.tobytes()))
            if st != 5:
                break
        _REF[key] = (T0, b0, states)
    return _REF[key]
