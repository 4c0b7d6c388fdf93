"""Case list and oracle helpers of the traced primal batch tests (lpr_batch_trace_*, DESIGN.md
section 22; TEST ONLY): lp_cases.all_cases() plus constructed models, and the oracle stepped one
pivot at a time (find_entering / find_leaving / pivot, as special_values.step_oracle) to give the
records a traced batch must hold.  test_batch_trace_cpu.py checks with the oracle alone that the
constructed cases do what the GPU tests rely on."""
import numpy as np

import lp_cases
from ref_py import PyConstraint

OPTIMAL, UNBOUNDED, LIMIT = 0, 1, 5  # lpr_status
CAP = 5000           # tie-heavy LPs can cycle: every solve is capped, here and in the oracle
TRACE_CAP = 64       # records kept per LP in the batch of every case
SMALL_TRACE_CAP = 3  # the record-cap test
SHAPE_PIVOTS = 6     # max_pivots at the G and H shapes: the slabs stay in the low megabytes
# (m, n) at each threshold and one column past it: W holds
# rows * (cols + 1) <= 2016 doubles, G <= 20352
THRESHOLDS = [(31, 30), (31, 31), (63, 253), (63, 254)]
W_MAX, G_MAX = 2016, 20352


def zero_pivot_lp():
    """Optimal with no pivot: under max every objective coefficient is <= 0, so row 0 has no
    negative entry."""
    return [-1.0, -2.0, 0.0], [PyConstraint([1.0, 1.0, 1.0], "<=", 4.0),
                               PyConstraint([1.0, 0.0, 2.0], "<=", 3.0)], True


def unbounded_later_lp():
    """x1 enters and row 1 leaves; then x2's column is [-3; -1]: unbounded after one pivot."""
    return [2.0, 1.0], [PyConstraint([1.0, -1.0], "<=", 4.0)], True


def cap_lp():
    """Tie-heavy, more pivots than SMALL_TRACE_CAP records hold."""
    return lp_cases.tie_heavy(24, 30, 2)


def form_models():
    """One model per natural form: W, G at (31, 31), H at (63, 254)."""
    return [("form_w_6x9", lp_cases.random_dense(6, 9, 11)),
            ("form_g_31x31", lp_cases.random_dense(31, 31, 131)),
            ("form_h_63x254", lp_cases.random_dense(63, 254, 354))]


def all_cases():
    return (lp_cases.all_cases() + [("zero_pivot", zero_pivot_lp()),
                                    ("unbounded_later", unbounded_later_lp())] + form_models())


def negative_zero_tableau():
    """The tableau of test_batch_gpu.test_zero_factor_meets_negative_zero: row 2 has factor +0 and
    a -0.0 under the pivot row's -2; the C# writes -0.0 - (+0 * -2) = +0.0 there."""
    T = np.array([[-1.0, 0.0, 0.0, 0.0],
                  [2.0, -4.0, 1.0, 6.0],
                  [0.0, -0.0, 0.0, 5.0]])
    return T, np.array([2, 3], dtype=np.int32)


def form_of(rows, cols):
    """batch_pick_form of DESIGN.md section 12 by the footprint rows * cols + rows."""
    fp = rows * cols + rows
    return 0 if fp <= W_MAX else (1 if fp <= G_MAX else 2)


def models_of(cases):
    from lpr_381_group_v22_amd import Constraint
    return [(obj, [Constraint(list(c.Coefficients), c.Relation, c.RHS) for c in cons], mx)
            for obj, cons, mx in cases]


def built(oracle, case):
    obj, cons, mx = case
    o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
    return oracle.primal_build(o, A, rel, rhs, mx, ncoef)[0]


def step_records(oracle, T0, max_pivots=CAP, keep=TRACE_CAP):
    """The oracle's loop one call at a time on a copy of T0: dict(status, pivots, records, T).
    records[i] = (leaving_row, entering_col, tableau after i pivots) for i < keep; record 0 has
    -1, -1.  The limit is checked where the batch checks it: after both selections."""
    T = np.ascontiguousarray(T0, dtype=np.float64).copy()
    records = [(-1, -1, T.copy())]
    it = 0
    while True:
        e = oracle.find_entering(T)
        if e < 0:
            status = OPTIMAL
            break
        r = oracle.find_leaving(T, e)
        if r < 0:
            status = UNBOUNDED
            break
        if max_pivots > 0 and it >= max_pivots:
            status = LIMIT
            break
        oracle.pivot(T, r, e)
        it += 1
        if it < keep:
            records.append((r, e, T.copy()))
    return dict(status=status, pivots=it, records=records, T=T)


_REFS = {}


def refs_of(oracle, key, tableaux, max_pivots=CAP, keep=TRACE_CAP):
    """step_records of a list of start tableaux, computed once per key and left unchanged."""
    if key not in _REFS:
        _REFS[key] = [step_records(oracle, T, max_pivots, keep) for T in tableaux]
    return _REFS[key]


def record_bytes(rec):
    r, e, T = rec
    return np.concatenate([[float(r), float(e)], T.reshape(-1)]).tobytes()
