"""Edit scripts for the sensitivity re-solve tests (TEST ONLY): a solved LP + a list of
(operation, args) applied in order to the same analyzer, as a user of the reference's sub-menu
(Program.cs:158-294) would."""
from __future__ import annotations

import math

import numpy as np

import lp_cases


def solved_lp(oracle, m, n, seed, integer=False):
    if integer:
        obj, cons, _ = lp_cases.tie_heavy(m, n, seed)
        cons = [type(c)(c.Coefficients, "<=", abs(c.RHS) + 1.0) for c in cons]
    else:
        obj, cons, _ = lp_cases.random_dense(m, n, seed)
    o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
    T, basis = oracle.primal_build(o, A, rel, rhs, True, ncoef)
    st, piv, log = oracle.primal_solve(T, basis)
    assert st == 0
    x, z = oracle.extract_solution(T, n)
    return T, x, z, basis


def scripts(oracle):
    """[(name, (T, x, z, basis), [(op, args), ...])]"""
    out = []
    for (m, n, seed, integer) in [(4, 6, 0, False), (8, 12, 1, False), (6, 6, 2, True),
                                  (12, 9, 3, True), (16, 24, 4, False)]:
        base = solved_lp(oracle, m, n, seed, integer)
        T, x, z, basis = base
        rng = np.random.RandomState(100 + seed)
        C = T.shape[1]
        bset = set(int(b) for b in basis)
        nonbasic = [j for j in range(C - 1) if j not in bset]
        basic = [j for j in range(n) if j in bset] or [int(basis[0])]
        ops = [
            ("resolve_all", ()),
            ("change_nonbasic_cbar", (nonbasic[0], -2.5)),          # makes a reduced cost negative
            ("change_basic", (basic[0], 0.75)),
            ("change_rhs", (1, float(T[1, -1]) + 3.0)),
            ("change_rhs", (min(2, m), -5.0)),                       # may be rolled back
            ("change_nonbasic_column", (1, nonbasic[-1], 0.5)),
            ("add_activity", (float(rng.uniform(5, 9)), rng.uniform(0.1, 1.0, size=m).tolist())),
            ("add_constraint", (None, 1.0)),                         # tech filled in by the test
            ("change_nonbasic_cbar", (10 ** 6, 1.0)),                # invalid index
            ("change_rhs", (1, 0.0)),
            ("add_constraint_infeasible", ()),                       # code 2, state left mid-way
            ("add_activity_unbounded", ()),                          # code 1
        ]
        out.append((f"lp_{m}x{n}_s{seed}", base, ops))
    return out


def make_tech(width: int, seed: int):
    rng = np.random.RandomState(seed)
    t = np.zeros(width)
    k = max(1, width // 3)
    t[:k] = rng.randint(1, 4, size=k)
    return t.tolist()


def materialize(op, args, T, k):
    """Fill in the arguments that depend on the analyzer's current shape."""
    R, C = T.shape
    if op == "add_constraint" and args[0] is None:
        return op, (make_tech(C - 1, 7 + k), args[1])
    if op == "add_constraint_infeasible":       # sum of all columns <= -1 with x >= 0
        return "add_constraint", ([1.0] * (C - 1), -1.0)
    if op == "add_activity_unbounded":          # profitable activity that uses nothing
        return "add_activity", (50.0, [-1.0] * (R - 1))
    return op, args


# ---- analyzers past one workgroup stride --------------------------------------------------------
# k_sens_select folds rows or columns on one 1024-lane workgroup: eps_fold in contiguous chunks of
# ceil(n / 1024) (cached up to 16 candidates per lane, a strided next-take search above 16 384,
# and the same search when more than kFoldCap = 1024 prefix minima survive), the phase-1 arg-min
# in a strided loop.  The bases below are built directly, so any shape is cheap: an identity basis
# on the first m structural columns, nonbasic structurals N, a nonbasic slack block S, RHS >= 0.
# Each script names the log entry its planted candidates must decide (checked on the CPU by
# test_oracle_sens.py, so a case cannot decay into an easy one).

EPS = 1e-9
# later candidate's value against the earlier one's, and which one an EPS-band fold keeps
TIE_MODES = {
    "exact": (0.0, 0),
    "later_better_in_band": (-2.0 ** -31, 0),
    "earlier_better_in_band": (2.0 ** -31, 0),
    "later_better_out_of_band": (-2.0 ** -26, 1),
}


def identity_basis(m, n_extra, seed):
    """(T, x, z, basis): T = [I_m | N | S | b] with Z = 0 on the basis, >= 1 on N, >= 0.5 on S,
    N in [-1, 1), S diagonal in [0.5, 1), b in [5, 10).  Optimal and primal feasible."""
    rng = np.random.RandomState(seed)
    n = m + n_extra
    T = np.zeros((m + 1, n + m + 1))
    T[0, m:n] = rng.uniform(1.0, 2.0, size=n_extra)
    T[0, n:n + m] = rng.uniform(0.5, 1.5, size=m)
    T[1:, :m] = np.eye(m)
    T[1:, m:n] = rng.uniform(-1.0, 1.0, size=(m, n_extra))
    T[1:, n:n + m] = np.diag(rng.uniform(0.5, 1.0, size=m))
    T[1:, -1] = rng.uniform(5.0, 10.0, size=m)
    T[0, -1] = 100.0
    x = np.zeros(n)
    x[:m] = T[1:, -1]
    return T, x, 100.0, np.arange(m, dtype=np.int32)


def _mode(mode):
    return TIE_MODES[mode]


def leaving_rows_script(mode, gap=1124, m=1200, n_extra=40):
    """Phase 0 on more than 1024 rows: one change_rhs drives rows 38 and 38 + gap to -1 and -1 + d
    (slack column k holds -1 in both); then change_basic on a column whose basic row lies past
    the first stride (k_sens_basic_row).  Expect: the first dual pivot leaves the planted row."""
    d, win = _mode(mode)
    T, x, z, basis = identity_basis(m, n_extra, 21)
    n = m + n_extra
    r1, r2 = 38, 38 + gap
    k = 500                                   # constraint k: slack column n + k - 1
    T[r1, n + k - 1] = T[r2, n + k - 1] = -1.0
    T[r1, -1] = 5.0
    T[r2, -1] = 5.0 + d
    x[r1 - 1], x[r2 - 1] = T[r1, -1], T[r2, -1]
    newb = float(T[k, -1]) + 6.0
    ops = [("change_rhs", (k, newb)),
           ("change_basic", (m - 3, 0.25)),
           ("resolve_all", ())]
    return (T, x, z, basis), ops, [(0, 0, 1, (r1, r2)[win])]


def _plant_entering(T, row, cols, d):
    """Row `row` gets -4 in the two columns (ratio Z / 4 = 0.25 and 0.25 + d), and its other
    negative entries keep ratios >= 1 (Z >= 1 on N, >= 0.5 on S where S is diagonal)."""
    c1, c2 = cols
    T[row, c1] = T[row, c2] = -4.0
    T[0, c1] = 1.0
    T[0, c2] = 1.0 + 4.0 * d


def entering_cols_script(mode, m, n_extra, gap, c1=100):
    """Phase 0 with more than 1024 (or 16 384) columns: change_rhs makes one row negative; its two
    cheapest ratios sit in N columns c1 and c1 + gap.  Expect: the first dual pivot enters the
    planted column."""
    d, win = _mode(mode)
    T, x, z, basis = identity_basis(m, n_extra, 22)
    r = m // 2 + 1
    T[r, m:m + n_extra] = np.abs(T[r, m:m + n_extra])
    T[r, m + 7:m + n_extra:13] *= -1.0
    cols = (c1, c1 + gap)
    assert m <= cols[0] and cols[1] < m + n_extra
    _plant_entering(T, r, cols, d)
    ops = [("change_rhs", (r, -20.0)), ("resolve_all", ())]
    return (T, x, z, basis), ops, [(0, 0, 2, cols[win])]


def argmin_cols_script(mode, m, n_extra, gap, c1=100, r1=6, r2=71):
    """Phase 1 with more than 1024 columns: two reduced costs c1, c1 + gap are negative.  The
    entering arg-min has no EPS band (a strictly smaller value wins, an exact tie goes to the lower
    index); the leaving fold over the rows does: rows r1 / r2 hold ratios 1 and 1 + d in both
    columns.  Expect: the first primal pivot is (planted row, planted column)."""
    d, win = _mode(mode)
    T, x, z, basis = identity_basis(m, n_extra, 23)
    cols = (c1, c1 + gap)
    assert m <= cols[0] and cols[1] < m + n_extra and r2 < m
    enter = cols[0] if d >= 0 else cols[1]
    T[0, cols[0]] = -1.0
    T[0, cols[1]] = -1.0 + d
    for c in cols:
        T[1:, c] = np.random.RandomState(c).uniform(-0.2, 0.2, size=m)   # ratios >= 25
        T[r1, c] = T[r2, c] = 4.0
    T[r1, -1] = 4.0
    T[r2, -1] = 4.0 * (1.0 + d)
    x[r1 - 1], x[r2 - 1] = T[r1, -1], T[r2, -1]
    return (T, x, z, basis), [("resolve_all", ())], [(0, 0, 1, (r1, r2)[win]), (0, 0, 2, enter)]


def prefix_minima_script(step, m=70, n_extra=1600):
    """More than kFoldCap strictly decreasing prefix minima: the negative row has -1 in every N
    column and Z falls by `step` per column, so every candidate is a prefix minimum.  With step 1
    every one is taken; with a step inside the EPS band only every third or so.  Expect: the
    column a sequential fold ends on."""
    T, x, z, basis = identity_basis(m, n_extra, 24)
    r = 9
    T[r, m:m + n_extra] = -1.0
    T[0, m:m + n_extra] = 1.0 + step * np.arange(n_extra, 0, -1)
    best, take = np.inf, -1
    for j in range(m, m + n_extra):             # the sequential fold (S entries of row r are >= 0)
        if T[0, j] < best - EPS:
            best, take = T[0, j], j
    return (T, x, z, basis), [("change_rhs", (r, -20.0))], [(0, 0, 2, take)]


def growth_script(m=1030, n_extra=20):
    """add_activity twice, add_constraint twice, on more than 1024 rows (the device analyzer
    re-allocates on every add), then resolve_all.  Each activity uses one row and has reduced cost
    -0.5: one primal pivot; each constraint caps one basic variable 1 below its value: one dual
    pivot."""
    T, x, z, basis = base = identity_basis(m, n_extra, 25)
    n = m + n_extra
    width = T.shape[1] - 1

    def activity(r, rows):
        a = np.zeros(rows)
        a[r - 1] = 1.0
        return float(T[0, n + r - 1]) + 0.5, a.tolist()   # c - y_r a_r = 0.5

    def cap(col, w, enter):
        # row col + 1 gets N entries >= 0 except -1 in `enter`, whose other entries are at most 1
        # in size: the new row is that row, its RHS -1, and one pivot leaves every RHS >= 4
        r = col + 1
        T[r, m:n] = np.abs(T[r, m:n])
        T[r, enter] = -1.0
        tech = np.zeros(w)
        tech[col] = 1.0
        return tech.tolist(), float(T[r, -1]) - 1.0

    e1, e2 = m + 5, m + 9
    T[18, e1] = T[4, e2] = 0.0               # the first pivot leaves row 18 alone
    ops = [("add_activity", activity(200, m)),
           ("add_activity", activity(900, m)),
           ("add_constraint", cap(3, width + 2, e1)),
           ("add_constraint", cap(17, width + 3, e2)),
           ("resolve_all", ())]
    return base, ops, [(0, 0, 2, n), (1, 0, 2, n + 1), (2, 0, 2, e1), (3, 0, 2, e2)]


def stride_scripts():
    """[(name, base, ops, expect)]: every edit ends with outcome 0, and for each (op index, k,
    field, value) of `expect` the k-th log entry that edit appended holds `value` in `field`
    (0 kind, 1 leaving row, 2 entering column)."""
    out = []
    for mode in TIE_MODES:
        out.append((f"leave_rows_{mode}",) + leaving_rows_script(mode))
    out.append(("leave_rows_exact_gap1024",) + leaving_rows_script("exact", gap=1024))
    for mode in TIE_MODES:
        out.append((f"enter_cols_{mode}",) + entering_cols_script(mode, 80, 1200, 1124))
        out.append((f"argmin_cols_{mode}",) + argmin_cols_script(mode, 80, 1200, 1124))
    for mode in ("exact", "later_better_in_band", "later_better_out_of_band"):
        out.append((f"uncached_enter_{mode}",) + entering_cols_script(mode, 6, 16500, 1124))
        out.append((f"uncached_enter_{mode}_8strides",)
                   + entering_cols_script(mode, 6, 16500, 8 * 1024))
    for mode in ("exact", "later_better_in_band"):
        out.append((f"uncached_argmin_{mode}",)
                   + argmin_cols_script(mode, 6, 16500, 9 * 1024 + 300, r1=2, r2=5))
    out.append(("prefix_minima_step1",) + prefix_minima_script(1.0))
    out.append(("prefix_minima_in_band",) + prefix_minima_script(4e-10))
    out.append(("grow_tall",) + growth_script())
    return out


def same_state(dev, orc, tag):
    T, basic, sol = dev.read()
    st = orc.state()
    assert (T.shape == st["T"].shape), tag
    assert T.tobytes() == st["T"].tobytes(), tag
    assert basic.tolist() == st["basic"], tag
    assert sol.tobytes() == st["sol"].tobytes(), tag
    assert dev.shape()[4] == st["z"] or (math.isnan(st["z"]) and math.isnan(dev.shape()[4])), tag
    assert dev.log() == orc.log(), tag


def run_script(engine, oracle, name, base, ops):
    """Device analyzer and oracle side by side: same outcome and the same state after every
    edit.  Returns the outcome codes."""
    from lpr_381_group_v22_amd.engine import SensState
    T, x, z, basis = base
    o = oracle.sens(T, x, z, basis)
    d = SensState.create(engine, T, x, z)
    same_state(d, o, (name, "ctor"))
    codes = []
    for k, (op, args) in enumerate(ops):
        op, args = materialize(op, args, o.state()["T"], k)
        rc = getattr(o, op)(*args)
        oc = getattr(d, op)(*args)
        assert oc == rc, (name, k, op, oc, rc)
        same_state(d, o, (name, k, op))
        codes.append(rc)
    d.destroy()
    return codes
