"""Models and scripts for the tests of the scenario batch built from an LP batch (TEST ONLY;
lpr_sens_batch_from_batch).  A model is an (objective, constraints,
isMaximization) triple solved by the oracle's primal simplex; its base is the (T, x, z, basis) the
C# hands to `new SensitivityAnalyzer(...)` (Program.cs:147-151).  A script is an op list in the
style of sens_grow_cases.py: `sens_grow_cases.follow` fills in what depends on the shape along an
oracle run of the script alone on a fresh analyzer over that base, and that run is what a scenario
of the batch is compared with (sens_batch_cases.same_scenario)."""
from __future__ import annotations

import numpy as np

import lp_cases
import sens_grow_cases as grow

OPTIMAL, UNBOUNDED = 0, 1

# (m, n): the shapes the issue names and the column counts 63 / 64 / 65 around a wave
SHAPES = [(1, 1), (2, 3), (3, 2), (8, 12), (33, 64), (10, 52), (10, 53), (10, 54)]
# the LP of every scenario of the mixed batch: permuted, LP 2 under three different scripts
MIXED_ITEMS = [4, 0, 7, 2, 2, 6, 2, 1, 5, 3, 0]
# one model per kind of shape, each under every script of edit_ops
EVERY_OP_MODELS = [0, 1, 2, 3, 6]


def solve(oracle, model):
    """(status, (T, x, z, basis)) of the oracle's PrimalSimplexSolver on one model."""
    obj, cons, is_max = model
    o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
    T, basis = oracle.primal_build(o, A, rel, rhs, is_max, ncoef)
    st, _, _ = oracle.primal_solve(T, basis)
    x, z = oracle.extract_solution(T, len(obj))
    return st, (T, x, z, basis)


def solved(oracle, model):
    st, base = solve(oracle, model)
    assert st == OPTIMAL, st
    return base


def shape_models():
    return [lp_cases.random_dense(m, n, 300 + q) for q, (m, n) in enumerate(SHAPES)]


def rebuilt_basis(oracle, base):
    """basicVars of a fresh analyzer on the base: what the constructor's rebuild leaves."""
    return oracle.sens(*base).state()["basic"]


def edit_ops(oracle, base, seed):
    """Eight op lists for any base: every op 0..6, growth by 0, 1, 2 and 3 edits, an invalid index
    (-1), a constructed infeasible constraint (2), a constructed unbounded activity (1) and an RHS
    pushed negative (8 where the row has no negative entry)."""
    T = base[0]
    m, C = T.shape[0] - 1, T.shape[1]
    bset = set(rebuilt_basis(oracle, base))
    nonbasic = [j for j in range(C - 1) if j not in bset]
    basic = sorted(b for b in bset if b >= 0) or [0]
    return [
        [],
        [("resolve_all", ()), ("change_rhs", (1, float(T[1, -1]) + 3.0))],
        [("change_nonbasic_cbar", (nonbasic[0], -2.5)), ("change_basic", (basic[0], 0.75))],
        [("add_activity", grow.activity(seed)), ("change_rhs", (min(2, m), -5.0))],
        [("add_constraint", grow.constraint(seed + 1)), ("add_activity", grow.activity(seed + 2)),
         ("change_nonbasic_column", (1, nonbasic[-1], 0.5))],
        [("change_nonbasic_cbar", (10 ** 6, 1.0)), ("add_constraint_infeasible", ()),
         ("change_rhs", (1, 0.0))],
        [("add_activity_unbounded", ()), ("add_constraint", grow.constraint(seed + 3, 2.0)),
         ("add_constraint", grow.constraint(seed + 4, 0.5))],
        [("change_rhs", (1, -5.0)), ("change_rhs", (1, 2.0))],
    ]


def follow_all(oracle, bases, items, ops_list):
    """(scripts, refs, shapes): ops_list[k] followed alone on a fresh oracle analyzer over
    bases[items[k]]."""
    got = [grow.follow(oracle, bases[it], ops) for it, ops in zip(items, ops_list)]
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]


def mixed_case(oracle):
    """(models, bases, items, ops_list): every shape of SHAPES in one batch, the items permuted,
    LP 2 under three different scripts and LP 0 under two."""
    models = shape_models()
    bases = [solved(oracle, mdl) for mdl in models]
    ops_list = [edit_ops(oracle, bases[it], 400 + 10 * k)[(k + 1) % 8]
                for k, it in enumerate(MIXED_ITEMS)]
    return models, bases, list(MIXED_ITEMS), ops_list


def every_op_case(oracle):
    """(models, bases, items, ops_list): five models of differing shapes, each under all eight
    scripts of edit_ops, so final shapes differ on top of differing bases."""
    every = shape_models()
    models = [every[q] for q in EVERY_OP_MODELS]
    bases = [solved(oracle, mdl) for mdl in models]
    items, ops_list = [], []
    for it, base in enumerate(bases):
        for ops in edit_ops(oracle, base, 500 + 10 * it):
            items.append(it)
            ops_list.append(ops)
    return models, bases, items, ops_list


# ---- tableaux on which ExtractSolution and the rebuild see different things -----------------------
# Each is a ready final tableau with cols >= rows and row 0 >= 0, so a PrimalSimplexBatch made with
# from_tableaux is optimal after Solve() without a pivot; n = cols - rows decision columns.
def _blank(m, cols, seed):
    rng = np.random.RandomState(seed)
    T = np.zeros((m + 1, cols))
    T[0, :-1] = rng.uniform(0.5, 2.0, size=cols - 1)
    T[1:, -1] = rng.uniform(1.0, 9.0, size=m)
    T[0, -1] = 42.5
    return T


def twin_unit_columns():
    """Columns 1 (decision) and 5 are the same unit column of row 2: the rebuild takes the first,
    ExtractSolution reports x1 = b2.  Row 3 has no unit column (basicVars[2] = -1).  Row 1 is basic
    in column 0 with RHS 0: a degenerate optimum."""
    T = _blank(3, 9, 601)
    T[1, 0] = 1.0
    T[1, -1] = 0.0
    T[2, 1] = T[2, 5] = 1.0
    T[0, 0] = T[0, 1] = T[0, 5] = 0.0
    T[3, 2:5] = [0.5, -0.25, 2.0]
    T[1, 3], T[2, 4] = 0.75, -0.5
    return T


def two_ones_in_a_column():
    """Decision column 0 holds 1 and 1 + 5e-10, column 1 holds 1 - 5e-10 twice: ExtractSolution
    meets a second 1 and gives 0; no row takes either column.  Column 2 is a plain unit column."""
    T = _blank(3, 8, 602)
    T[1, 0], T[2, 0] = 1.0, 1.0 + 5e-10
    T[2, 1], T[3, 1] = 1.0 - 5e-10, 1.0 - 5e-10
    T[3, 2] = 1.0
    T[0, 2] = 0.0
    T[1, 5], T[2, 6] = 1.0, 1.0
    return T


def threshold_entries():
    """One decision column per value around both 1e-9 thresholds.  Columns 0..5: the value in row 1
    is 1 +- 1e-9 or one ulp either side of those, alone in its column.  Columns 6..11: 1.0 in row
    2 and, in row 3, +-1e-9 or one ulp either side of it."""
    eps = 1e-9
    ones = [1.0 + eps, np.nextafter(1.0 + eps, 0.0), np.nextafter(1.0 + eps, 2.0),
            1.0 - eps, np.nextafter(1.0 - eps, 0.0), np.nextafter(1.0 - eps, 2.0)]
    smalls = [eps, np.nextafter(eps, 0.0), np.nextafter(eps, 1.0),
              -eps, -np.nextafter(eps, 0.0), -np.nextafter(eps, 1.0)]
    T = _blank(3, 16, 603)           # n = 12
    for q, v in enumerate(ones):
        T[1, q] = v
    for q, w in enumerate(smalls):
        T[2, 6 + q] = 1.0
        T[3, 6 + q] = w
    T[3, 14] = 1.0
    return T


def disagreement_tableaux():
    return [("twin_unit_columns", twin_unit_columns()),
            ("two_ones_in_a_column", two_ones_in_a_column()),
            ("threshold_entries", threshold_entries())]


def tableau_base(oracle, T):
    """The base the C# would hand to the analyzer for a ready final tableau: ExtractSolution over
    n = cols - rows and T[0, cols - 1]; the basis argument is rebuilt by the constructor."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    x, z = oracle.extract_solution(T.copy(), T.shape[1] - T.shape[0])
    return T, x, z, np.zeros(T.shape[0] - 1, dtype=np.int32)


def tableau_ops(T):
    return [[], [("resolve_all", ())], [("change_rhs", (1, 1.25))],
            [("add_constraint", grow.constraint(611)), ("add_activity", grow.activity(612))]]


# ---- forms ---------------------------------------------------------------------------------------
def large_model():
    """A 200 x 300 tableau: past form G's LDS, so a batch that holds it runs in form H."""
    return lp_cases.random_dense(199, 100, 77)


def forms_case(oracle):
    """(models, bases, items, ops_list, shared): textbook models plus large_model() as the last
    one; the scenarios listed in `shared` use only the textbook models."""
    every = shape_models()
    models = [every[1], every[2], every[3], large_model()]
    bases = [solved(oracle, mdl) for mdl in models]
    items = [0, 1, 2, 2, 1, 0, 3, 3]
    pick = [1, 3, 4, 7, 6, 2]
    ops_list = [edit_ops(oracle, bases[it], 700 + 10 * k)[pick[k]]
                for k, it in enumerate(items[:6])]
    b1 = float(bases[3][0][1, -1])
    ops_list += [[], [("change_rhs", (1, b1 + 3.0)), ("add_activity", grow.activity(771))]]
    return models, bases, items, ops_list, list(range(6))


# ---- refusals --------------------------------------------------------------------------------------
def unbounded_model():
    return lp_cases.unbounded_lp()


def many_pivot_model():
    """More than one pivot on the oracle: Solve(max_pivots=1) leaves it at its pivot limit."""
    return lp_cases.random_dense(8, 12, 303)


def tall_tableau():
    """cols < rows: lpr_batch_create takes it, an analyzer does not."""
    T = np.zeros((4, 3))
    T[0, :2] = 1.0
    T[1:, -1] = [1.0, 2.0, 3.0]
    T[1, 0] = T[2, 1] = 1.0
    return T


def wide_optimal_tableau():
    """A 3 x 2048 final tableau, optimal as it stands: one more column is past form H."""
    T = np.zeros((3, 2048))
    T[0, :-1] = 1.0
    T[0, 0] = T[0, 1] = 0.0
    T[1, 0] = T[2, 1] = 1.0
    T[1:, -1] = [2.0, 3.0]
    return T
