"""Non-finite and extreme-magnitude test data (TEST ONLY): the value classes, the NaN-aware parity
comparator of DESIGN.md section 2, seeded generators that plant the values into otherwise ordinary
cases (ready tableaux for the primal solver, (c, A, b) for the revised one, B&B start tableaux,
cut / dual / primal2 tableaux, sensitivity edit scripts), and a planter that puts a value into the pivot row / pivot column of a chosen later pivot of a
larger case.  Shared by test_special_values_cpu.py (oracle against the
Python restatements, and the coverage conditions) and test_special_values_gpu.py (device against
the oracle)."""
from __future__ import annotations

import math
import struct

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
MIN_NORMAL = float(np.finfo(np.float64).tiny)
EPS9 = 1e-9

# name -> value.  The last four feed the B&B rounding helpers (Math.Round's 1e16 cut, the int
# range); they are planted like the others.
CLASSES = {
    "+inf": math.inf, "-inf": -math.inf, "nan": math.nan, "-0": -0.0,
    "+denorm_min": 5e-324, "-denorm_min": -5e-324, "min_normal": MIN_NORMAL,
    "+1e308": 1e308, "-1e308": -1e308, "+dbl_max": DBL_MAX, "-dbl_max": -DBL_MAX, "1e-300": 1e-300,
    "eps": EPS9, "eps+ulp": float(np.nextafter(EPS9, math.inf)),
    "eps-ulp": float(np.nextafter(EPS9, -math.inf)),
    "-eps": -EPS9, "-eps-ulp": -float(np.nextafter(EPS9, math.inf)),
    "-eps+ulp": -float(np.nextafter(EPS9, -math.inf)),
    "1e16": 1e16, "2^31-0.5": 2.0 ** 31 - 0.5, "2^31+0.5": 2.0 ** 31 + 0.5,
}
NAMES = list(CLASSES)
VALUES = [CLASSES[k] for k in NAMES]


def bits(x) -> str:
    return struct.pack(">d", float(x)).hex()


# ------------------------------------------------------------------------------------------------
# The comparator: NaN positions identical, every other element identical in
# all 64 bits (sign of zero, +-inf included).  NaN sign / payload bits are outside parity.
# ------------------------------------------------------------------------------------------------
def same(a, b) -> bool:
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    ua = np.where(na, np.uint64(0), a.view(np.uint64))
    ub = np.where(nb, np.uint64(0), b.view(np.uint64))
    return bool(np.array_equal(ua, ub))


def first_difference(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        return "shapes %r / %r" % (a.shape, b.shape)
    for k in range(a.size):
        if not same(a[k], b[k]):
            return "element %d: %r (%s) / %r (%s)" % (k, a[k], bits(a[k]), b[k], bits(b[k]))
    return None


def assert_same(a, b, what="") -> None:
    assert same(a, b), (what, first_difference(a, b))


def has_nan(a) -> bool:
    return bool(np.isnan(a).any())


def has_inf(a) -> bool:
    return bool(np.isinf(a).any())


def holds(a, v) -> bool:
    """Does array a hold the value class v (NaN: any NaN; else the exact bits)?"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if v != v:
        return has_nan(a)
    return bool((a.view(np.uint64) == np.float64(v).view(np.uint64)).any())


# ------------------------------------------------------------------------------------------------
# Ready tableaux for the primal solver
# ------------------------------------------------------------------------------------------------
def clean_tableau(rng, m, n):
    """An ordinary (m + 1) x (n + m + 1) start tableau: row 0 = -c, slack identity, b > 0; about
    a third of the constraint entries negative so that unbounded directions exist."""
    T = np.zeros((m + 1, n + m + 1))
    T[0, :n] = -np.round(rng.uniform(0.1, 3.0, size=n), 3)
    A = np.round(rng.uniform(-0.6, 2.0, size=(m, n)), 3)
    T[1:, :n] = A
    T[1:, n:n + m] = np.eye(m)
    T[1:, -1] = np.round(rng.uniform(1.0, 9.0, size=m), 3)
    return T, np.arange(n, n + m, dtype=np.int32)


def first_entering(T) -> int:
    """FindEnteringVariable (:152-167) on row 0: the first most negative entry, -1 if none."""
    row = T[0, :-1]
    col, best = -1, 0.0
    for j in range(row.size):
        if row[j] < best:
            best, col = row[j], j
    return col


def plant_small(rng, T, count):
    """count entries of T replaced by values drawn from the classes.  Where the value goes: the
    first entering column (so it is a factor or the pivot of the first pivot), the Z row, the RHS
    column, or anywhere."""
    R, C = T.shape
    planted = []
    e = first_entering(T)
    for _ in range(count):
        v = VALUES[int(rng.randint(len(VALUES)))]
        where = int(rng.randint(10))
        if where < 4 and e >= 0:
            i, j = int(rng.randint(1, R)), e
        elif where < 6:
            i, j = 0, int(rng.randint(C - 1))
        elif where < 7:
            i, j = int(rng.randint(1, R)), C - 1
        else:
            i, j = int(rng.randint(R)), int(rng.randint(C))
        T[i, j] = v
        planted.append((i, j, v))
    return planted


FUZZ_SEED = 0       # picked on the CPU so that the oracle alone meets the conditions of
FUZZ_COUNT = 300    # test_special_values_cpu.py::test_small_fuzz_is_not_vacuous
FUZZ_CAP = 64       # pivots per case (a NaN-ridden tableau may cycle)


def primal_fuzz(count=FUZZ_COUNT, seed=FUZZ_SEED):
    """[(T, basis, planted)]: R <= 9, C <= 18, one to three planted entries each."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        m = int(rng.randint(2, 9))
        n = int(rng.randint(2, 18 - m))
        T, basis = clean_tableau(rng, m, n)
        planted = plant_small(rng, T, int(rng.randint(1, 4)))
        out.append((T, basis, planted))
    return out


def oracle_primal(oracle, T, basis, n, max_pivots=FUZZ_CAP):
    """One oracle run on copies: dict(T0, T, basis, status, pivots, log, x, z)."""
    T = np.ascontiguousarray(T, dtype=np.float64).copy()
    T0 = T.copy()
    basis = np.ascontiguousarray(basis, dtype=np.int32).copy()
    st, piv, log = oracle.primal_solve(T, basis, max_pivots)
    x, z = oracle.extract_solution(T, n)
    return dict(T0=T0, T=T, basis=basis, status=st, pivots=piv, log=log, x=x, z=z)


def step_oracle(oracle, T, max_pivots):
    """The oracle's loop one call at a time on a copy of T: yields (q, r, e, pivot row before the
    pivot, pivot column before the pivot, T) for every pivot."""
    T = np.ascontiguousarray(T, dtype=np.float64).copy()
    for q in range(max_pivots):
        e = oracle.find_entering(T)
        if e < 0:
            return
        r = oracle.find_leaving(T, e)
        if r < 0:
            return
        yield q, r, e, T[r].copy(), T[:, e].copy(), T
        oracle.pivot(T, r, e)


def constructed_primal():
    """{name: (T, basis, n)}: a few rows each, one special-value mechanism per case (the
    expectations that do not need an oracle are asserted in test_special_values_cpu.py)."""
    inf, nan = math.inf, math.nan
    up, dn = CLASSES["eps+ulp"], CLASSES["eps-ulp"]
    d = {}
    # inf in the pivot row (row 1, column 1); rows 2 and 3 have factor +0 / -0 in the entering
    # column 0: 0 * inf = NaN there, while the Z row (factor -1) gets 0.5 - (-1 * inf) = +inf
    d["inf_in_pivot_row_zero_factors"] = (np.array(
        [[-1.0, 0.5, 0.0, 0.0, 0.0, 0.0],
         [2.0, inf, 1.0, 0.0, 0.0, 4.0],
         [0.0, 3.0, 0.0, 1.0, 0.0, 5.0],
         [-0.0, -2.0, 0.0, 0.0, 1.0, 6.0]]), [2, 3, 4], 2)
    # the Z row's factor is never 0 for the entering column, so the Z row takes its NaN one pivot
    # later: row 2 (factor 0) turns NaN in column 2 at the first pivot and is the second pivot row
    d["inf_in_pivot_row_z_row_nan"] = (np.array(
        [[-2.0, -1.0, 0.0, 0.0, 0.0, 0.0],
         [1.0, 0.0, inf, 1.0, 0.0, 4.0],
         [0.0, 1.0, 0.0, 0.0, 1.0, 5.0]]), [3, 4], 2)
    # NaN and -0.0 in the Z row never enter; -5e-324 does (strict < 0)
    d["z_row_nan_negzero_denorm"] = (np.array(
        [[nan, -0.0, -5e-324, 0.0, 0.0, 0.0],
         [1.0, 1.0, 2.0, 1.0, 0.0, 4.0],
         [1.0, 1.0, 4.0, 0.0, 1.0, 4.0]]), [3, 4], 3)
    d["z_row_only_nan_negzero"] = (np.array(
        [[nan, -0.0, 0.0, 0.0, 0.0],
         [1.0, 1.0, 1.0, 0.0, 4.0],
         [1.0, 1.0, 0.0, 1.0, 4.0]]), [2, 3], 2)
    # entering-column entries at 1e-9 and one ulp either side: only the one above is a candidate
    # (a > 1e-9), although the other two rows would give smaller ratios
    d["entering_entry_at_eps"] = (np.array(
        [[-1.0, 0.0, 0.0, 0.0, 0.0],
         [EPS9, 1.0, 0.0, 0.0, 1e-12],
         [dn, 0.0, 1.0, 0.0, 1e-12],
         [up, 0.0, 0.0, 1.0, 3.0]]), [1, 2, 3], 1)
    d["entering_entries_all_at_or_below_eps"] = (np.array(
        [[-1.0, 0.0, 0.0, 1.0],
         [EPS9, 1.0, 0.0, 1.0],
         [dn, 0.0, 1.0, 1.0]]), [1, 2], 1)
    # f * p overflows (1e200 * 1e200), then inf - inf: row 2 has +inf already in column 1
    d["product_overflows_then_inf_minus_inf"] = (np.array(
        [[-1.0, 0.0, 0.0, 0.0, 0.0, 0.0],
         [1.0, 1e200, 1.0, 0.0, 0.0, 2.0],
         [1e200, inf, 0.0, 1.0, 0.0, 1e300],
         [-1e200, 1e150, 0.0, 0.0, 1.0, 7.0]]), [2, 3, 4], 2)
    # subnormal RHS over ordinary entries: subnormal ratios; rows 1 and 3 tie (10e-324 / 2 ==
    # 5e-324 / 1 after rounding): the lower row leaves
    d["subnormal_ratios_tie_lower_row"] = (np.array(
        [[-1.0, 0.0, 0.0, 0.0, 0.0],
         [2.0, 1.0, 0.0, 0.0, 1e-323],
         [1.0, 0.0, 1.0, 0.0, 1.5e-323],
         [1.0, 0.0, 0.0, 1.0, 5e-324]]), [1, 2, 3], 1)
    # a pivot element just above 1e-9: normalising the row overflows (1e308 / 2e-9 = +inf)
    d["tiny_pivot_row_overflows"] = (np.array(
        [[-1.0, -0.5, 0.0, 0.0, 0.0],
         [2e-9, 1e308, 1.0, 0.0, 1e-12],
         [1.0, 1.0, 0.0, 1.0, 3.0]]), [2, 3], 2)
    # NaN RHS: NaN ratio, the row is skipped and row 2 leaves; in the
    # second case the NaN is the basic value of x1 and ExtractSolution (:213-252) returns it
    d["nan_rhs_row_skipped_then_basic"] = (np.array(
        [[-3.0, -1.0, 0.0, 0.0, 0.0, 0.0],
         [1.0, 0.0, 1.0, 0.0, 0.0, nan],
         [2.0, 1.0, 0.0, 1.0, 0.0, 8.0],
         [0.0, 1.0, 0.0, 0.0, 1.0, 3.0]]), [2, 3, 4], 2)
    d["nan_rhs_in_basic_row_of_a_decision_variable"] = (np.array(
        [[0.0, -1.0, 0.0, 0.0, 0.0],
         [1.0, 0.0, 1.0, 0.0, nan],
         [0.0, 2.0, 0.0, 1.0, 8.0]]), [0, 3], 2)
    return {k: (np.array(T, dtype=np.float64), np.array(b, dtype=np.int32), n)
            for k, (T, b, n) in d.items()}


# ------------------------------------------------------------------------------------------------
# The planter for larger shapes
# ------------------------------------------------------------------------------------------------
STRIP = 512  # columns per sweep strip of the K-pivot paths (256 lanes x double2)


def last_strip_start(cols) -> int:
    return ((cols - 1) // STRIP) * STRIP


def _nonfinite_or(v):
    if math.isfinite(v):
        return lambda a: bool((~np.isfinite(a)).any()) or holds(a, v)
    return lambda a: bool((~np.isfinite(a)).any())


def check_in_block(oracle, T, value, block=16, follow=16, cap=400):
    """Steps the oracle on T: (index q of the first pivot whose pivot row or pivot column holds
    the planted value or a non-finite value, pivots made in all), or (-1, pivots)."""
    hit = _nonfinite_or(value)
    first, made = -1, 0
    for q, r, e, prow, pcol, _ in step_oracle(oracle, T, cap):
        made = q + 1
        if first < 0 and (hit(prow) or hit(pcol)):
            first = q
        if first >= 0 and made > first + follow + 1:
            break
    return first, made


def plant_in_block(oracle, T0, log, value, prefer="row", block=16, follow=16, min_row=64):
    """Plants `value` into a copy of the clean start tableau T0 so that it is in the pivot row (a
    slack column of the last column strip, in the row of a later pivot) or in the pivot column (a
    row >= min_row, where the entering column lies in the last strip) of a pivot that is not the
    first of its block of `block`, with at least `follow` pivots after it.  log: the clean case's
    pivot log from the oracle.  Candidates are tried in pivot order, the preferred kind first;
    each is verified by stepping the oracle.  Returns (T, (i, j), q, kind)."""
    R, C = T0.shape
    lo = last_strip_start(C)
    if R <= min_row + 1:
        min_row = 1
    rows = [int(r) for r, _ in log]
    cols = [int(c) for _, c in log]
    order = list(range(block + 1, len(rows))) + list(range(1, block))  # later blocks first
    for kind in (prefer, "col" if prefer == "row" else "row"):
        for q in order:
            if q % block == 0:
                continue
            r, e = rows[q], cols[q]
            pos = None
            if kind == "row" and r >= min_row:
                # pivot-row entry: a zero of a slack column near the right edge
                for j in range(C - 2, lo - 1, -1):
                    if T0[r, j] == 0.0 and j not in cols[:q + 1]:
                        pos = (r, j)
                        break
            if kind == "col" and e >= lo:
                # pivot-column entry in a row that has not been a pivot row so far
                for i in range(R - 1, min_row - 1, -1):
                    if i not in rows[:q + 1]:
                        pos = (i, e)
                        break
            if pos is None:
                continue
            T = T0.copy()
            T[pos] = value
            first, made = check_in_block(oracle, T, value, block, follow)
            if first >= 0 and first % block != 0 and made >= first + 1 + follow:
                return T, pos, first, kind
    raise AssertionError("no position puts %r inside a block" % (value,))


IN_BLOCK_SHAPES = ((300, 700), (600, 50), (8, 3000))   # ov_step_cases.SHAPES: two head
IN_BLOCK_VALUES = (math.inf, math.nan, 1e308)          # workgroups / further rows / repeated rows
IN_BLOCK_PREFER = {bits(math.inf): "row", bits(math.nan): "col", bits(1e308): "col"}
IN_BLOCK_CAP = 400
_IN_BLOCK = {}


def in_block_case(oracle, m, n, value):
    """(T0, basis0, (i, j), q, kind) for one shape and planted value, computed once."""
    import lp_cases
    import ov_step_cases
    key = (m, n, bits(value))
    if key not in _IN_BLOCK:
        obj, cons, is_max = ov_step_cases.case(m, n, "optimal")
        o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
        T0, b0 = oracle.primal_build(o, A, rel, rhs, is_max, ncoef)
        T, b = T0.copy(), b0.copy()
        _, _, log = oracle.primal_solve(T, b, IN_BLOCK_CAP)
        Tp, pos, q, kind = plant_in_block(oracle, T0, log.tolist(), value,
                                          IN_BLOCK_PREFER[bits(value)])
        _IN_BLOCK[key] = (Tp, b0, pos, q, kind)
    return _IN_BLOCK[key]


_IN_BLOCK_REF = {}


def in_block_reference(oracle, m, n, value, legs):
    """(T0, basis0, [(status, pivots, log, basis, T) after each leg]) on the oracle, once."""
    key = (m, n, bits(value), legs)
    if key not in _IN_BLOCK_REF:
        T0, b0, _, _, _ = in_block_case(oracle, m, n, value)
        T, basis = T0.copy(), b0.copy()
        states = []
        for leg in legs:
            st, piv, log = oracle.primal_solve(T, basis, leg)
            states.append((st, piv, log.tolist(), basis.tolist(), T.copy()))
            if st != 5:
                break
        _IN_BLOCK_REF[key] = (T0, b0, states)
    return _IN_BLOCK_REF[key]


# ------------------------------------------------------------------------------------------------
# (c, A, b) for the revised solver
# ------------------------------------------------------------------------------------------------
REVISED_SHAPES = ((5, 3), (17, 33), (40, 70))   # (m, n)
REVISED_PER_SHAPE = 10
REVISED_SEED = 0
REVISED_CAP = 40


def revised_fuzz(seed=REVISED_SEED):
    """[(name, c, A, b)]: dense positive LPs with one to three entries of A, b and c replaced."""
    rng = np.random.RandomState(seed)
    out = []
    for (m, n) in REVISED_SHAPES:
        for k in range(REVISED_PER_SHAPE):
            A = np.round(rng.uniform(0.1, 2.0, size=(m, n)), 3)
            b = np.round(rng.uniform(5.0, 10.0, size=m), 3)
            c = np.round(rng.uniform(0.5, 2.0, size=n), 3)
            for _ in range(int(rng.randint(1, 4))):
                v = VALUES[int(rng.randint(len(VALUES)))]
                where = int(rng.randint(4))
                if where < 2:
                    A[int(rng.randint(m)), int(rng.randint(n))] = v
                elif where == 2:
                    b[int(rng.randint(m))] = v
                else:
                    c[int(rng.randint(n))] = v
            out.append(("fuzz_%dx%d_%d" % (m, n, k), c, A, b))
    return out


def constructed_revised():
    """[(name, c, A, b)], RevisedPrimalSimplexSolver.cs line numbers in the comments."""
    inf, nan = math.inf, math.nan
    up, dn = CLASSES["eps+ulp"], CLASSES["eps-ulp"]
    out = []
    # Iteration 1: x1 enters, row 0 leaves, eta factors -1e10 in rows 1 and 2.  Iteration 2: x2 has
    # reduced cost 1 - (3 * -1e308) = +inf (:96-102) and direction u = (-1e308, +inf, +inf, 5e307);
    # rows 1 and 2 tie at ratio 0, row 1 leaves with pivot +inf.  UpdateBInverse (:264-275): the
    # eta factor of row 2 is -inf / inf = NaN and must NOT be skipped by `|a_ik| < EPS` (:436),
    # while 1 / inf = 0 (the pivot row: zeroed), 1e308 / inf = 0 and -5e307 / inf = -0 are.
    out.append(("nan_and_sub_eps_eta_inf_reduced_cost",
                np.array([3.0, 1.0]),
                np.array([[1.0, -1e308], [1e10, 1.0], [1e10, 1.0], [0.5, 1.0]]),
                np.array([1.0, 5e10, 7e10, 4.0])))
    # x_B = B^-1 b (:89) sums 0 * inf and 0 * NaN: every basic value and so every ratio
    # (:154-176) is NaN, neither comparison holds, no row leaves: "unbounded"
    out.append(("nan_ratios_from_inf_and_nan_rhs",
                np.array([2.0, 1.0]),
                np.array([[1.0, 1.0], [2.0, 1.0], [1.0, 3.0]]),
                np.array([inf, nan, 6.0])))
    # 1e308 / 1e-8 = +inf: a ratio that is not below double.MaxValue, so row 1 leaves
    out.append(("inf_ratio_from_overflow",
                np.array([1.0, 0.5]),
                np.array([[1e-8, 1.0], [1.0, 1.0]]),
                np.array([1e308, 4.0])))
    # direction entries at 1e-9 and one ulp either side (u_i > EPS :158): only the one above is a
    # candidate, and its pivot passes `|pivot| < EPS` (:266-267), which no ratio-test winner fails
    out.append(("pivot_at_eps_plus_ulp",
                np.array([1.0, 0.5]),
                np.array([[EPS9, 1.0], [dn, 1.0], [up, 1.0]]),
                np.array([1e10, 1e10, 5.0])))
    out.append(("direction_at_or_below_eps_is_unbounded",
                np.array([1.0, -1.0]),
                np.array([[EPS9, 1.0], [dn, 1.0]]),
                np.array([1.0, 1.0])))
    # subnormal right-hand sides and an overflowing cost
    out.append(("subnormal_rhs_dbl_max_cost",
                np.array([DBL_MAX, 1.0, 5e-324]),
                np.array([[1.0, 2.0, 1.0], [3.0, 1.0, 1.0]]),
                np.array([5e-324, 1e-323])))
    return out


def revised_cases():
    return constructed_revised() + revised_fuzz()


# ------------------------------------------------------------------------------------------------
# Branch & Bound: the rounding helpers on the value classes
# ------------------------------------------------------------------------------------------------
def rounding_tableau():
    """An 8 x 8 array (not a simplex tableau; lpr_bb_create takes any rows x cols) that holds every
    value class, its neighbours one ulp away where finite, and 4-decimal midpoints; columns 0 and 1
    hold a 1.0 each, so that nvars = 2 reads two decision values (one of them NaN's row)."""
    vals = list(VALUES)
    vals += [float(np.nextafter(v, math.inf)) for v in (1e16, 2.0 ** 31 - 0.5, 2.0 ** 31 + 0.5)]
    vals += [float(np.nextafter(v, -math.inf)) for v in (1e16, 2.0 ** 31 - 0.5, 2.0 ** 31 + 0.5)]
    vals += [-1e16, -(2.0 ** 31) - 0.5, 0.00005, 0.00015, -0.00025, 2.5, 1e15 + 0.5, 4503599627370497.0]
    vals += [0.12345, 12345.67895, 0.49999999999999994, 9.2e18, 1e300, -1e-300, 3.5]
    T = np.zeros((8, 8))
    assert len(vals) <= 48
    T.reshape(-1)[:len(vals)] = vals
    T[7, 0] = 1.0
    T[6, 1] = 1.0
    T[6, 7] = math.nan
    T[7, 7] = 1e308
    return T


# ------------------------------------------------------------------------------------------------
# Branch & Bound start tableaux
# ------------------------------------------------------------------------------------------------
BB_VALUES = (math.inf, -math.inf, math.nan, 1e308)
BB_NODE_CAP = 12
# NaN in the Z row over the basic column of row 2: the primal phase of DoDualSimplex, a
# `while (true)` without an iteration cap (:352), leaves on `All(num => num >= 0)` (:368-373),
# which the NaN keeps false; neither restatement returns
BB_NON_TERMINATING = {("nan", 0, 5)}


def bb_start_tableaux(oracle):
    """[(name, T, nvars)]: the final tableau of bb_cases.fractional_program(4, 2, 10) with one
    entry replaced, every position and every value of BB_VALUES."""
    import bb_cases
    st, T0, n = bb_cases.primal_final_tableau(oracle, *bb_cases.fractional_program(4, 2, 10))
    assert st == 0 and T0.shape == (7, 11)
    out = []
    for v in BB_VALUES:
        tag = "nan" if v != v else repr(v)
        for i in range(T0.shape[0]):
            for j in range(T0.shape[1]):
                if (tag, i, j) in BB_NON_TERMINATING:
                    continue
                T = T0.copy()
                T[i, j] = v
                out.append(("%s@%d,%d" % (tag, i, j), T, n))
    return out


def same_records(a, b) -> bool:
    """B&B node records: integers exactly, z and bound with the comparator."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        for k in x:
            if k in ("z", "bound"):
                if not same(x[k], y[k]):
                    return False
            elif x[k] != y[k]:
                return False
    return True


def bb_probe(T, n):
    """The restatement's search on T with every pivot of every child inspected before it is made
    (its trace is asserted equal to the oracle's in test_special_values_cpu.py): returns
    (row_hit, col_hit).  row_hit: some pivot's normalised pivot row is non-finite while another
    row has factor exactly 0 (the `nonfinite` vote of k_bb_select: 0 * inf must give NaN, so the
    zero-factor rows cannot be left out).  col_hit: some pivot has a non-finite factor."""
    from ref_py_bb import BranchAndBound, DualSimplexSolverBB, _div
    hits = [False, False]

    def look(tab, trace_len, solver):
        if len(solver.trace) == trace_len:
            return
        _, pr, pc = solver.trace[-1]
        p = tab[pr][pc]
        prow = [_div(v, p) for v in tab[pr]]
        factors = [tab[i][pc] for i in range(len(tab)) if i != pr]
        if any(not math.isfinite(v) for v in prow) and any(f == 0.0 for f in factors):
            hits[0] = True
        if any(not math.isfinite(f) for f in factors):
            hits[1] = True

    class Probe(DualSimplexSolverBB):
        def PerformDualPivot(self, tableau):
            k = len(self.trace)
            out = DualSimplexSolverBB.PerformDualPivot(self, tableau)
            look(tableau, k, self)
            return out

        def PerformPrimalPivot(self, tableau):
            k = len(self.trace)
            out = DualSimplexSolverBB.PerformPrimalPivot(self, tableau)
            look(tableau, k, self)
            return out

    bb = BranchAndBound(n, node_cap=BB_NODE_CAP)
    bb.solver = Probe()
    bb.Execute([list(map(float, row)) for row in T.tolist()])
    return hits[0], hits[1]


_BB_DEVICE = {}


def bb_device_cases(oracle, per_kind=10):
    """The start tableaux the device runs: up to per_kind with a row hit, as many with a column
    hit (bb_probe), and every 25th of the rest.  [(name, T, nvars, row_hit, col_hit)], once."""
    if "cases" not in _BB_DEVICE:
        rows, cols, rest = [], [], []
        for k, (name, T, n) in enumerate(bb_start_tableaux(oracle)):
            rh, ch = bb_probe(T, n)
            item = (name, T, n, rh, ch)
            if rh and len(rows) < per_kind:
                rows.append(item)
            elif ch and len(cols) < per_kind:
                cols.append(item)
            elif k % 25 == 0:
                rest.append(item)
        _BB_DEVICE["cases"] = rows + cols + rest
    return _BB_DEVICE["cases"]


# ------------------------------------------------------------------------------------------------
# Cut, dual and primal2 tableaux (row 0 = objective row)
# ------------------------------------------------------------------------------------------------
CUT_VALUES = (math.inf, -math.inf, math.nan, 1e308, -1e308, DBL_MAX, 5e-324, -5e-324, -0.0,
              CLASSES["eps+ulp"], CLASSES["eps-ulp"], CLASSES["-eps-ulp"], CLASSES["-eps+ulp"])
CUT_HARD_CAP = 200


def _planted_copies(name, T0, rng, count, have):
    """count copies of T0 with one or two entries replaced; the first value of every copy goes
    round CUT_VALUES (have: copies made so far), so that a family holds every value."""
    out = []
    for k in range(count):
        T = T0.copy()
        for q in range(int(rng.randint(1, 3))):
            v = CUT_VALUES[(have + k) % len(CUT_VALUES) if q == 0 else
                           int(rng.randint(len(CUT_VALUES)))]
            T[int(rng.randint(T.shape[0])), int(rng.randint(T.shape[1]))] = v
        out.append(("%s_p%d" % (name, k), T))
    return out


def _first_dual_row(T):
    """The first leaving row of DualSimplexSolver.Solve on a finite tableau: the most negative
    right-hand side."""
    rhs = T[1:, -1]
    return 1 + int(np.argmin(rhs)) if rhs.min() < -EPS9 else -1


def cut_planted(oracle):
    """{"dual" | "primal2" | "cut": [(name, T)]}: small cut_cases tableaux with planted values,
    seeded, and constructed ones that put a +inf and a NaN candidate ratio into the ratio tests
    (DualSimplexSolver.Solve DualSimplex.cs:14-114, PrimalSimplexSolver2.Solve :46-97,
    CuttingPlaneSolution CuttingPlaneSolver.cs:64-229) and a NaN fractional part into the cut's
    source row (Frac, CuttingPlaneSolver.cs:12-17).  A NaN ratio cannot arise in the cut's own ratio
    test: its numerator passes `|num| > EPS` and its divisor is a fractional part in (-1, 0).  The
    seeded copies put the values into the two arg-min selections (most negative right-hand side,
    most negative cost) as well."""
    import cut_cases
    rng = np.random.RandomState(7)
    inf, nan = math.inf, math.nan
    out = {"dual": [], "primal2": [], "cut": []}
    small = lambda cases: [(k, T) for k, T in cases if T.size <= 600]
    for name, T0 in small(cut_cases.dual_tableaux(oracle)):
        out["dual"] += _planted_copies(name, T0, rng, 4, len(out["dual"]))
        r = _first_dual_row(T0)
        neg = [j for j in range(T0.shape[1] - 1) if T0[r, j] < -EPS9 and abs(T0[0, j]) > EPS9]
        if r > 0 and len(neg) >= 2:
            T = T0.copy()
            T[0, neg[0]] = inf                  # ratio |inf / a| = +inf
            T[0, neg[1]] = inf
            T[r, neg[1]] = -inf                 # ratio |inf / -inf| = NaN
            out["dual"].append((name + "_inf_and_nan_ratio", T))
            T = T0.copy()
            T[r, -1] = -inf                     # the leaving-row selection meets -inf
            T[(r % (T.shape[0] - 1)) + 1, -1] = nan
            out["dual"].append((name + "_inf_and_nan_rhs", T))
    for name, T0 in small(cut_cases.primal2_tableaux(oracle)):
        out["primal2"] += _planted_copies(name, T0, rng, 4, len(out["primal2"]))
        pc = int(np.argmin(T0[0, :-1]))
        pos = [i for i in range(1, T0.shape[0]) if T0[i, pc] > EPS9]
        if len(pos) >= 3:
            T = T0.copy()
            T[pos[0], -1] = inf                 # ratio +inf
            T[pos[1], -1] = nan                 # ratio NaN
            out["primal2"].append((name + "_inf_and_nan_ratio", T))
            T = T0.copy()
            T[0, pc] = -inf                     # the entering-column selection meets -inf, NaN
            T[0, (pc + 1) % (T.shape[1] - 1)] = nan
            out["primal2"].append((name + "_inf_and_nan_cost", T))
    for name, T0 in small(cut_cases.cutting_plane_tableaux(oracle)):
        out["cut"] += _planted_copies(name, T0, rng, 3, len(out["cut"]))
        fr = T0[1:, -1] - np.floor(T0[1:, -1])
        ok = np.where((fr > 1e-6) & (fr < 1 - 1e-6))[0]
        if ok.size:
            src = 1 + int(ok[np.argmin(np.abs(fr[ok] - 0.5))])   # the cut's source row
            cols = [j for j in range(T0.shape[1] - 1)
                    if 1e-6 < T0[src, j] - math.floor(T0[src, j]) < 1 - 1e-6]
            if len(cols) >= 2:
                T = T0.copy()
                T[0, cols[0]] = inf             # cut ratio +inf
                out["cut"].append((name + "_inf_ratio", T))
                T = T0.copy()
                T[src, cols[0]] = inf           # frac(inf) = inf - inf = NaN in the source row
                T[src, cols[1]] = nan
                out["cut"].append((name + "_nan_fractional_part", T))
    return out


# ------------------------------------------------------------------------------------------------
# Sensitivity edit scripts with special arguments
# ------------------------------------------------------------------------------------------------
SENS_VALUES = (math.inf, -math.inf, math.nan, 1e308, -1e308, -0.0, 5e-324)


def sens_scripts(oracle):
    """[(name, base, ops)] with concrete arguments: on two bases of sens_cases.scripts every edit
    kind once per special value (new reduced cost, cost change, new RHS, new column entry, the
    add-activity cost and one column entry, one add-constraint coefficient and its RHS), each
    followed by resolve_all and an ordinary change_rhs; and one start tableau with a planted
    inf."""
    import sens_cases
    out = []
    for name, base, _ in sens_cases.scripts(oracle)[:2]:
        T, x, z, basis = base
        R, C = T.shape
        m = R - 1
        bset = set(int(b) for b in basis)
        nonbasic = [j for j in range(C - 1) if j not in bset]
        basic = [j for j in range(C - 1 - m) if j in bset] or [int(basis[0])]
        act = np.round(np.linspace(0.2, 0.9, m), 3).tolist()
        tech = [float(1 + (j % 3)) if j < (C - 1) // 3 + 1 else 0.0 for j in range(C - 1)]
        tail = [("resolve_all", ()), ("change_rhs", (1, float(T[1, -1]) + 1.0))]
        for v in SENS_VALUES:
            tag = "nan" if v != v else repr(v)
            a2, t2 = list(act), list(tech)
            a2[m // 2] = v
            t2[0] = v
            edits = [("change_nonbasic_cbar", (nonbasic[0], v)),
                     ("change_basic", (basic[0], v)),
                     ("change_rhs", (1, v)),
                     ("change_nonbasic_column", (1, nonbasic[-1], v)),
                     ("add_activity", (v, act)), ("add_activity", (6.0, a2)),
                     ("add_constraint", (t2, 1.0)), ("add_constraint", (tech, v))]
            for op, args in edits:
                out.append(("%s_%s_%s_%d" % (name, op, tag, len(out)), base, [(op, args)] + tail))
    name, (T, x, z, basis), _ = sens_cases.scripts(oracle)[0]
    bset = set(int(b) for b in basis)
    nonbasic = [j for j in range(T.shape[1] - 1) if j not in bset]
    T = T.copy()
    T[2, nonbasic[1]] = math.inf
    out.append((name + "_start_inf", (T, x, z, basis),
                [("resolve_all", ()), ("change_nonbasic_cbar", (nonbasic[1], -1.0)),
                 ("change_rhs", (1, float(T[1, -1]) + 2.0))]))
    return out
