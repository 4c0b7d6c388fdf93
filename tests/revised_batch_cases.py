"""Shared inputs of the revised-simplex batch tests: the models of
test_oracle_revised.revised_cases(), the shapes on both sides of the form thresholds (derived
from the footprint formula the Python mirror repeats from rev_batch_common.hpp), the tie-heavy
set that exercises the ratio fold's tie clause, and an instrumented copy of both folds
(tie_stats; with a probe list it also reports what the entering and the ratio fold saw and chose
at every iteration, which seam_cases.py uses to find and assert where its plants are live)."""
import math

import numpy as np

import lp_cases
from ref_py import DBL_MAX, REV_EPS, PyConstraint, _dot, _mat_mul_skip, _mat_vec, _vec_mat
from test_oracle_revised import flat, revised_cases

CAP = 3000  # max_pivots of the uninterrupted solves (klee_minty_8 needs 255)


def models():
    """(name, (objective, constraints, is_min)) of revised_cases()."""
    return revised_cases()


def to_model(c, A, b, is_min=False):
    A = np.asarray(A, dtype=np.float64)
    return (list(map(float, c)),
            [PyConstraint([float(v) for v in A[i]], "<=", float(b[i])) for i in range(len(b))],
            is_min)


def oracle_ref(oracle, model, max_iter=CAP):
    obj, cons, is_min = model
    A, b = flat(cons)
    return oracle.revised_solve(obj, A, b, is_min, max_iter=max_iter)


# ------------------------------------------------------------------------------ thresholds
def threshold_shapes():
    """[(name, m, n, form)]: for W and for G, the largest square-ish LP that fits -- the largest
    m with (m, m) inside, then the largest n at that m -- and its two neighbours outside, one
    column and one row further."""
    from lpr_381_group_v22_amd import revised_batch as rb
    out = []
    for name, limit in (("W", rb.MAX_LDS_W), ("G", rb.MAX_LDS_G)):
        m = 1
        while 8 * rb.footprint(m + 1, m + 1) <= limit:
            m += 1
        n = m
        while 8 * rb.footprint(m, n + 1) <= limit:
            n += 1
        out.append((f"{name}_last_inside", m, n, rb.pick_form(m, n)))
        out.append((f"{name}_first_outside_n", m, n + 1, rb.pick_form(m, n + 1)))
        mm = m
        while 8 * rb.footprint(mm, n) <= limit:
            mm += 1
        out.append((f"{name}_first_outside_m", mm, n, rb.pick_form(mm, n)))
    return out


def threshold_models():
    return [(name, lp_cases.random_dense(m, n, 11 + q)[:2] + (False,))
            for q, (name, m, n, _) in enumerate(threshold_shapes())]


# ------------------------------------------------------------------------------ tie clause
TIE_SHAPES = ((6, 6), (8, 8), (8, 12), (5, 10))
TIE_SEEDS = range(64)


def tie_models():
    """256 tie-heavy LPs; relations are ignored, as the revised constructor does."""
    return [lp_cases.tie_heavy(m, n, seed)[:2] + (False,)
            for (m, n) in TIE_SHAPES for seed in TIE_SEEDS]


def tie_stats(model, max_iter=CAP, probe=None):
    """The loop of Solve() (:82-251) on ref_py's helpers with an instrumented ratio fold.
    Returns (status, iterations, fired, changed): the iterations at which the tie clause replaces
    an already-taken row, and those at which the chosen row differs from the pure
    "ratio < best - EPS" fold.  probe: a list that receives, per iteration that reaches a pivot,
    what the two folds saw and chose: dict(it, rc (per index of n + m, None: not a candidate),
    entering, ratios (per row, None: u_i <= EPS), basic (before the pivot), leaving)."""
    obj, cons, is_min = model
    n, m = len(obj), len(cons)
    c = [-v for v in obj] if is_min else list(obj)
    A = [list(con.Coefficients) for con in cons]
    b = [con.RHS for con in cons]
    basic = [n + i for i in range(m)]
    nonbasic = list(range(n))
    Binv = [[1.0 if i == j else 0.0 for j in range(m)] for i in range(m)]
    cB = [0.0] * m
    it = fired = changed = 0
    while True:
        xB = _mat_vec(Binv, b)
        if any(v < -REV_EPS for v in xB):
            return "infeasible_basis", it, fired, changed
        y = _vec_mat(cB, Binv)
        rcX = [c[j] - _dot(y, [A[i][j] for i in range(m)]) for j in range(n)]
        rcS = [-y[k] for k in range(m)]
        entering, best = -1, -math.inf
        seen = [None] * (n + m)
        for v in sorted(nonbasic):
            rc = rcX[v] if v < n else rcS[v - n]
            if rc > REV_EPS:
                seen[v] = rc
            if rc > REV_EPS and (entering == -1 or rc > best + REV_EPS):
                best, entering = rc, v
        if entering == -1:
            return "optimal", it, fired, changed
        if max_iter > 0 and it >= max_iter:
            return "limit", it, fired, changed
        if entering < n:
            u = _mat_vec(Binv, [A[i][entering] for i in range(m)])
        else:
            u = [Binv[i][entering - n] for i in range(m)]
        leaving, best_ratio = -1, DBL_MAX
        pure, pure_best = -1, DBL_MAX
        tie_here = False
        ratios = [None] * m
        for i in range(m):
            if u[i] > REV_EPS:
                ratio = xB[i] / u[i]
                ratios[i] = ratio
                if ratio < pure_best - REV_EPS:
                    pure, pure_best = i, ratio
                if ratio < best_ratio - REV_EPS:
                    best_ratio, leaving = ratio, i
                elif abs(ratio - best_ratio) <= REV_EPS and \
                        (leaving == -1 or basic[i] < basic[leaving]):
                    tie_here = tie_here or leaving != -1
                    best_ratio, leaving = ratio, i
        if leaving == -1:
            return "unbounded", it, fired, changed
        fired += tie_here
        changed += leaving != pure
        if probe is not None:
            probe.append(dict(it=it, rc=seen, entering=entering, ratios=ratios,
                              basic=list(basic), leaving=leaving))
        leaving_var = basic[leaving]
        if leaving_var == entering:
            return "entering_already_basic", it, fired, changed
        basic[leaving] = entering
        nonbasic.remove(entering)
        if leaving_var not in nonbasic:
            nonbasic.append(leaving_var)
        cB[leaving] = c[entering] if entering < n else 0.0
        pivot = u[leaving]
        if abs(pivot) < REV_EPS:
            return "pivot_too_small", it, fired, changed
        E = [[1.0 if i == j else 0.0 for j in range(m)] for i in range(m)]
        for i in range(m):
            E[i][leaving] = (1.0 / pivot) if i == leaving else (-u[i] / pivot)
        Binv = _mat_mul_skip(E, Binv)
        it += 1


# ------------------------------------------------------------------------------ constructed
def duplicated_rows(m, n, copies, seed):
    """The family of test_ratio_fold_beyond_the_lds_replay: every base row `copies` times, noise
    inside the EPS band.  Draw order: the base rows, then the noise, then c."""
    rng = np.random.RandomState(seed)
    base = rng.uniform(0.5, 2.0, size=(m // copies, n))
    A = np.repeat(base, copies, axis=0)[:m].copy()
    A += rng.uniform(0.0, 2e-10, size=A.shape)
    b = np.full(m, 10.0)
    c = rng.uniform(1.0, 2.0, size=n)
    return to_model(c, A, b)


def ieee_div_model():
    """One pivot on row 0 whose eta factor -a10 / a00 is the operand pair on which the hardware's
    division sequence rounds the other way."""
    return to_model([1.0], [[float.fromhex("0x1.ffffffffffffbp+1")],
                            [float.fromhex("0x1.6666666666663p+0")]], [1.0, 1.0])


def zero_skip_models():
    """The inputs of test_update_binverse_zero_skip_and_negative_zero (tests/test_revised_gpu.py)."""
    out = []
    for seed in range(5):
        obj, cons, _ = lp_cases.tie_heavy(20, 16, 100 + seed)
        out.append((obj, [PyConstraint(c.Coefficients, c.Relation, abs(float(c.RHS)))
                          for c in cons], False))
    return out


def degenerate_models():
    return [
        ("m1_n1", to_model([2.0], [[3.0]], [6.0])),
        ("m1_n12", lp_cases.random_dense(1, 12, 21)[:2] + (False,)),
        ("m8_n1", lp_cases.random_dense(8, 1, 22)[:2] + (False,)),
        ("zero_objective", to_model([0.0, 0.0, 0.0], np.ones((2, 3)), [1.0, 2.0])),
        ("zero_A", to_model([1.0, 2.0], np.zeros((3, 2)), [1.0, 1.0, 1.0])),
    ]


def mixed_models():
    """W-, G- and H-sized LPs interleaved (tie-heavy ones with |b| so that they run)."""
    def ties(m, n, seed):
        obj, cons, _ = lp_cases.tie_heavy(m, n, seed)
        return (obj, [PyConstraint(c.Coefficients, "<=", abs(float(c.RHS))) for c in cons], False)
    return [ties(4, 6, 1), lp_cases.random_dense(32, 64, 5)[:2] + (False,),
            lp_cases.random_dense(100, 120, 7)[:2] + (False,),
            lp_cases.random_dense(5, 8, 2)[:2] + (False,), ties(32, 64, 6), ties(6, 3, 3),
            lp_cases.random_dense(110, 90, 8)[:2] + (False,)]
