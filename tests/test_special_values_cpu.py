"""CPU tests on non-finite and extreme-magnitude data (tests/special_values.py): the C oracle
against the second restatements (ref_py*) on every generated case of every family, compared with
the NaN-aware comparator of DESIGN.md section 2 -- this is what entitles
test_special_values_gpu.py to treat the oracle as the truth -- and, on the oracle alone, the
conditions that keep those GPU tests from passing vacuously."""
import collections
import math

import numpy as np
import pytest

import special_values as sv
from ref_py import PyPrimal

STATUS = {0: "optimal", 1: "unbounded", 5: "limit"}


# ------------------------------------------------------------------------------ the comparator
def test_comparator():
    nan2 = np.frombuffer(np.uint64(0xfff8000000000123).tobytes(), dtype=np.float64)[0]
    assert sv.same([1.0, math.nan, math.inf], [1.0, nan2, math.inf])      # NaN bits are outside
    assert sv.same(math.nan, -math.nan)
    assert not sv.same([0.0], [-0.0])                                     # the sign of zero is in
    assert not sv.same([math.inf], [-math.inf])
    assert not sv.same([math.nan, 1.0], [1.0, math.nan])                  # NaN positions
    assert not sv.same([math.nan], [math.inf])
    assert not sv.same([1.0], [np.nextafter(1.0, 2.0)])
    assert not sv.same([5e-324], [0.0])
    assert not sv.same([1.0, 2.0], [1.0])
    assert len(sv.CLASSES) == len({sv.bits(v) for v in sv.VALUES}) == 21


# ------------------------------------------------------------------------------ primal
def _py_primal_from_tableau(T, basis, n):
    p = PyPrimal.__new__(PyPrimal)
    p.t = [[float(v) for v in row] for row in T]
    p.n, p.m = n, T.shape[0] - 1
    p.basic = [int(v) for v in basis]
    p.log, p.status, p.FinalZ, p.SolutionVector = [], None, 0.0, None
    return p


def _oracle_equals_py_primal(oracle, T, basis, n, cap, tag):
    r = sv.oracle_primal(oracle, T, basis, n, cap)
    p = _py_primal_from_tableau(T, basis, n)
    ps = p.solve(max_pivots=cap)
    assert ps == STATUS[r["status"]], tag
    assert [tuple(v) for v in r["log"].tolist()] == p.log, tag
    assert r["basis"].tolist() == p.basic, tag
    sv.assert_same(np.array(p.t), r["T"], tag)
    sv.assert_same(p.extract_solution(), r["x"], tag)
    sv.assert_same(p.t[0][-1], r["z"], tag)
    return r


@pytest.fixture(scope="module")
def fuzz_runs(oracle):
    """(case, oracle result) of every small-fuzz case; the restatement is checked on the way."""
    out = []
    for k, (T, basis, planted) in enumerate(sv.primal_fuzz()):
        n = T.shape[1] - T.shape[0]
        out.append(((T, basis, planted), _oracle_equals_py_primal(oracle, T, basis, n,
                                                                   sv.FUZZ_CAP, k)))
    return out


def test_small_fuzz_oracle_equals_restatement(fuzz_runs):
    assert len(fuzz_runs) == sv.FUZZ_COUNT
    assert all(T.shape[0] <= 9 and T.shape[1] <= 18 for (T, _, _), _ in fuzz_runs)


def test_small_fuzz_is_not_vacuous(oracle, fuzz_runs):
    """The thresholds of the committed generator and seed, on the oracle alone: NaN in >= 15 % of
    the final tableaux, +-inf in >= 10 %, two or more pivots in >= 40 % of the cases, both end
    statuses; and every value class in the pivot row or pivot column at the moment of a pivot in
    at least 3 cases."""
    N = len(fuzz_runs)
    finals = [r["T"] for _, r in fuzz_runs]
    assert sum(sv.has_nan(T) for T in finals) >= 0.15 * N
    assert sum(sv.has_inf(T) for T in finals) >= 0.10 * N
    assert sum(r["pivots"] >= 2 for _, r in fuzz_runs) >= 0.40 * N
    assert {0, 1} <= {r["status"] for _, r in fuzz_runs}
    seen = collections.Counter()
    for (T, _, _), _ in fuzz_runs:
        here = set()
        for _, _, _, prow, pcol, _ in sv.step_oracle(oracle, T, sv.FUZZ_CAP):
            here |= {name for name, v in sv.CLASSES.items()
                     if sv.holds(prow, v) or sv.holds(pcol, v)}
        seen.update(here)
    assert {k: seen[k] for k in sv.NAMES if seen[k] < 3} == {}


def test_constructed_primal_cases(oracle):
    """Oracle == restatement on each constructed case, and the mechanism each is named for."""
    res = {}
    for name, (T, basis, n) in sv.constructed_primal().items():
        res[name] = _oracle_equals_py_primal(oracle, T, basis, n, 16, name)
    inf, isnan = math.inf, math.isnan
    T = res["inf_in_pivot_row_zero_factors"]["T"]
    assert res["inf_in_pivot_row_zero_factors"]["log"].tolist() == [[1, 0]]
    assert T[0, 1] == inf and T[1, 1] == inf and isnan(T[2, 1]) and isnan(T[3, 1])
    T = res["inf_in_pivot_row_z_row_nan"]["T"]
    assert np.isnan(T[:, 2]).all() and isnan(T[0, 2])               # the Z row included
    r = res["z_row_nan_negzero_denorm"]
    assert r["log"].tolist() == [[2, 2]] and r["status"] == 0        # only -5e-324 enters
    assert res["z_row_only_nan_negzero"]["pivots"] == 0
    assert res["entering_entry_at_eps"]["log"].tolist() == [[3, 0]]  # only the row above 1e-9
    assert res["entering_entries_all_at_or_below_eps"]["status"] == 1
    T = res["product_overflows_then_inf_minus_inf"]["T"]
    assert isnan(T[2, 1]) and T[3, 1] == inf
    r = res["subnormal_ratios_tie_lower_row"]
    assert r["log"].tolist() == [[1, 0]] and r["T"][1, -1] == 5e-324
    T = res["tiny_pivot_row_overflows"]["T"]
    assert T[1, 1] == inf and T[2, 1] == -inf and T[0, 1] == inf
    assert res["nan_rhs_row_skipped_then_basic"]["log"].tolist() == [[2, 0]]
    assert isnan(res["nan_rhs_in_basic_row_of_a_decision_variable"]["x"][0])
    everything = np.concatenate([r["T"].reshape(-1) for r in res.values()] +
                                [T.reshape(-1) for T, _, _ in sv.constructed_primal().values()])
    assert sv.has_nan(everything) and sv.has_inf(everything)
    assert sv.holds(everything, 5e-324) or sv.holds(everything, -5e-324)


@pytest.mark.parametrize("m,n", sv.IN_BLOCK_SHAPES)
@pytest.mark.parametrize("value", sv.IN_BLOCK_VALUES, ids=["inf", "nan", "1e308"])
def test_in_block_cases_hit_inside_a_block(oracle, m, n, value):
    """For every planted larger case the oracle's stepping shows the planted value, or a
    non-finite value derived from it, in the pivot row or pivot column of a pivot q with
    q % 16 != 0, and at least 16 further pivots follow it.  Oracle against restatement: the
    whole solve at (8, 3000); at (300, 700) and (600, 50) only up to two pivots past the hit,
    because PyPrimal needs about 0.1 s per pivot there -- the later pivots of those two shapes,
    which the GPU test takes from the oracle alone, are not cross-checked."""
    T0, b0, (i, j), q, kind = sv.in_block_case(oracle, m, n, value)
    assert sv.holds(T0[i, j], value)
    assert j >= sv.last_strip_start(T0.shape[1]) and (i >= 64 or T0.shape[0] <= 65)
    first, made = sv.check_in_block(oracle, T0, value)
    assert first == q and q % 16 != 0 and made >= q + 1 + 16
    # the pivot itself: the value sits in the pivot row (kind "row") or in the pivot column
    for qq, r, e, prow, pcol, _ in sv.step_oracle(oracle, T0, q + 1):
        if qq == q:
            assert (r == i) if kind == "row" else (e == j)
    cap = sv.IN_BLOCK_CAP if (m, n) == (8, 3000) else q + 3
    _oracle_equals_py_primal(oracle, T0, b0, n, cap, (m, n, value))


# ------------------------------------------------------------------------------ revised
REV_STATUS = {0: "optimal", 1: "unbounded", 2: "infeasible_basis", 3: "pivot_too_small",
              4: "entering_already_basic", 5: "limit"}
REV_SNAP = ("y", "rcX", "rcS", "u_pre", "ratios_pre", "xB", "BInvA", "BInv")


@pytest.mark.parametrize("name,c,A,b", sv.revised_cases(), ids=[k[0] for k in sv.revised_cases()])
def test_revised_oracle_equals_restatement(oracle, name, c, A, b):
    """Result and every CaptureSnapshot number of the C oracle against PyRevised."""
    from ref_py import PyConstraint, PyRevised
    cons = [PyConstraint(row.tolist(), "<=", float(rhs)) for row, rhs in zip(A, b)]
    r = oracle.revised_solve(c, A, b, False, max_iter=sv.REVISED_CAP)
    p = PyRevised(c.tolist(), cons, False)
    assert p.solve(max_iter=sv.REVISED_CAP, capture=True) == REV_STATUS[r["status"]]
    assert [tuple(v) for v in r["log"].tolist()] == p.log
    assert r["basis"].tolist() == p.basic
    sv.assert_same(p.Binv, r["Binv"], "Binv")
    sv.assert_same(p.xB, r["xB"], "xB")
    if r["status"] == 0:
        sv.assert_same(p.FinalZ, r["z"], "z")
        sv.assert_same(p.SolutionVector, r["x"], "x")
    tr = oracle.revised_trace(c, A, b, False, max_iter=sv.REVISED_CAP, cap=sv.REVISED_CAP + 2)
    assert tr["count"] == len(p.snapshots) == len(tr["snapshots"])
    for k, (a, q) in enumerate(zip(tr["snapshots"], p.snapshots)):
        for key in ("entering", "leaving_row", "leaving_var"):
            assert a[key] == q[key], (k, key)
        assert a["basis_pre"].tolist() == q["basis_pre"], k
        assert a["basis_post"].tolist() == q["basis_post"], k
        for key in ("rc_pre", "z_working", "z_original") + REV_SNAP:
            sv.assert_same(a[key], q[key], (k, key))


def test_constructed_revised_cases(oracle):
    """The mechanism each constructed case is named for, on the oracle alone."""
    cases = {name: (c, A, b) for name, c, A, b in sv.constructed_revised()}
    tr = oracle.revised_trace(*cases["nan_and_sub_eps_eta_inf_reduced_cost"], False, max_iter=8)
    s = tr["snapshots"][1]
    assert s["rc_pre"] == math.inf and s["leaving_row"] == 1 and s["u_pre"][1] == math.inf
    assert s["u_pre"][2] == math.inf and s["u_pre"][3] == 5e307       # eta: 0, 0, NaN, -0
    assert np.isnan(s["BInv"][2]).all() and not s["BInv"][1].any()    # NaN row kept, pivot row 0
    assert s["BInv"][3].tolist() == [-0.5, 0.0, 0.0, 1.0]             # sub-EPS factor: skipped
    r = oracle.revised_solve(*cases["nan_ratios_from_inf_and_nan_rhs"], False)
    assert r["status"] == 1 and np.isnan(r["xB"]).all()
    tr = oracle.revised_trace(*cases["inf_ratio_from_overflow"], False, max_iter=8)
    assert tr["snapshots"][0]["ratios_pre"].tolist() == [math.inf, 4.0]
    assert tr["snapshots"][0]["leaving_row"] == 1
    tr = oracle.revised_trace(*cases["pivot_at_eps_plus_ulp"], False, max_iter=8)
    s = tr["snapshots"][0]
    assert s["leaving_row"] == 2 and sv.same(s["u_pre"][2], sv.CLASSES["eps+ulp"])
    assert s["ratios_pre"][:2].tolist() == [math.inf, math.inf] and tr["status"] != 3
    assert oracle.revised_solve(*cases["direction_at_or_below_eps_is_unbounded"],
                                False)["status"] == 1
    data = np.concatenate([np.concatenate([c, A.reshape(-1), b]) for c, A, b in cases.values()])
    assert sv.has_nan(data) and sv.has_inf(data) and sv.holds(data, 5e-324)
    assert sv.holds(data, sv.DBL_MAX)
    fuzz = np.concatenate([np.concatenate([c, A.reshape(-1), b])
                           for _, c, A, b in sv.revised_fuzz()])
    assert [k for k, v in sv.CLASSES.items() if not sv.holds(fuzz, v)] == []


# ------------------------------------------------------------------------------ B&B rounding
def test_bb_rounding_helpers_on_the_value_classes(oracle):
    """Math.Round(x, 4) and Math.Round(x): C oracle against ref_py_bb on every value class, the
    neighbours of 1e16 and 2^31 +- 0.5 and 4-decimal midpoints; and RoundTableau / the node
    scoring on the array test_special_values_gpu.py gives the device."""
    from ref_py_bb import BranchAndBound, round4, round_int
    T = sv.rounding_tableau()
    assert [k for k, v in sv.CLASSES.items() if not sv.holds(T, v)] == []
    for x in T.reshape(-1).tolist():
        sv.assert_same(oracle.round4(x), round4(x), x)
        sv.assert_same(oracle.round_int(x), round_int(x), x)
    assert oracle.round4(1e16) == 1e16 and oracle.round4(math.inf) == math.inf
    assert math.isnan(oracle.round4(math.nan)) and math.copysign(1.0, oracle.round4(-0.0)) < 0
    assert oracle.round4(5e-324) == 0.0 and oracle.round4(1e308) == 1e308
    assert oracle.round4(2.0 ** 31 - 0.5) == 2.0 ** 31 - 0.5
    bb = BranchAndBound(2)
    rounded, z, vals = oracle.bb_node_info(T, 2)
    sv.assert_same(rounded, bb.RoundTableau(T.tolist()), "RoundTableau")
    sv.assert_same(rounded, oracle.bb_round_tableau(T), "bb_round_tableau")
    sv.assert_same(vals, bb._decision(bb.RoundTableau(T.tolist())), "decision values")
    sv.assert_same(z, round4(T[0, -1]), "z")
    assert math.isnan(vals[1]) and vals[0] == 1e308


# ------------------------------------------------------------------------------ B&B start tableaux
def test_bb_oracle_equals_restatement_on_planted_start_tableaux(oracle):
    """oracle.bb_solve against ref_py_bb.BranchAndBound from start tableaux with one planted
    +-inf, NaN or 1e308 at every position: node records, pop order, every pivot, incumbent.
    (Before this test the restatement raised on a non-finite decision value: Python's math.floor
    refuses what Math.Floor :837 / :870-871 returns unchanged.)"""
    from ref_py_bb import BranchAndBound
    cases = sv.bb_start_tableaux(oracle)
    assert len(cases) == 4 * 77 - 1
    pivots = nonfinite_z = 0
    for name, T, n in cases:
        r = oracle.bb_solve(T, n, node_cap=sv.BB_NODE_CAP)
        bb = BranchAndBound(n, node_cap=sv.BB_NODE_CAP)
        p = bb.Execute([list(map(float, row)) for row in T.tolist()])
        assert (r["status"] == 6) == p["capped"], name
        assert r["processed"] == p["processed"] and r["pop_order"] == bb.pop_order, name
        assert sv.same_records(r["records"], bb.records), name
        assert r["trace"] == bb.trace, name
        assert r["found"] == (p["x"] is not None), name
        sv.assert_same(r["z"], p["z"], name)
        if r["found"]:
            sv.assert_same(r["x"], p["x"], name)
            assert r["best_node"] == p["best_node"], name
        pivots += len(r["trace"]) > 0
        nonfinite_z += any(not math.isfinite(rec["z"]) for rec in r["records"])
    # most cases still branch and pivot; the three non-finite values planted in the objective
    # cell alone give a non-finite root z
    assert pivots >= len(cases) // 2 and nonfinite_z >= 3


def test_bb_device_cases_take_the_nonfinite_branch(oracle):
    """Section 4 of the issue for B&B, on the cases the device runs: the trace shows a pivot whose
    normalised pivot row is non-finite while at least one other row has factor exactly 0 (the
    `nonfinite` vote of k_bb_select), and a pivot with a non-finite factor.  The stepping is the
    restatement's, whose trace the test above pins to the oracle's pivot for pivot."""
    cases = sv.bb_device_cases(oracle)
    assert sum(1 for c in cases if c[3]) >= 10 and sum(1 for c in cases if c[4]) >= 10
    assert any(c[3] and not c[4] for c in cases) or any(c[4] and not c[3] for c in cases)
    data = np.concatenate([c[1].reshape(-1) for c in cases])
    assert sv.has_nan(data) and sv.has_inf(data) and sv.holds(data, 1e308)
    for name, T, n, row_hit, col_hit in cases:
        if row_hit or col_hit:
            assert oracle.bb_solve(T, n, node_cap=sv.BB_NODE_CAP)["trace"], name


# ------------------------------------------------------------------------------ cut, dual, primal2
def _split(T):
    return list(map(float, T[0])), [list(map(float, r)) for r in T[1:]]


def test_cut_oracle_equals_restatement_on_planted_tableaux(oracle):
    """DualSimplex.cs, PrimalSimplexSolver2.cs and CuttingPlaneSolver.cs: oracle against
    ref_py_cut on every planted tableau.  (Before this test ref_py_cut's Frac raised on +-inf and
    NaN, where Math.Floor, CuttingPlaneSolver.cs:14, returns them unchanged.)"""
    import ref_py_cut as rp
    planted = sv.cut_planted(oracle)
    dual = {0: "ok", 1: "infeasible", 5: "limit"}
    prim = {0: "ok", 1: "unbounded", 5: "limit"}
    cap = sv.CUT_HARD_CAP
    seen = {"dual": set(), "primal2": set(), "cut": set()}
    for name, T0 in planted["dual"]:
        T = T0.copy()
        rc, piv, log = oracle.dual_solve(T, print_steps=True, hard_cap=cap)
        obj, rows = _split(T0)
        plog = []
        try:
            st = rp.dual_solve(obj, rows, print_steps=True, log=plog, hard_cap=cap)
        except rp.PivotTooSmall:
            st = 3
        assert st == dual.get(rc, rc), (name, st, rc)
        assert plog == log, name
        sv.assert_same(np.array([obj] + rows), T, name)
        seen["dual"].add(rc)
    for name, T0 in planted["primal2"]:
        T = T0.copy()
        rc, piv, log = oracle.primal2_solve(T, print_steps=False, hard_cap=cap)
        obj, rows = _split(T0)
        plog = []
        try:
            st = rp.primal2_solve(obj, rows, print_steps=False, log=plog, hard_cap=cap)
        except rp.PivotTooSmall:
            st = 3
        assert st == prim.get(rc, rc), (name, st, rc)
        assert plog == log, name
        if st != 3:   # the C# works on its own copy and throws before writing back
            sv.assert_same(np.array([obj] + rows), T, name)
        seen["primal2"].add(rc)
    for name, T0 in planted["cut"]:
        rc, cuts, T, log = oracle.cutting_plane(T0, max_cuts=4, hard_cap=cap)
        obj, rows = _split(T0)
        plog = []
        prc, pcuts = rp.cutting_plane(obj, rows, max_cuts=4, log=plog, hard_cap=cap)
        assert (prc, pcuts) == (rc, cuts), (name, prc, pcuts, rc, cuts)
        assert plog == log, name
        sv.assert_same(np.array([obj] + rows), T, name)
        seen["cut"].add(rc)
    assert len(seen["dual"]) >= 2 and len(seen["primal2"]) >= 2 and len(seen["cut"]) >= 3
    for kind in planted:
        data = np.concatenate([T.reshape(-1) for _, T in planted[kind]])
        assert sv.has_nan(data) and sv.has_inf(data) and sv.holds(data, 5e-324), kind
        assert sv.holds(data, sv.DBL_MAX) or sv.holds(data, 1e308), kind
    names = [n for k in planted for n, _ in planted[k]]
    for tag in ("_inf_and_nan_ratio", "_inf_and_nan_rhs", "_inf_and_nan_cost", "_inf_ratio",
                "_nan_fractional_part"):
        assert sum(n.endswith(tag) for n in names) >= 2, tag


# ------------------------------------------------------------------------------ sensitivity
def test_sens_oracle_equals_restatement_on_special_edit_arguments(oracle):
    """SensitivityAnalyzer.cs: oracle against ref_py_sens after every edit of every script."""
    import ref_py_sens as rp
    codes = set()
    scripts = sv.sens_scripts(oracle)
    for name, (T, x, z, basis), ops in scripts:
        o = oracle.sens(T, x, z, basis)
        p = rp.PySens(T.tolist(), list(map(float, x)), float(z), [int(b) for b in basis])
        for k, (op, args) in enumerate(ops):
            rc = getattr(o, op)(*args)
            prc = rp.run(getattr(p, op), *args)
            prc = 0 if prc is None else prc
            assert prc == rc, (name, k, op, rc, prc)
            st = o.state()
            sv.assert_same(np.array(p.t), st["T"], (name, k, op))
            assert p.basic == st["basic"], (name, k, op)
            sv.assert_same(p.sol, st["sol"], (name, k, op))
            sv.assert_same(p.z, st["z"], (name, k, op))
            assert p.log == o.log(), (name, k, op)
            codes.add(rc)
    assert {0, 1, 2, 8} <= codes, codes
    args = np.array([v for _, _, ops in scripts for _, a in ops for v in np.hstack(
        [np.ravel(np.asarray(q, dtype=np.float64)) for q in a] or [np.zeros(0)])])
    assert sv.has_nan(args) and sv.has_inf(args) and sv.holds(args, 1e308)
    assert sv.holds(args, 5e-324) and sv.holds(args, -0.0)
