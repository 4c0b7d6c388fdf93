"""CPU tests of the sensitivity report's restatement (tests/ref_py_ranging.py) and of its fixtures
(tests/ranging_cases.py): the literal per-index loops and the vectorised formulation agree under
the parity comparator, Math.Max / Math.Min on their special cases, a hand-worked model, and every
planted case holds what it plants.  test_ranging_gpu.py holds the device against the same
restatement."""
import math

import numpy as np
import pytest

import ranging_cases as rc
import ref_py_ranging as ref
import special_values as sv


def assert_same_report(a, b, what):
    for f in ref.FIELDS:
        if f in ref.INT_FIELDS:
            assert np.array_equal(a[f], b[f]), (what, f, a[f].tolist(), b[f].tolist())
        else:
            sv.assert_same(a[f], b[f], (what, f))


def _bits(v):
    return sv.bits(v)


def test_dotnet_max_min_table():
    nan, inf = math.nan, math.inf
    # +-0 ties: neither > nor < holds, the second argument comes back
    for a, b in [(0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0)]:
        assert _bits(ref.dotnet_max(a, b)) == _bits(b)
        assert _bits(ref.dotnet_min(a, b)) == _bits(b)
    for x in (-inf, -1.0, -0.0, 0.0, 2.5, inf):
        assert math.isnan(ref.dotnet_max(x, nan)) and math.isnan(ref.dotnet_min(x, nan))
        assert math.isnan(ref.dotnet_max(nan, x)) and math.isnan(ref.dotnet_min(nan, x))
        assert _bits(ref.dotnet_max(inf, x)) == _bits(inf)
        assert _bits(ref.dotnet_max(x, inf)) == _bits(inf)
        assert _bits(ref.dotnet_min(-inf, x)) == _bits(-inf)
        assert _bits(ref.dotnet_min(x, -inf)) == _bits(-inf)
        assert _bits(ref.dotnet_max(-inf, x)) == _bits(x)      # the identities of the folds
        assert _bits(ref.dotnet_min(inf, x)) == _bits(x)
    assert math.isnan(ref.dotnet_max(nan, nan)) and math.isnan(ref.dotnet_min(nan, nan))
    # where Python's max / min differ: they keep the FIRST of a tie and drop a NaN second argument
    assert _bits(max(0.0, -0.0)) != _bits(ref.dotnet_max(0.0, -0.0))
    assert not math.isnan(max(1.0, nan))


@pytest.fixture(scope="module")
def cases():
    return rc.cpu_cases()


def test_two_formulations_agree(cases):
    assert len(cases) >= 60
    for name, T, basic in cases:
        assert T.shape[0] <= 70 and T.shape[1] <= 200, name
        assert_same_report(ref.report_literal(T, basic), ref.report_numpy(T, basic), name)


def test_hand_worked_model():
    T, x, z, basic, want = rc.hand_worked()
    assert rc.rebuilt_basis(T) == basic
    for rep in (ref.report_literal(T, basic), ref.report_numpy(T, basic)):
        for f in ref.FIELDS:
            assert rep[f].tolist() == want[f], f


def _swap_flips(T, fold, pick, swap):
    """The literal fold's answer is a zero, and swapping the two planted entries changes its sign;
    returns the sign bit before the swap."""
    a = fold(T.tolist())[pick]
    T2 = T.copy()
    (i1, j1), (i2, j2) = swap
    T2[i1, j1], T2[i2, j2] = T[i2, j2], T[i1, j1]
    b = fold(T2.tolist())[pick]
    assert a == 0.0 and b == 0.0, (a, b)
    assert np.signbit(a) != np.signbit(b), (a, b)
    return bool(np.signbit(a))


def test_zero_tie_cases_hold_what_they_plant():
    T, x, z, plants = rc.row_zero_ties()
    basic = rc.rebuilt_basis(T)
    assert basic == list(range(len(basic)))
    signs = set()
    for (r, which, p1, p2) in plants:
        pick = 0 if which == "lo" else 1
        neg = _swap_flips(T, lambda L: ref.basic_range(L, basic, r - 1, r), pick,
                          ((0, p1), (0, p2)))
        signs.add((which, neg))
        other = [(-T[0, j] / T[r, j]) for j in range(T.shape[1] - 1)
                 if j not in basic and j not in (p1, p2) and abs(T[r, j]) > rc.EPS]
        assert other and all((q < 0) if which == "lo" else (q > 0) for q in other), r
    assert signs == {("lo", True), ("lo", False), ("hi", True), ("hi", False)}

    T, x, z, plants = rc.col_zero_ties()
    n = T.shape[1] - T.shape[0]
    signs = set()
    for (c, which, r1, r2) in plants:
        pick = 0 if which == "lo" else 1
        s = n + c - 1
        neg = _swap_flips(T, lambda L: ref.rhs_range(L, s), pick, ((r1, -1), (r2, -1)))
        signs.add((which, neg))
        other = [(-T[i, -1] / T[i, s]) for i in range(1, T.shape[0])
                 if i not in (r1, r2) and abs(T[i, s]) > rc.EPS]
        assert other and all((q < 0) if which == "lo" else (q > 0) for q in other), c
    assert signs == {("lo", True), ("lo", False), ("hi", True), ("hi", False)}


def test_zero_tie_geometry():
    """The planted pairs are separated the way their comments say, for the documented tile."""
    lane = lambda c: (c % rc.TILE_COLS) // 2
    tile = lambda c: c // rc.TILE_COLS
    cls = [("lane", lambda a, b: tile(a) == tile(b) and lane(a) == lane(b)),
           ("segment", lambda a, b: lane(a) != lane(b) and lane(a) // 8 == lane(b) // 8),
           ("wave", lambda a, b: lane(a) // 8 != lane(b) // 8 and lane(a) // 64 == lane(b) // 64),
           ("group", lambda a, b: tile(a) == tile(b) and lane(a) // 64 != lane(b) // 64),
           ("tiles", lambda a, b: tile(a) != tile(b)), ("tiles", lambda a, b: tile(a) != tile(b))]
    for k, (a, b) in enumerate(rc.ROW_PAIRS):
        assert a < b and cls[k // 2][1](a, b), (k, cls[k // 2][0])
    sub = lambda r: (r - 1) // rc.SUB_ROWS
    trow = lambda r: (r - 1) // rc.TILE_ROWS
    rcls = [lambda a, b: sub(a) == sub(b), lambda a, b: sub(a) != sub(b) and trow(a) == trow(b),
            lambda a, b: trow(a) != trow(b), lambda a, b: trow(a) != trow(b)]
    for k, (a, b) in enumerate(rc.COL_PAIRS):
        assert a < b and rcls[k // 2](a, b), k


def test_equal_maxima_case():
    T, x, z = rc.equal_maxima()
    m = T.shape[0] - 1
    assert np.array_equal(T[:, m + 9], T[:, m + 2])
    rep = ref.report_literal(T, rc.rebuilt_basis(T))
    assert (rep["cost_lo"][:m] == 100.0).all() and (rep["rhs_lo"] >= 80.0).all()
    assert np.array_equal(T[1, m + 40:], T[2, m + 40:])


def test_eps_boundary_case():
    T, x, z, vals = rc.eps_boundary()
    up, dn = sv.CLASSES["eps+ulp"], sv.CLASSES["-eps-ulp"]
    basic = rc.rebuilt_basis(T)
    m = T.shape[0] - 1
    n = T.shape[1] - T.shape[0]
    rep = ref.report_literal(T, basic)
    q = vals.index(up), vals.index(dn)
    # row 1 (basic column 0): exactly the two entries beyond EPS count
    assert rep["cost_lo"][0] == -T[0, m + q[0]] / up and rep["cost_hi"][0] == -T[0, m + q[1]] / dn
    assert rep["cost_lo"][6] == -math.inf and rep["cost_hi"][6] == math.inf       # row 7: nothing
    assert rep["rhs_lo"][2] == -T[1 + q[0], -1] / up and rep["rhs_hi"][2] == -T[1 + q[1], -1] / dn
    assert rep["rhs_lo"][3] == -math.inf and rep["rhs_hi"][3] == math.inf
    assert n == m + 8


def test_coverage_case():
    T, x, z = rc.coverage()
    rep = ref.report_literal(T, rc.rebuilt_basis(T))
    m = T.shape[0] - 1
    for lo, hi in ((rep["cost_lo"][:m], rep["cost_hi"][:m]), (rep["rhs_lo"], rep["rhs_hi"])):
        assert np.isfinite(lo).any() and np.isfinite(hi).any()
        assert (hi == math.inf).any() and (lo == -math.inf).any()
    assert set(rep["kind"].tolist()) >= {ref.NONBASIC_RANGE, ref.NONBASIC_BOUNDARY,
                                         ref.NONBASIC_NOT_OPTIMAL, ref.BASIC}


def test_nonfinite_cases_reach_the_report():
    reached = {"nan": 0, "inf": 0}
    for name, T, x, z in rc.nonfinite_cases(12, 30):
        rep = ref.report_literal(T, rc.rebuilt_basis(T))
        vals = np.concatenate([rep[f] for f in ref.FIELDS if f not in ref.INT_FIELDS])
        if name == "nan_entry_skipped":
            assert not np.isnan(np.concatenate([rep[f] for f in ("cost_lo", "cost_hi", "rhs_lo",
                                                                 "rhs_hi")])).any()
        if name == "nan_quotient_sticks":
            assert np.isnan(rep["cost_lo"][:12]).all() and np.isnan(rep["rhs_hi"]).all()
        if name == "inf_over_inf":
            assert np.isnan(rep["cost_lo"][1]) and np.isnan(rep["rhs_lo"][1])
        reached["nan"] += bool(np.isnan(vals).any())
        reached["inf"] += bool(np.isinf(rep["reduced_cost"]).any() or np.isinf(rep["rhs_now"]).any())
    # NaN: in the Z row and the RHS (two ends each) and the two constructed quotients; a NaN
    # entry `a` is skipped and reaches nothing
    assert reached["nan"] >= 6 and reached["inf"] >= 4, reached


def test_degenerate_bases():
    (n1, T1, _, _), (n2, T2, _, _) = rc.degenerate_created()
    b1 = rc.rebuilt_basis(T1)
    assert b1[2] == -1 and b1.count(-1) == 1
    b2 = rc.rebuilt_basis(T2)
    rep = ref.report_literal(T2, b2)
    assert 10 not in b2 and ref.get_basic_row(T2.tolist(), 10) == 2
    assert rep["kind"][10] in (ref.NONBASIC_RANGE, ref.NONBASIC_BOUNDARY, ref.NONBASIC_NOT_OPTIMAL)
    assert rep["var_row"][10] == -1
    for name, T, basic in rc.raw_bases():
        rep = ref.report_literal(T, basic)
        if name == "non_unit_entry":
            assert rep["kind"][8] == ref.BASIC_ROW_NOT_FOUND and rep["var_row"][8] == -1
            assert rep["cost_lo"][8] == -math.inf and rep["cost_hi"][8] == math.inf
        if name == "duplicate_entry":
            assert rep["kind"][2] != ref.BASIC and rep["kind"][1] == ref.BASIC
        if name == "minus_one_entry":
            assert (rep["kind"] == ref.BASIC).sum() == 4


def test_row_not_found_script_on_the_oracle(oracle):
    """The edit leaves column 0 in basicVars without a basic row (so the GPU test that runs the
    same edit does meet BASIC_ROW_NOT_FOUND)."""
    T, x, z, (k, new_b) = rc.row_not_found_script()
    o = oracle.sens(T, x, z, np.array(rc.rebuilt_basis(T), dtype=np.int32))
    assert o.change_rhs(k, new_b) == 0
    st = o.state()
    assert 0 in st["basic"]
    rep = ref.report_literal(st["T"], st["basic"])
    assert rep["kind"][0] == ref.BASIC_ROW_NOT_FOUND
    assert_same_report(rep, ref.report_numpy(st["T"], st["basic"]), "after the edit")
