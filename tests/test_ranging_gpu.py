"""GPU parity tests of the sensitivity report (lpr_sens_ranging) against
tests/ref_py_ranging.py: doubles under the parity comparator (NaN positions identical, every other
element identical in all 64 bits, the sign of zero included), ints exactly.  The reference is
always computed on the state read back from the same handle (tableau and basicVars), so it sees
what the device holds.  Fixtures: tests/ranging_cases.py, checked on the CPU by
test_ranging_cpu.py.

The sweep's tile is 32 rows x 512 columns, its rows taken 8 at a time
(csrc/sens_ranging_common.hpp: kRngTileRows, kRngTileCols, kRngSubRows); ranging_cases.TILE_ROWS /
TILE_COLS / SUB_ROWS restate them and test_tile_constants_match_the_kernel reads them back from the
header.

Degenerate bases: lpr_sens_create takes no basicVars -- like the C#'s constructor (:35) it
rebuilds them from the tableau -- so the bases that can be handed over are those a tableau
produces: a -1 entry (a row without a unit column) and two identical unit columns of which only
the first is basic.  A basicVars entry without a basic row is reached through an edit
(ranging_cases.row_not_found_script).  A duplicate entry cannot be produced through the ABI; the
restatement's handling of one is covered on the CPU (test_ranging_cpu.py::test_degenerate_bases)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ranging_cases as rc
import ref_py_ranging as ref
import sens_cases
import special_values as sv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(engine, T, x, z):
    from lpr_381_group_v22_amd.engine import SensState
    return SensState.create(engine, T, x, z)


def _snapshot(d):
    T, basic, sol = d.read()
    return T.tobytes(), basic.tolist(), sol.tobytes(), d.shape(), len(d.log())


def assert_report(d, what, numpy_ref=False, check_untouched=True):
    """One ranging() call on handle d against the restatement on d's own state; returns both."""
    before = _snapshot(d) if check_untouched else None
    rep = d.ranging()
    if check_untouched:
        assert _snapshot(d) == before, (what, "the call changed the analyzer")
    T, basic, _ = d.read()
    want = (ref.report_numpy if numpy_ref else ref.report_literal)(T, basic.tolist())
    for f in ref.FIELDS:
        got = getattr(rep, f)
        if f in ref.INT_FIELDS:
            assert got.dtype == np.int32 and np.array_equal(got, want[f]), (what, f)
        else:
            sv.assert_same(got, want[f], (what, f))
    return rep, want


def _check(engine, name, T, x, z, numpy_ref=False):
    d = _create(engine, T, x, z)
    try:
        return assert_report(d, name, numpy_ref)
    finally:
        d.destroy()


def test_tile_constants_match_the_kernel():
    text = open(os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc", "sens_ranging_common.hpp")).read()
    val = lambda k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1))
    assert val("kRngTileRows") == rc.TILE_ROWS and val("kRngSubRows") == rc.SUB_ROWS
    assert 2 * val("kRngLanes") == rc.TILE_COLS


def test_tiny_and_edge_shapes(engine):
    seen = set()
    for name, T, x, z, numpy_ref in rc.shape_cases():
        rep, want = _check(engine, name, T, x, z, numpy_ref)
        seen.add(T.shape)
        if not name.startswith("n0"):
            assert (want["kind"] == ref.BASIC).sum() == T.shape[0] - 1, name
    assert (2, 2) in seen and (1030, 2100) in seen and (200, 1300) in seen
    assert {(6, w + 1) for w in (15, 16, 17, 63, 64, 65, 127, 129)} <= seen
    assert {(rc.TILE_ROWS + d + 1, 2 * (rc.TILE_ROWS + d) + 4) for d in (-1, 0, 1)} <= seen


def test_planted_zero_ties_in_rows(engine):
    T, x, z, plants = rc.row_zero_ties()
    rep, want = _check(engine, "row_zero_ties", T, x, z, numpy_ref=True)
    signs = set()
    for (r, which, p1, p2) in plants:
        v = (rep.cost_lo if which == "lo" else rep.cost_hi)[r - 1]
        assert v == 0.0, (r, which, v)
        # the later of the two wins: -cbar / (+-1) of column p2
        assert sv.bits(v) == sv.bits(-T[0, p2] / T[r, p2]), (r, which, p1, p2)
        signs.add((which, bool(np.signbit(v))))
    assert len(signs) == 4


def test_planted_zero_ties_in_slack_columns(engine):
    T, x, z, plants = rc.col_zero_ties()
    rep, want = _check(engine, "col_zero_ties", T, x, z, numpy_ref=True)
    n = T.shape[1] - T.shape[0]
    signs = set()
    for (c, which, r1, r2) in plants:
        v = (rep.rhs_lo if which == "lo" else rep.rhs_hi)[c - 1]
        assert v == 0.0, (c, which, v)
        assert sv.bits(v) == sv.bits(-T[r2, -1] / T[r2, n + c - 1]), (c, which, r1, r2)
        signs.add((which, bool(np.signbit(v))))
    assert len(signs) == 4


def test_equal_maxima_and_coverage(engine):
    T, x, z = rc.equal_maxima()
    rep, _ = _check(engine, "equal_maxima", T, x, z)
    assert (rep.cost_lo[:T.shape[0] - 1] == 100.0).all()
    T, x, z = rc.coverage()
    rep, _ = _check(engine, "coverage", T, x, z)
    for lo, hi in ((rep.cost_lo[:12], rep.cost_hi[:12]), (rep.rhs_lo, rep.rhs_hi)):
        assert np.isfinite(lo).any() and np.isfinite(hi).any()
        assert (lo == -math.inf).any() and (hi == math.inf).any()
    assert set(rep.kind.tolist()) == {0, 1, 2, 3}


def test_eps_boundary(engine):
    T, x, z, vals = rc.eps_boundary()
    rep, _ = _check(engine, "eps_boundary", T, x, z)
    up, dn = sv.CLASSES["eps+ulp"], sv.CLASSES["-eps-ulp"]
    m = T.shape[0] - 1
    assert rep.cost_lo[0] == -T[0, m + vals.index(up)] / up
    assert rep.cost_hi[0] == -T[0, m + vals.index(dn)] / dn
    assert rep.cost_lo[6] == -math.inf and rep.cost_hi[6] == math.inf
    assert rep.rhs_lo[2] == -T[1 + vals.index(up), -1] / up
    assert rep.rhs_hi[2] == -T[1 + vals.index(dn), -1] / dn
    assert rep.rhs_lo[3] == -math.inf and rep.rhs_hi[3] == math.inf


def test_non_finite_data(engine):
    """m = 40 rows (two tile rows), 641 columns (two tile columns): `end` 0 / 1 of a case is the
    first / last tile."""
    m, ne = 40, 560
    assert m > rc.TILE_ROWS and 2 * m + ne > rc.TILE_COLS
    nan_reports = 0
    for name, T, x, z in rc.nonfinite_cases(m, ne):
        rep, _ = _check(engine, name, T, x, z, numpy_ref=True)
        ranges = np.concatenate([rep.cost_lo, rep.cost_hi, rep.rhs_lo, rep.rhs_hi])
        nan_reports += bool(np.isnan(ranges).any())
        if name == "nan_entry_skipped":
            assert not np.isnan(ranges).any()
        if name == "nan_quotient_sticks":
            assert np.isnan(rep.cost_lo[:m]).all() and np.isnan(rep.rhs_hi).all()
        if name == "inf_over_inf":
            assert np.isnan(rep.cost_lo[1]) and np.isnan(rep.rhs_lo[1])
    assert nan_reports >= 6


def test_degenerate_bases(engine):
    (n1, T1, x1, z1), (n2, T2, x2, z2) = rc.degenerate_created()
    d = _create(engine, T1, x1, z1)
    assert d.read(tableau=False)[1].tolist()[2] == -1
    rep, _ = assert_report(d, n1)
    assert (rep.kind == ref.BASIC).sum() == 5 and rep.kind[2] != ref.BASIC
    d.destroy()
    d = _create(engine, T2, x2, z2)
    assert 10 not in d.read(tableau=False)[1].tolist() and d.basic_row(10) == 2
    rep, _ = assert_report(d, n2)
    assert rep.kind[10] < ref.BASIC and rep.var_row[10] == -1 and rep.kind[1] == ref.BASIC
    d.destroy()
    # a basicVars entry whose column is no unit column any more: reached through an edit
    T, x, z, (k, new_b) = rc.row_not_found_script()
    d = _create(engine, T, x, z)
    assert d.change_rhs(k, new_b) == 0
    assert 0 in d.read(tableau=False)[1].tolist() and d.basic_row(0) == -1
    rep, _ = assert_report(d, "row_not_found")
    assert rep.kind[0] == ref.BASIC_ROW_NOT_FOUND and rep.var_row[0] == -1
    assert rep.cost_lo[0] == -math.inf and rep.cost_hi[0] == math.inf
    d.destroy()


def test_after_edits(engine, oracle):
    """add_activity shifts the slack block, add_constraint grows rows and columns, change_rhs may
    be rolled back: the report follows the handle's state after every edit and never changes it."""
    seen_ops, rolled_back = set(), 0
    for name, base, ops in sens_cases.scripts(oracle)[:3]:
        T, x, z, basis = base
        d = _create(engine, T, x, z)
        assert_report(d, (name, "ctor"))
        for k, (op, args) in enumerate(ops):
            op, args = sens_cases.materialize(op, args, d.read()[0], k)
            shape0 = d.shape()[:2]
            oc = getattr(d, op)(*args)
            rolled_back += oc == 8
            if op == "add_activity" and oc == 0:
                assert d.shape()[:2] == (shape0[0], shape0[1] + 1)
            if op == "add_constraint" and oc == 0:
                assert d.shape()[:2] == (shape0[0] + 1, shape0[1] + 1)
            assert_report(d, (name, k, op, oc))
            seen_ops.add(op)
        d.destroy()
    assert {"add_activity", "add_constraint", "change_rhs"} <= seen_ops and rolled_back >= 1


@pytest.mark.parametrize("m,n,seed", [(4, 6, 0), (16, 24, 4), (96, 160, 7)])
def test_solved_models_and_the_mirror_text(engine, oracle, m, n, seed):
    from lpr_381_group_v22_amd.sensitivity_analyzer import SensitivityAnalyzer
    T, x, z, basis = sens_cases.solved_lp(oracle, m, n, seed)
    an = SensitivityAnalyzer(T, x, z, engine=engine)
    rep, want = assert_report(an._s, ("solved", m, n), numpy_ref=m > 16)
    # the per-index mirror folds with Python's max / min: it agrees with the report only without
    # NaN and without zero quotients -- the precondition of the text comparison
    ranges = np.concatenate([rep.cost_lo, rep.cost_hi, rep.rhs_lo, rep.rhs_hi])
    assert not np.isnan(ranges).any() and not (ranges == 0.0).any()
    assert not np.isnan(T).any()
    an.Out.clear()
    an.DisplayRangingReport()
    got = list(an.Out)
    an.Out.clear()
    basic = set(an.basicVars)
    for j in range(T.shape[1] - 1):
        (an.DisplayRangeBasic if j in basic else an.DisplayRangeNonBasic)(j + 1)
    for k in range(1, T.shape[0]):
        an.DisplayRangeRHS(k)
    assert got == an.Out
    assert len(got) == 2 * (T.shape[1] - 1) + 3 * (T.shape[0] - 1)
    an._s.destroy()


def test_null_output_pointers(engine):
    from lpr_381_group_v22_amd import _native as N
    T, x, z = rc.coverage()
    d = _create(engine, T, x, z)
    full = d.ranging()
    R, Cc = T.shape
    for pos, f in enumerate(ref.FIELDS):
        size = (Cc - 1) if pos < 5 else (R - 1)
        buf = np.zeros(size, dtype=np.int32 if f in ref.INT_FIELDS else np.float64)
        args = [None] * 9
        args[pos] = buf.ctypes.data_as(C.POINTER(C.c_int32 if f in ref.INT_FIELDS else C.c_double))
        assert N.lib.lpr_sens_ranging(d._h, *args) == 0, f
        if f in ref.INT_FIELDS:
            assert np.array_equal(buf, getattr(full, f)), f
        else:
            sv.assert_same(buf, getattr(full, f), f)
    assert N.lib.lpr_sens_ranging(d._h, *([None] * 9)) == 0
    sweep_ms, finish_ms = d.ranging_times()
    assert sweep_ms > 0.0 and finish_ms > 0.0
    d.destroy()


def test_negative_n_and_bad_handles(engine):
    """n = cols - rows < 0 is LPR_BAD_ARGUMENT.  No handle can hold such a shape (lpr_sens_create
    refuses it, and every edit keeps cols - rows or raises it), so the call's own check is reached
    with a null handle only; tools/ranging_plan_check.cpp covers the plan's refusal on the host."""
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.engine import SensState
    T = np.zeros((5, 4))
    with pytest.raises(N.EngineError) as e:
        SensState.create(engine, T, np.zeros(1), 0.0)
    assert e.value.status == N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_sens_ranging(None, *([None] * 9)) == N.LPR_BAD_ARGUMENT
    a, b = C.c_double(), C.c_double()
    d = _create(engine, *rc.coverage())
    assert N.lib.lpr_sens_ranging_times(d._h, C.byref(a), C.byref(b)) == N.LPR_BAD_ARGUMENT
    d.destroy()
