"""GPU parity tests of the scenario batch's sensitivity report (lpr_sens_batch_ranging, DESIGN.md
section 19) against tests/ref_py_ranging.py: doubles under the parity comparator (NaN positions
identical, every other element identical in all 64 bits, the sign of zero included), ints exactly.
The reference of scenario k is always computed on the state read back from the same batch --
Tableau(k) and state_arrays() -- so it sees what the device holds: the literal restatement up to
LITERAL_MAX tableau entries, the vectorised one above (test_ranging_cpu.py holds the two against
each other).  Where the shapes allow, the independent route is compared as well: a fresh SensState
on the base, the same edits one after another, then ranging().

The kernel's mapping (csrc/sens_batch_ranging_common.hpp; restated below, read back from the header
by test_sens_batch_ranging_cpu.py): one workgroup of LANES per scenario; the column pass gives lane
l the columns l, l + LANES, ... and walks each down all rows in scan order (nothing is cut); the
row pass gives wave w the rows 1 + w, 1 + w + WAVES, ... and lane l of it the columns l,
l + WAVE_LANES, ..., LOAD at a time, combined over the lanes by (value, column).  So the sizes at
which the code takes another path are C - 1 around WAVE_LANES, LOAD * WAVE_LANES and LANES, and m
around WAVES and 2 WAVES."""
import ctypes as C
import math

import numpy as np
import pytest

import ranging_cases as rc
import ref_py_ranging as ref
import sens_batch_cases as cases
import sens_cases
import sens_grow_cases as grow
import special_values as sv

pytestmark = pytest.mark.gpu

LANES, WAVE_LANES, WAVES, LOAD = 256, 64, 4, 4
FORM_G, FORM_H = 1, 2
VARIANT_G, VARIANT_H = 2, 3
LITERAL_MAX = 3000
COLUMN_FIELDS = ("kind", "var_row", "reduced_cost", "cost_lo", "cost_hi")
NO_ENTRY = -2 ** 31


# ---- helpers ---------------------------------------------------------------------------------------
def _handle(engine, base, prefix=()):
    from lpr_381_group_v22_amd.engine import SensState
    T, x, z = base[:3]
    d = SensState.create(engine, T, x, z)
    for op, args in prefix:
        getattr(d, op)(*args)
    return d


def _batch(engine, base, scripts, prefix=(), grow_batch=False, **kw):
    """(batch, the base handle's own ranging()) -- the handle is destroyed before the batch runs."""
    from lpr_381_group_v22_amd import SensitivityBatch, SensitivityGrowBatch
    d = _handle(engine, base, prefix)
    b = (SensitivityGrowBatch if grow_batch else SensitivityBatch)(d, scripts, **kw)
    single = d.ranging()
    d.destroy()
    return b, single


def _snapshot(b):
    """Everything a later run depends on or a read returns: tableaux, z / counts / basicVars,
    outcomes and pivots per edit, log counts and entries."""
    return ([b.Tableau(k).tobytes() for k in range(b.Count)],
            [a.tobytes() for a in b.state_arrays()],
            [a.tobytes() for a in b.outcome_arrays()],
            [(b.LogCount(k), b.Log(k)) for k in range(b.Count)],
            [b.Solution(k).tobytes() for k in range(b.Count)])


def _same_report(got, want, what):
    field = lambda rep, f: rep[f] if isinstance(rep, dict) else getattr(rep, f)
    for f in ref.FIELDS:
        g, w = field(got, f), field(want, f)
        if f in ref.INT_FIELDS:
            assert g.dtype == np.int32 and np.array_equal(g, w), (what, f, g, w)
        else:
            sv.assert_same(g, w, (what, f))


def check_batch(b, what, snapshot=True):
    """One ranging_arrays() call against the restatement on every scenario's read-back state, the
    padding fill and the trimmed Ranging(k) of the first and last scenario; the call must leave the
    batch as it was.  Returns (padded arrays, [restatement per scenario])."""
    before = _snapshot(b) if snapshot else None
    arr = b.ranging_arrays()
    if snapshot:
        assert _snapshot(b) == before, (what, "the call changed the batch")
    rows, cols, max_rows, max_cols = b._shape_read()
    _, _, basic = b.state_arrays()
    assert basic.shape == (b.Count, max_rows - 1), what
    wants = []
    for k in range(b.Count):
        R, Cc = int(rows[k]), int(cols[k])
        T = b.Tableau(k)
        assert T.shape == (R, Cc), (what, k)
        fn = ref.report_literal if R * Cc <= LITERAL_MAX else ref.report_numpy
        want = fn(T, basic[k, :R - 1].tolist())
        wants.append(want)
        for f in ref.FIELDS:
            a = getattr(arr, f)
            is_col = f in COLUMN_FIELDS
            assert a.shape == (b.Count, (max_cols if is_col else max_rows) - 1), (what, f)
            own = (Cc if is_col else R) - 1
            if f in ref.INT_FIELDS:
                assert a.dtype == np.int32 and np.array_equal(a[k, :own], want[f]), (what, k, f)
                assert (a[k, own:] == NO_ENTRY).all(), (what, k, f, "padding")
            else:
                assert a.dtype == np.float64
                sv.assert_same(a[k, :own], want[f], (what, k, f))
                assert np.isnan(a[k, own:]).all(), (what, k, f, "padding")
    for k in sorted({0, b.Count - 1}):
        _same_report(b.Ranging(k), wants[k], (what, k, "Ranging(k)"))
    return arr, wants


def _edits_for(T):
    """Three cheap scripts on any base: none, a re-solve, an RHS change of the last constraint."""
    return [[], [("resolve_all", ())], [("change_rhs", (T.shape[0] - 1, 1.25))]]


def _base_and_edited(engine, name, T, x, z, max_pivots=8, scripts=None, **run_kw):
    """A batch of the base itself plus edited scenarios: the report before the first run (every
    scenario is the base: equal to the handle's own ranging()), then after a bounded run."""
    scripts = _edits_for(T) if scripts is None else scripts
    b, single = _batch(engine, (T, x, z), scripts)
    arr, wants = check_batch(b, (name, "before the run"))
    for k in range(b.Count):
        _same_report({f: getattr(arr, f)[k] for f in ref.FIELDS}, single, (name, k, "base"))
    res = b.Run(max_pivots=max_pivots, **run_kw)
    arr, wants = check_batch(b, (name, "after the run"))
    _same_report({f: getattr(arr, f)[0] for f in ref.FIELDS}, single, (name, "0-edit scenario"))
    b.destroy()
    return arr, wants, single, res


# ---- shapes ------------------------------------------------------------------------------------------
def _small_bases():
    out = []
    T, x, z = rc.dense(1, 0, 201)
    out.append(("2x2", np.ascontiguousarray(T[:, 1:]), np.zeros(0), z))     # m = 1, n = 0
    out.append(("2x3", T, x, z))
    T, x, z = rc.dense(3, 0, 202)
    out.append(("4x6", np.ascontiguousarray(T[:, 1:]), np.zeros(2), z))     # row 1 has no unit column
    return out


def test_tiny_bases(engine):
    seen = set()
    for name, T, x, z in _small_bases():
        _base_and_edited(engine, name, T, x, z)
        seen.add(T.shape)
    assert seen == {(2, 2), (2, 3), (4, 6)}


@pytest.mark.parametrize("w", [63, 64, 65, 255, 256, 257, 511, 513])
def test_widths_around_the_lane_strides(engine, w):
    assert {WAVE_LANES - 1, WAVE_LANES + 1, LANES - 1, LANES, LANES + 1, 2 * LANES + 1} <= \
        {63, 64, 65, 255, 256, 257, 511, 513} and LOAD * WAVE_LANES == LANES
    m = 5
    T, x, z = rc.dense(m, w - 2 * m, 210 + w)
    assert T.shape == (m + 1, w + 1)
    arr, wants, _, _ = _base_and_edited(engine, "width_%d" % w, T, x, z)
    assert (wants[0]["kind"] == ref.BASIC).sum() == m


def test_heights_around_the_wave_count(engine):
    for m in (WAVES - 1, WAVES, WAVES + 1, 2 * WAVES - 1, 2 * WAVES, 2 * WAVES + 1,
              LOAD + 1, 2 * LOAD + 1):
        T, x, z = rc.dense(m, 3, 230 + m)
        arr, wants, _, _ = _base_and_edited(engine, "height_%d" % m, T, x, z)
        assert (wants[0]["kind"] == ref.BASIC).sum() == m


def test_h_sized_base_with_three_scenarios(engine):
    T, x, z = rc.dense(199, 1300 - 1 - 2 * 199, 81)
    assert T.shape == (200, 1300)
    scripts = [[], [("change_nonbasic_cbar", (700, -0.5))], [("change_rhs", (150, 2.5))]]
    arr, wants, _, res = _base_and_edited(engine, "200x1300", T, x, z, max_pivots=4,
                                          scripts=scripts)
    assert res.form == FORM_H and res.pivots > 0
    assert not all(sv.same(getattr(arr, f)[1], getattr(arr, f)[0]) for f in ref.FIELDS)


# ---- forms -------------------------------------------------------------------------------------------
def test_both_sides_of_the_g_h_boundary(engine):
    ne = cases.largest_g_extra(60)
    for extra, form in ((ne, FORM_G), (ne + 1, FORM_H)):
        base, scripts = cases.threshold_case(60, extra, 41)
        b, _ = _batch(engine, base, scripts + [[]])
        res = b.Run()
        assert res.form == form and res.running == 0 and res.pivots > 0
        check_batch(b, ("threshold", form))
        b.destroy()


def test_forced_forms_give_the_same_report(engine, oracle):
    base, scripts = cases.rhs_sweep(oracle)
    reports = {}
    for variant, form in ((VARIANT_G, FORM_G), (VARIANT_H, FORM_H)):
        b, _ = _batch(engine, base, scripts)
        assert b.Run(variant=variant).form == form
        arr, _ = check_batch(b, ("forced", form))
        reports[form] = arr
        b.destroy()
    for f in ref.FIELDS:
        g, h = getattr(reports[FORM_G], f), getattr(reports[FORM_H], f)
        assert np.array_equal(g, h) if f in ref.INT_FIELDS else sv.same(g, h), f


# ---- scan order ----------------------------------------------------------------------------------------
def test_planted_zero_ties_in_rows(engine):
    T, x, z, plants = rc.row_zero_ties()
    arr, wants, single, _ = _base_and_edited(engine, "row_zero_ties", T, x, z)
    signs = set()
    for (r, which, p1, p2) in plants:
        v = (arr.cost_lo if which == "lo" else arr.cost_hi)[0, r - 1]
        assert v == 0.0 and sv.bits(v) == sv.bits(-T[0, p2] / T[r, p2]), (r, which, p1, p2)
        signs.add((which, bool(np.signbit(v))))
    assert len(signs) == 4


# Column pairs by what separates them in THIS kernel's row pass (lane = column % 64, 4 columns of a
# lane per load group), each class in both sign orders (pair k even: (-0, +0), odd: (+0, -0)):
OWN_ROW_PAIRS = [(70, 134), (72, 136),       # one lane, neighbours in one load group
                 (74, 266), (76, 268),       # one lane, the last of a group and the first of the next
                 (78, 334), (80, 592),       # one lane, two load groups
                 (150, 193), (152, 195),     # the LATER column in a LOWER lane, shuffle distance 1..32
                 (90, 186), (92, 188),       # lanes 26 / 58: met at the first shuffle step (xor 32)
                 (100, 101), (102, 103),     # met at the last shuffle step (xor 1)
                 (256, 1023), (320, 1087)]   # lane 0 against lane 63, far apart
OWN_COL_PAIRS = [(2, 3), (6, 7),             # the column pass walks down in scan order; its only
                 (4, 5), (8, 9)]             # seams are the division pairs and the load groups of 4


def test_zero_ties_at_this_kernels_own_seams(engine, monkeypatch):
    for p1, p2 in OWN_ROW_PAIRS[:6]:
        assert p1 % WAVE_LANES == p2 % WAVE_LANES
    assert all(p1 % WAVE_LANES > p2 % WAVE_LANES for p1, p2 in OWN_ROW_PAIRS[6:8])
    assert all((p1 % WAVE_LANES) ^ (p2 % WAVE_LANES) == 32 for p1, p2 in OWN_ROW_PAIRS[8:10])
    monkeypatch.setattr(rc, "ROW_PAIRS", OWN_ROW_PAIRS)
    T, x, z, plants = rc.row_zero_ties()
    arr, _, _, _ = _base_and_edited(engine, "own_row_ties", T, x, z)
    signs = set()
    for (r, which, p1, p2) in plants:
        v = (arr.cost_lo if which == "lo" else arr.cost_hi)[0, r - 1]
        assert v == 0.0 and sv.bits(v) == sv.bits(-T[0, p2] / T[r, p2]), (r, which, p1, p2)
        signs.add((which, bool(np.signbit(v))))
    assert len(signs) == 4
    monkeypatch.setattr(rc, "COL_PAIRS", OWN_COL_PAIRS)
    T, x, z, plants = rc.col_zero_ties()
    arr, _, _, _ = _base_and_edited(engine, "own_col_ties", T, x, z)
    n = T.shape[1] - T.shape[0]
    signs = set()
    for (c, which, r1, r2) in plants:
        v = (arr.rhs_lo if which == "lo" else arr.rhs_hi)[0, c - 1]
        assert v == 0.0 and sv.bits(v) == sv.bits(-T[r2, -1] / T[r2, n + c - 1]), (c, which)
        signs.add((which, bool(np.signbit(v))))
    assert len(signs) == 4


def test_planted_zero_ties_in_slack_columns(engine):
    T, x, z, plants = rc.col_zero_ties()
    arr, _, _, _ = _base_and_edited(engine, "col_zero_ties", T, x, z)
    n = T.shape[1] - T.shape[0]
    signs = set()
    for (c, which, r1, r2) in plants:
        v = (arr.rhs_lo if which == "lo" else arr.rhs_hi)[0, c - 1]
        assert v == 0.0 and sv.bits(v) == sv.bits(-T[r2, -1] / T[r2, n + c - 1]), (c, which)
        signs.add((which, bool(np.signbit(v))))
    assert len(signs) == 4


def test_equal_maxima_and_eps_boundary(engine):
    T, x, z = rc.equal_maxima()
    arr, _, _, _ = _base_and_edited(engine, "equal_maxima", T, x, z)
    assert (arr.cost_lo[0, :T.shape[0] - 1] == 100.0).all()
    T, x, z, vals = rc.eps_boundary()
    arr, _, _, _ = _base_and_edited(engine, "eps_boundary", T, x, z)
    up, dn = sv.CLASSES["eps+ulp"], sv.CLASSES["-eps-ulp"]
    m = T.shape[0] - 1
    assert arr.cost_lo[0, 0] == -T[0, m + vals.index(up)] / up
    assert arr.cost_hi[0, 0] == -T[0, m + vals.index(dn)] / dn
    assert arr.cost_lo[0, 6] == -math.inf and arr.cost_hi[0, 6] == math.inf
    assert arr.rhs_lo[0, 2] == -T[1 + vals.index(up), -1] / up
    assert arr.rhs_hi[0, 2] == -T[1 + vals.index(dn), -1] / dn
    assert arr.rhs_lo[0, 3] == -math.inf and arr.rhs_hi[0, 3] == math.inf


def test_non_finite_data(engine):
    """m = 6 rows (more than one row per wave), 313 columns (past LANES and past one load group of
    the row pass): `end` 0 / 1 of a case is the first / last lane stride."""
    m, ne = 6, 300
    assert m > WAVES and 2 * m + ne > LANES
    nan_reports = 0
    for name, T, x, z in rc.nonfinite_cases(m, ne):
        arr, _, _, _ = _base_and_edited(engine, name, T, x, z, max_pivots=4,
                                        scripts=[[], [("resolve_all", ())]])
        ranges = np.concatenate([arr.cost_lo[0], arr.cost_hi[0], arr.rhs_lo[0], arr.rhs_hi[0]])
        nan_reports += bool(np.isnan(ranges).any())
        if name == "nan_entry_skipped":
            assert not np.isnan(ranges).any()
        if name == "nan_quotient_sticks":
            assert np.isnan(arr.cost_lo[0, :m]).all() and np.isnan(arr.rhs_hi[0]).all()
        if name == "inf_over_inf":
            assert np.isnan(arr.cost_lo[0, 1]) and np.isnan(arr.rhs_lo[0, 1])
    assert nan_reports >= 6


# ---- stale basis ---------------------------------------------------------------------------------------
def test_stale_basis_is_taken_as_stored(engine):
    """The base is left by an edit with column 0 in basicVars but no unit column any more: a
    rebuild would drop it, the stored basicVars keeps it, and the 0-edit scenario must say so."""
    T, x, z, (k, new_b) = rc.row_not_found_script()
    prefix = [("change_rhs", (k, new_b))]
    scripts = [[], [("change_nonbasic_cbar", (6, 0.5))], [("change_rhs", (1, 6.0))]]
    b, single = _batch(engine, (T, x, z), scripts, prefix=prefix)
    assert single.kind[0] == ref.BASIC_ROW_NOT_FOUND
    for stage in ("before", "after"):
        arr, wants = check_batch(b, ("stale", stage))
        assert 0 in b.state_arrays()[2][0].tolist()
        assert arr.kind[0, 0] == ref.BASIC_ROW_NOT_FOUND and arr.var_row[0, 0] == -1
        assert arr.cost_lo[0, 0] == -math.inf and arr.cost_hi[0, 0] == math.inf
        _same_report({f: getattr(arr, f)[0] for f in ref.FIELDS}, single, ("stale", stage))
        if stage == "before":
            assert b.Run().running == 0
    # the rebuilt scenario (change_nonbasic_cbar rebuilds basicVars) has lost the entry
    assert 0 not in b.state_arrays()[2][1].tolist() and arr.kind[1, 0] != ref.BASIC_ROW_NOT_FOUND
    b.destroy()


# ---- edits -----------------------------------------------------------------------------------------------
def _independent(engine, base, script):
    d = _handle(engine, base)
    for op, args in script:
        getattr(d, op)(*args)
    rep = d.ranging()
    d.destroy()
    return rep


def test_every_scenario_of_the_edit_cases(engine, oracle):
    seen = set()
    for name, base, scripts in cases.all_edit_cases(oracle):
        b, _ = _batch(engine, base, scripts)
        assert b.Run().running == 0
        arr, wants = check_batch(b, name)
        seen |= set(b.outcome_arrays()[0].tolist())
        if name == "rollback":                       # the independent route, edit by edit
            for k, script in enumerate(scripts):
                _same_report({f: getattr(arr, f)[k] for f in ref.FIELDS},
                             _independent(engine, base, script), (name, k, "independent"))
        b.destroy()
    assert {0, 8} <= seen and seen & {1, 2}, seen    # OK, a rollback and a non-OK outcome


def test_rhs_sweep_reports_differ_and_match_single_handles(engine, oracle):
    base, scripts = cases.rhs_sweep(oracle)
    b, _ = _batch(engine, base, scripts)
    assert b.Run().running == 0
    arr, wants = check_batch(b, "sweep")
    assert 8 in b.outcome_arrays()[0].tolist()
    distinct = {tuple(sv.bits(v) for v in arr.rhs_now[k]) for k in range(b.Count)}
    assert len(distinct) >= 2, "every scenario reports the same state: slice 0 read for every k?"
    for k in range(0, b.Count, 3):
        _same_report({f: getattr(arr, f)[k] for f in ref.FIELDS},
                     _independent(engine, base, scripts[k]), ("sweep", k, "independent"))
    b.destroy()


# ---- batch size -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 257])
def test_batch_sizes(engine, count):
    T, x, z, _ = sens_cases.identity_basis(3, 2, 240)    # every new b keeps it feasible: outcome 0
    scripts = [[("change_rhs", (1 + k % 3, 0.5 + 0.25 * k))] if k % 5 else [] for k in range(count)]
    b, _ = _batch(engine, (T, x, z), scripts)
    check_batch(b, ("count", count, "before"), snapshot=count == 1)
    b.Run(max_pivots=6)
    arr, _ = check_batch(b, ("count", count, "after"), snapshot=count == 1)
    if count > 1:
        assert len({arr.rhs_now[k].tobytes() for k in range(count)}) > 10
        assert b.RangingTime() > 0.0
    b.destroy()


# ---- grow batch ---------------------------------------------------------------------------------------------
def test_grow_batch_mixed_shapes(engine, oracle):
    base, ops_list = grow.mixed_shapes(oracle)
    scripts = [grow.follow(oracle, base, ops)[0] for ops in ops_list]
    b, single = _batch(engine, base, scripts, grow_batch=True)
    arr, _ = check_batch(b, "mixed before")          # every scenario is the base, padded to the max
    R, Cc = base[0].shape
    assert arr.kind.shape == (len(scripts), Cc + 3 - 1) and arr.shadow.shape[1] == R + 2 - 1
    assert b.Run().running == 0
    arr, wants = check_batch(b, "mixed after")
    rows, cols, _, _ = b.shape_arrays()
    assert len(set(zip(rows.tolist(), cols.tolist()))) >= 5
    for k in range(b.Count):
        rep = b.Ranging(k)
        assert rep.kind.shape == (cols[k] - 1,) and rep.shadow.shape == (rows[k] - 1,)
        _same_report(rep, wants[k], ("mixed", k))
    _same_report(b.Ranging(2), single, "the empty script is the base")
    b.destroy()


def test_grow_batch_across_lane_strides(engine, oracle):
    for name, base, ops, form in grow.stride_cases():
        script = grow.follow(oracle, base, ops)[0]
        b, _ = _batch(engine, base, [script, [], script[:1]], grow_batch=True)
        res = b.Run()
        assert res.form == form and res.running == 0, name
        arr, wants = check_batch(b, name)
        assert b.Shape(0) != b.Shape(1)
        b.destroy()


# ---- stopped inside an edit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,form", [(VARIANT_G, FORM_G), (VARIANT_H, FORM_H)])
def test_report_between_two_runs(engine, oracle, variant, form):
    """Run(max_pivots=1) leaves the scenarios that pivot stopped inside their edit (in form G
    their tableau is then the alt slice).  Their report is the restatement on the read-back state,
    and asking for it changes nothing: run to the end, everything equals an uninterrupted batch
    that was never asked for a report."""
    base, scripts = cases.rhs_sweep(oracle)
    b, _ = _batch(engine, base, scripts)
    res = b.Run(max_pivots=1, variant=variant)
    assert res.form == form and res.running > 0 and res.finished > 0
    arr, _ = check_batch(b, ("stopped", form))
    res = b.Run(max_pivots=1, variant=variant)       # a second stop, after a resumed run
    arr, _ = check_batch(b, ("stopped twice", form))
    while res.running:
        res = b.Run(variant=variant)
    check_batch(b, ("finished", form))
    plain, _ = _batch(engine, base, scripts)
    assert plain.Run(variant=variant).running == 0
    assert _snapshot(b) == _snapshot(plain)
    b.destroy()
    plain.destroy()


# ---- NULL outputs ----------------------------------------------------------------------------------------------
def test_null_output_pointers(engine, oracle):
    from lpr_381_group_v22_amd import _native as N
    base, scripts = cases.rhs_sweep(oracle)
    b, _ = _batch(engine, base, scripts[:5])
    ms = C.c_double()
    assert N.lib.lpr_sens_batch_ranging_time(b._h, C.byref(ms)) == N.LPR_BAD_ARGUMENT
    b.Run()
    full = b.ranging_arrays()
    R, Cc = base[0].shape

    def buffers():
        out = []
        for f in ref.FIELDS:
            width = (Cc if f in COLUMN_FIELDS else R) - 1
            out.append(np.full((b.Count, width), 77, dtype=np.int32 if f in ref.INT_FIELDS
                               else np.float64))
        return out

    def ptr(a):
        return a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double))

    for skip in range(9):                            # every single pointer NULL in turn
        bufs = buffers()
        args = [None if q == skip else ptr(a) for q, a in enumerate(bufs)]
        assert N.lib.lpr_sens_batch_ranging(b._h, *args) == 0, skip
        for q, f in enumerate(ref.FIELDS):
            if q == skip:
                assert (bufs[q] == 77).all(), f
            elif f in ref.INT_FIELDS:
                assert np.array_equal(bufs[q], getattr(full, f)), f
            else:
                sv.assert_same(bufs[q], getattr(full, f), f)
    for only in range(9):                            # and every single pointer alone
        bufs = buffers()
        args = [ptr(a) if q == only else None for q, a in enumerate(bufs)]
        assert N.lib.lpr_sens_batch_ranging(b._h, *args) == 0, only
        f = ref.FIELDS[only]
        assert np.array_equal(bufs[only], getattr(full, f)) if f in ref.INT_FIELDS else \
            sv.same(bufs[only], getattr(full, f)), f
    assert N.lib.lpr_sens_batch_ranging(b._h, *([None] * 9)) == 0
    assert b.RangingTime() > 0.0
    b.destroy()
    assert N.lib.lpr_sens_batch_ranging(b._h, *([None] * 9)) == N.LPR_BAD_ARGUMENT
