"""GPU parity tests of the scenario batch built from an LP batch (lpr_sens_batch_from_batch,
DESIGN.md section 20) against the C oracle.  The reference of scenario k is always
`oracle.sens(T, x, z, basis)` on the oracle's own solve of model item[k], followed by script k
alone; the comparison is sens_batch_cases.same_scenario: outcome and pivots per edit, pivot log,
tableau shape and bytes, basicVars, z, and the solution length and bytes.  The fixtures are
tests/sens_model_batch_cases.py, checked on the CPU by test_sens_model_batch_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import ref_py_ranging as ref
import sens_batch_cases as cases
import sens_grow_cases as grow
import sens_model_batch_cases as mc
import special_values as sv

pytestmark = pytest.mark.gpu

FORM_G, FORM_H = 1, 2
VARIANT_G, VARIANT_H = 2, 3
LITERAL_MAX = 3000
NO_ENTRY = -2 ** 31


# ---- helpers -----------------------------------------------------------------------------------------
def _solved_lps(engine, models):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    lps = PrimalSimplexBatch(models, engine=engine)
    lps.Solve()
    return lps


def _solved_tableaux(engine, tableaux):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    lps = PrimalSimplexBatch.from_tableaux(tableaux, engine=engine)
    lps.Solve()
    return lps


def _model_batch(lps, scripts, items=None, **kw):
    from lpr_381_group_v22_amd import SensitivityModelBatch
    return SensitivityModelBatch(lps, scripts, items=items, **kw)


def _check_all(b, refs, shapes, bases, items, name):
    rows, cols, max_rows, max_cols = b.shape_arrays()
    for k, r in enumerate(refs):
        cases.same_scenario(b, k, r, (name, k))
        want = shapes[k][-1] if shapes[k] else bases[items[k]][0].shape
        assert (int(rows[k]), int(cols[k])) == want == b.Shape(k), (name, k)
        assert b.Item(k) == items[k], (name, k)
    assert max_rows >= rows.max() and max_cols >= cols.max(), name
    _, _, basic = b.state_arrays()
    assert basic.shape == (b.Count, max_rows - 1), name
    for k in range(b.Count):
        assert (basic[k, rows[k] - 1:] == NO_ENTRY).all(), (name, k)


def _same_report(got, want, what):
    field = lambda rep, f: rep[f] if isinstance(rep, dict) else getattr(rep, f)
    for f in ref.FIELDS:
        g, w = field(got, f), field(want, f)
        if f in ref.INT_FIELDS:
            assert g.dtype == np.int32 and np.array_equal(g, w), (what, f, g, w)
        else:
            sv.assert_same(g, w, (what, f))


def _refused(lps, count, items, scripts, needle):
    """The raw call is LPR_BAD_ARGUMENT with a message that holds every string of `needle`, and
    returns no handle."""
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.sens_batch import pack_grow_scripts
    p = pack_grow_scripts(scripts)
    h = C.c_void_p(12345)
    iarr = None if items is None else np.asarray(items, dtype=np.int32)
    rc = N.lib.lpr_sens_batch_from_batch(
        lps._h if lps is not None else None, count,
        None if iarr is None else iarr.ctypes.data_as(C.POINTER(C.c_int32)),
        p.nedits.ctypes.data_as(C.POINTER(C.c_int32)),
        p.edits.ctypes.data_as(C.POINTER(N.SensEdit)) if p.edits.size else None,
        p.payload.ctypes.data_as(C.POINTER(C.c_double)) if p.payload.size else None,
        p.payload.size, 0, C.byref(h))
    msg = N.lib.lpr_last_error().decode()
    assert rc == N.LPR_BAD_ARGUMENT, (rc, msg)
    assert not h.value, "a handle was returned"
    assert "lpr_sens_batch_from_batch" in msg, msg
    for s in needle:
        assert s in msg, (s, msg)
    return msg


@pytest.fixture(scope="module")
def mixed(oracle):
    models, bases, items, ops_list = mc.mixed_case(oracle)
    return (models, bases, items) + mc.follow_all(oracle, bases, items, ops_list)


@pytest.fixture(scope="module")
def every_op(oracle):
    models, bases, items, ops_list = mc.every_op_case(oracle)
    return (models, bases, items) + mc.follow_all(oracle, bases, items, ops_list)


# ---- 1. the constructor alone ------------------------------------------------------------------------------
def test_constructor_only(engine, oracle):
    from lpr_381_group_v22_amd import optimal_items
    from lpr_381_group_v22_amd.engine import SensState
    models = mc.shape_models()
    bases = [mc.solved(oracle, mdl) for mdl in models]
    lps = _solved_lps(engine, models)
    assert optimal_items(lps) == list(range(len(models)))
    b = _model_batch(lps, [[] for _ in models])          # items None: scenario k is LP k
    assert b.Count == len(models) and b.TotalEdits == 0
    assert (b.Rows, b.Cols) == (max(t[0].shape[0] for t in bases), max(t[0].shape[1] for t in bases))
    rows, cols, max_rows, max_cols = b.shape_arrays()
    assert (max_rows, max_cols) == (b.Rows, b.Cols)
    z, ns, basic = b.state_arrays()
    arr = b.ranging_arrays()
    assert b.ConstructTime() > 0.0
    for k, base in enumerate(bases):
        T, x, zk, basis = base
        st = oracle.sens(T, x, zk, basis).state()
        assert b.Shape(k) == T.shape == (int(rows[k]), int(cols[k])), k
        assert b.Tableau(k).tobytes() == st["T"].tobytes(), k
        assert b.Solution(k).tobytes() == st["sol"].tobytes() and ns[k] == len(x), k
        assert z[k] == st["z"] == T[0, -1], k
        assert basic[k, :T.shape[0] - 1].tolist() == st["basic"], k
        assert (basic[k, T.shape[0] - 1:] == NO_ENTRY).all(), k
        assert b.Outcomes(k) == [] and b.LogCount(k) == 0, k
        fn = ref.report_literal if T.size <= LITERAL_MAX else ref.report_numpy
        want = fn(st["T"], st["basic"])
        _same_report(b.Ranging(k), want, (k, "restatement"))
        for f in ref.FIELDS:                              # the padded arrays themselves
            a = getattr(arr, f)[k]
            own = (T.shape[1] if f in cases_column_fields() else T.shape[0]) - 1
            assert (a[own:] == NO_ENTRY).all() if f in ref.INT_FIELDS else np.isnan(a[own:]).all()
        d = SensState.create(engine, T, x, zk)
        _same_report(b.Ranging(k), d.ranging(), (k, "single handle"))
        d.destroy()
    b.destroy()
    lps.destroy()


def cases_column_fields():
    from lpr_381_group_v22_amd.sens_batch import RANGING_COLUMN_FIELDS
    return RANGING_COLUMN_FIELDS


# ---- 2. mixed shapes in one batch -----------------------------------------------------------------------
def test_mixed_shapes_in_one_batch(engine, mixed):
    models, bases, items, scripts, refs, shapes = mixed
    lps = _solved_lps(engine, models)
    b = _model_batch(lps, scripts, items=items)
    res = b.Run()
    assert res.finished == len(scripts) and res.running == 0 and res.form == FORM_G
    assert res.pivots == sum(sum(r[2]) for r in refs)
    _check_all(b, refs, shapes, bases, items, "mixed")
    rows, cols, _, _ = b.shape_arrays()
    assert {3, 6, 21, 63, 64, 65, 98} <= {bases[it][0].shape[1] for it in items}
    assert len(set(zip(rows.tolist(), cols.tolist()))) >= 8
    twice = [k for k, it in enumerate(items) if it == 2]
    assert len(twice) == 3 and len({b.Tableau(k).tobytes() for k in twice}) == 3
    b.destroy()
    lps.destroy()


# ---- 3. every op on differing bases ----------------------------------------------------------------------
def test_every_op_on_differing_bases(engine, every_op):
    models, bases, items, scripts, refs, shapes = every_op
    lps = _solved_lps(engine, models)
    b = _model_batch(lps, scripts, items=items)
    res = b.Run()
    assert res.finished == len(scripts) and res.running == 0
    _check_all(b, refs, shapes, bases, items, "every op")
    seen = set(b.outcome_arrays()[0].tolist())
    assert {0, 1, 2, 8, -1} <= seen, seen
    rows, cols, _, _ = b.shape_arrays()
    growth = {(int(rows[k]) - bases[it][0].shape[0], int(cols[k]) - bases[it][0].shape[1])
              for k, it in enumerate(items)}
    assert {(0, 0), (0, 1), (1, 2), (1, 1), (2, 3)} <= growth, growth
    b.destroy()
    lps.destroy()


# ---- 4. where ExtractSolution and the rebuild see different things ---------------------------------------
def test_extract_solution_and_rebuild_disagree(engine, oracle):
    named = mc.disagreement_tableaux()
    lps = _solved_tableaux(engine, [T for _, T in named])
    assert [int(s) for s in lps.Status] == [0] * len(named) and sum(lps.Iterations) == 0
    bases = [mc.tableau_base(oracle, T) for _, T in named]
    items, ops_list = [], []
    for it, (_, T) in enumerate(named):
        for ops in mc.tableau_ops(T):
            items.append(it)
            ops_list.append(ops)
    scripts, refs, shapes = mc.follow_all(oracle, bases, items, ops_list)
    b = _model_batch(lps, scripts, items=items)
    z, ns, basic = b.state_arrays()                      # before the run: the constructor's state
    for k, it in enumerate(items):
        st = oracle.sens(*bases[it]).state()
        R = bases[it][0].shape[0]
        assert basic[k, :R - 1].tolist() == st["basic"], (named[it][0], k)
        assert b.Solution(k).tobytes() == st["sol"].tobytes(), (named[it][0], k)
        assert ns[k] == bases[it][0].shape[1] - R and z[k] == st["z"], (named[it][0], k)
    first = {name: items.index(it) for it, (name, _) in enumerate(named)}
    assert basic[first["twin_unit_columns"], :3].tolist() == [0, 1, -1]
    assert b.Solution(first["two_ones_in_a_column"])[:2].tolist() == [0.0, 0.0]
    assert b.Run().running == 0
    _check_all(b, refs, shapes, bases, items, "disagree")
    b.destroy()
    lps.destroy()


# ---- 5. forms ------------------------------------------------------------------------------------------------
def test_forms(engine, oracle):
    models, bases, items, ops_list, shared = mc.forms_case(oracle)
    scripts, refs, shapes = mc.follow_all(oracle, bases, items, ops_list)
    lps = _solved_lps(engine, models)
    h = _model_batch(lps, scripts, items=items)
    res = h.Run()
    assert res.form == FORM_H and res.running == 0       # the 200 x 300 LP sizes every slice
    _check_all(h, refs, shapes, bases, items, "with the large LP")
    sub = [scripts[k] for k in shared]
    sub_items = [items[k] for k in shared]
    g = _model_batch(lps, sub, items=sub_items)
    assert g.Run().form == FORM_G
    f = _model_batch(lps, sub, items=sub_items)
    assert f.Run(variant=VARIANT_H).form == FORM_H       # forcing works
    f2 = _model_batch(lps, sub, items=sub_items)
    assert f2.Run(variant=VARIANT_G).form == FORM_G
    lps.destroy()
    for q, k in enumerate(shared):
        for other, kk in ((h, k), (f, q), (f2, q)):
            assert g.Tableau(q).tobytes() == other.Tableau(kk).tobytes(), (q, k)
            assert g.Solution(q).tobytes() == other.Solution(kk).tobytes(), (q, k)
            assert g.Log(q) == other.Log(kk) and g.Outcomes(q) == other.Outcomes(kk), (q, k)
            assert g.State(q)["basic"] == other.State(kk)["basic"], (q, k)
            assert sv.bits(g.State(q)["z"]) == sv.bits(other.State(kk)["z"]), (q, k)
    for x in (h, g, f, f2):
        x.destroy()


# ---- 6. resume -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [VARIANT_G, VARIANT_H])
def test_resume_one_pivot_per_call(engine, every_op, variant):
    models, bases, items, scripts, refs, shapes = every_op
    lps = _solved_lps(engine, models)
    b = _model_batch(lps, scripts, items=items)
    lps.destroy()
    pivots, calls = 0, 0
    for _ in range(400):
        res = b.Run(max_pivots=1, variant=variant)
        pivots += res.pivots
        calls += 1
        assert res.finished + res.running == len(scripts)
        if res.running == 0:
            break
    assert res.running == 0 and calls > 2
    assert pivots == sum(sum(r[2]) for r in refs)
    _check_all(b, refs, shapes, bases, items, ("resumed", variant))
    b.destroy()


# ---- 7. refusals -------------------------------------------------------------------------------------------------
def test_refusals(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch, optimal_items
    from lpr_381_group_v22_amd import _native as N
    every = mc.shape_models()
    models = [every[1], mc.unbounded_model(), every[2]]
    lps = _solved_lps(engine, models)
    assert lps.Status[1] == N.LPR_UNBOUNDED and optimal_items(lps) == [0, 2]
    one = [[("resolve_all", ())]]
    _refused(lps, 3, None, one * 3, ["scenario 1", "item 1", "unbounded"])       # among the items
    _refused(lps, 1, [1], one, ["scenario 0", "item 1"])
    _refused(lps, 2, [0, 3], one * 2, ["scenario 1", "item 3"])                   # out of range
    _refused(lps, 1, [-1], one, ["scenario 0", "item -1"])
    _refused(lps, 2, None, one * 2, ["count=2"])                                  # NULL items
    _refused(lps, 0, [0], one, [])                                                # count < 1
    _refused(None, 1, [0], one, ["null or orphaned"])
    # the op and payload errors of the grow create, naming scenario, item and edit
    h = C.c_void_p()
    nedits = (C.c_int32 * 2)(0, 2)
    ed = (N.SensEdit * 2)(N.SensEdit(op=0), N.SensEdit(op=5, a=60, b=2, v=1.0))
    pool = (C.c_double * 4)(0.5, 0.5, 0.5, 0.5)
    it = (C.c_int32 * 2)(2, 0)
    rc = N.lib.lpr_sens_batch_from_batch(lps._h, 2, it, nedits, ed, pool, 4, 0, C.byref(h))
    msg = N.lib.lpr_last_error().decode()
    assert rc == N.LPR_BAD_ARGUMENT and "scenario 1" in msg and "item 0" in msg and "edit 1" in msg
    ed[1].op = 7
    rc = N.lib.lpr_sens_batch_from_batch(lps._h, 2, it, nedits, ed, pool, 4, 0, C.byref(h))
    assert rc == N.LPR_BAD_ARGUMENT and "op 7" in N.lib.lpr_last_error().decode()
    assert not h.value
    # the LP batch is still usable: the optimal items make a batch
    good = optimal_items(lps)
    b = _model_batch(lps, [[("resolve_all", ())] for _ in good], items=good)
    assert b.Run().running == 0 and b.Outcomes(0) == [0]
    b.destroy()
    assert lps.GetFinalTableau(0).tobytes() == mc.solved(oracle, models[0])[0].tobytes()
    lps.destroy()

    # an unsolved batch, then one stopped by max_pivots
    lps = PrimalSimplexBatch([every[1], mc.many_pivot_model()], engine=engine)
    _refused(lps, 2, None, one * 2, ["scenario 0", "item 0", "not solved"])
    lps.Solve(max_pivots=1)
    assert lps.Status[1] == N.LPR_PIVOT_LIMIT
    _refused(lps, 1, [1], one, ["scenario 0", "item 1", "pivot limit"])
    lps.Solve()
    assert optimal_items(lps) == [0, 1]                                           # usable afterwards
    b = _model_batch(lps, one * 2)
    assert b.Run().running == 0
    b.destroy()
    lps.destroy()

    # cols < rows, and a script that grows its own base past 1024 x 2048
    lps = _solved_tableaux(engine, [mc.tall_tableau(), mc.wide_optimal_tableau(),
                                    mc.twin_unit_columns()])
    assert [int(s) for s in lps.Status] == [0, 0, 0]
    _refused(lps, 1, [0], one, ["scenario 0", "item 0", "4 x 3"])
    grow_one = [[("add_activity", (1.0, [0.5, 0.5]))]]
    _refused(lps, 2, [2, 1], [[]] + grow_one, ["scenario 1", "item 1", "1024 x 2048"])
    b = _model_batch(lps, [[], []], items=[1, 2])                                 # without growth: fine
    assert b.Shape(0) == (3, 2048) and b.Shape(1) == (4, 9)
    assert b.Tableau(0).tobytes() == mc.wide_optimal_tableau().tobytes()
    b.destroy()
    lps.destroy()


# ---- 8. lifetime ---------------------------------------------------------------------------------------------------
def test_lp_batch_destroyed_right_after_the_create(engine, mixed):
    models, bases, items, scripts, refs, shapes = mixed
    lps = _solved_lps(engine, models)
    b = _model_batch(lps, scripts, items=items, log_cap=2)
    lps.destroy()
    other = _solved_lps(engine, models[::-1])            # the freed slab may be handed out again
    assert b.Run().running == 0
    assert b.LogCap == 2
    _check_all(b, refs, shapes, bases, items, "lifetime")
    other.destroy()
    b.destroy()


# ---- 9. the old creates share the rebuild ------------------------------------------------------------------------------
def test_old_creates_are_unchanged(engine, oracle):
    from lpr_381_group_v22_amd import SensitivityBatch, SensitivityGrowBatch
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.engine import SensState
    for name, base, scripts in cases.all_edit_cases(oracle)[:2] + cases.all_edit_cases(oracle)[-3:]:
        d = SensState.create(engine, *base[:3])
        b = SensitivityBatch(d, scripts)
        d.destroy()
        assert b.Run().running == 0
        for k, script in enumerate(scripts):
            cases.same_scenario(b, k, cases.oracle_run(oracle, base, script), (name, k))
        ms = C.c_double()
        assert N.lib.lpr_sens_batch_from_batch_time(b._h, C.byref(ms)) == N.LPR_BAD_ARGUMENT
        b.destroy()
    base, ops_list = grow.mixed_shapes(oracle)
    got = [grow.follow(oracle, base, ops) for ops in ops_list]
    d = SensState.create(engine, *base[:3])
    b = SensitivityGrowBatch(d, [g[0] for g in got])
    d.destroy()
    assert b.Run().running == 0
    for k, g in enumerate(got):
        cases.same_scenario(b, k, g[1], ("grow", k))
        assert b.Shape(k) == (g[2][-1] if g[2] else base[0].shape)
    b.destroy()
