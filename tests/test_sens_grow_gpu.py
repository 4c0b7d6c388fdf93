"""GPU parity tests of the growing scenario batch (lpr_sens_batch_create_grow, DESIGN.md section
14) against the C oracle (oracle/oracle_sens.c): every scenario is compared with the oracle run on
that script alone on a fresh analyzer -- outcome and pivots per edit, pivot log, tableau shape and
bytes, basicVars, z, and the solution length and bytes.  The fixtures are tests/sens_grow_cases.py,
checked on the CPU by test_sens_grow_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import sens_batch_cases as cases
import sens_cases
import sens_grow_cases as grow

pytestmark = pytest.mark.gpu

FORM_G, FORM_H = 1, 2
VARIANT_G, VARIANT_H = 2, 3
NOT_RUN = -100


def _handle(engine, base, prefix=()):
    from lpr_381_group_v22_amd.engine import SensState
    T, x, z, _ = base
    d = SensState.create(engine, T, x, z)
    for op, args in prefix:
        getattr(d, op)(*args)
    return d


def _batch(engine, base, scripts, prefix=(), **kw):
    """A grow batch over a fresh handle holding `base` (after `prefix`); the handle is destroyed
    before the batch runs."""
    from lpr_381_group_v22_amd import SensitivityGrowBatch
    d = _handle(engine, base, prefix)
    b = SensitivityGrowBatch(d, scripts, **kw)
    d.destroy()
    return b


def _follow_all(oracle, base, ops_list, prefix=()):
    """scripts, refs and per-edit shapes of every op list, each alone on a fresh oracle."""
    got = [grow.follow(oracle, base, ops, prefix) for ops in ops_list]
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]


def _check_all(batch, refs, shapes, base, name):
    rows, cols, max_rows, max_cols = batch.shape_arrays()
    for k, ref in enumerate(refs):
        cases.same_scenario(batch, k, ref, (name, k))
        want = shapes[k][-1] if shapes[k] else base[0].shape
        assert (int(rows[k]), int(cols[k])) == want == batch.Shape(k), (name, k)
    assert max_rows >= rows.max() and max_cols >= cols.max(), name
    _, _, basic = batch.state_arrays()
    assert basic.shape == (batch.Count, max_rows - 1), name
    for k in range(batch.Count):
        assert (basic[k, rows[k] - 1:] == -2 ** 31).all(), (name, k)


def _run_and_check(engine, oracle, name, base, ops_list, form=None, prefix=(), **run_kw):
    scripts, refs, shapes = _follow_all(oracle, base, ops_list, prefix)
    b = _batch(engine, base, scripts, prefix)
    res = b.Run(**run_kw)
    assert res.finished == len(scripts) and res.running == 0, name
    if form is not None:
        assert res.form == form, (name, res.form)
    assert res.pivots == sum(sum(r[2]) for r in refs), name
    _check_all(b, refs, shapes, base, name)
    return b, scripts, refs


@pytest.fixture(scope="module")
def edit_cases(oracle):
    """[(name, base, scripts, refs, shapes)] of grow.all_edit_cases and the rollback-across-growth
    script, followed once on the oracle and shared."""
    out = []
    for name, base, ops_list in grow.all_edit_cases(oracle):
        out.append((name, base) + _follow_all(oracle, base, ops_list))
    base, ops = grow.rollback_growth_case()
    out.append(("rollback_growth", base) + _follow_all(oracle, base, [ops, ops[:2], ops[:3]]))
    return out


def test_all_edits_all_outcomes(engine, edit_cases):
    seen = set()
    for name, base, scripts, refs, shapes in edit_cases[:-1]:
        b = _batch(engine, base, scripts)
        res = b.Run()
        assert res.finished == len(scripts) and res.running == 0 and res.form == FORM_G, name
        _check_all(b, refs, shapes, base, name)
        b.destroy()
        for ref in refs:
            seen |= set(ref[1])
        assert refs[-2][1][-4] in (0, 2) and refs[-1][1][-4] == 1, name
    assert {0, 1, 2, 8, -1} <= seen, seen


def test_mixed_shapes_in_one_batch(engine, oracle):
    base, ops_list = grow.mixed_shapes(oracle)
    b, scripts, refs = _run_and_check(engine, oracle, "mixed", base, ops_list, form=FORM_G)
    rows, cols, max_rows, max_cols = b.shape_arrays()
    R, Cc = base[0].shape
    assert (max_rows, max_cols) == (R + 2, Cc + 3)
    assert len(set(zip(rows.tolist(), cols.tolist()))) >= 5
    assert (b.Rows, b.Cols) == (R, Cc)                       # info keeps the base's shape
    assert b.State(2)["T"].tobytes() == base[0].tobytes()    # the empty script: the base
    b.destroy()


def test_stale_base(engine, oracle):
    """basicVars[4] = -1 as stored: add_constraint is outcome 9 and changes nothing, the script
    goes on; add_activity reads the row 0 the prefix's pivot left."""
    base, prefix, _ = cases.stale_base()
    R, Cc = base[0].shape
    ops_list = grow.stale_scripts(Cc - 1, R)
    before = cases.oracle_run(oracle, base, [], prefix)[0].state()
    for variant, form in ((VARIANT_G, FORM_G), (VARIANT_H, FORM_H)):
        b, scripts, refs = _run_and_check(engine, oracle, ("stale", variant), base, ops_list,
                                          form=form, prefix=prefix, variant=variant)
        assert b.Outcomes(0) == [9] and b.Pivots(0) == [0] and b.Outcomes(1)[0] == 9
        st = b.State(0)
        assert st["T"].tobytes() == before["T"].tobytes() and st["basic"] == before["basic"]
        assert st["z"] == before["z"] and st["basic"][4] == -1
        assert b.Outcomes(2) == [0] and b.Shape(2) == (R, Cc + 1)
        b.destroy()


def test_stale_solution_vector_in_ax(engine, oracle):
    base, ops = grow.stale_solution_case()
    for variant in (VARIANT_G, VARIANT_H):
        b, scripts, refs = _run_and_check(engine, oracle, ("stale sol", variant), base,
                                          [ops, ops[:1], ops[:2]], variant=variant)
        assert b.Outcomes(1) == [1] and b.Pivots(1)[0] >= 1
        assert b.Solution(1).tobytes() == np.asarray(base[1], dtype=np.float64).tobytes()
        b.destroy()


@pytest.mark.parametrize("variant,form", [(VARIANT_G, FORM_G), (VARIANT_H, FORM_H)])
def test_snapshot_and_rollback_across_a_growth(engine, edit_cases, variant, form):
    name, base, scripts, refs, shapes = edit_cases[-1]
    b = _batch(engine, base, scripts)
    res = b.Run(variant=variant)
    assert res.form == form and res.running == 0
    _check_all(b, refs, shapes, base, (name, variant))
    assert b.Outcomes(0)[:2] == [0, 8] and b.Outcomes(1) == [0, 8]
    R, Cc = base[0].shape
    assert b.Shape(1) == (R, Cc + 1) and b.Shape(0) == (R + 1, Cc + 2)
    b.destroy()


def test_lane_strides(engine, oracle):
    for name, base, ops, form in grow.stride_cases():
        after = [op for op, _ in ops].index("change_nonbasic_cbar")
        b, scripts, refs = _run_and_check(engine, oracle, name, base,
                                          [ops, ops[:after], ops[:1]], form=form)
        assert sum(b.Pivots(0)[after:]) > 0, name
        b.destroy()


def test_form_boundary(engine, oracle):
    ne = cases.largest_g_extra(60)
    # fits G alone; one add_activity takes the batch's maximal shape past G
    base, ops_list = grow.boundary_case(ne)
    b, _, _ = _run_and_check(engine, oracle, "past G", base, ops_list, form=FORM_H)
    b.destroy()
    b, _, _ = _run_and_check(engine, oracle, "no add: G", base, ops_list[2:], form=FORM_G)
    b.destroy()
    # one column fewer: G holds the grown shape, and both forms give the same bytes
    base, ops_list = grow.boundary_case(ne - 1)
    g, scripts, refs = _run_and_check(engine, oracle, "forced G", base, ops_list, form=FORM_G,
                                      variant=VARIANT_G)
    h, _, _ = _run_and_check(engine, oracle, "forced H", base, ops_list, form=FORM_H,
                             variant=VARIANT_H)
    for k in range(len(scripts)):
        assert g.Tableau(k).tobytes() == h.Tableau(k).tobytes()
        assert g.Solution(k).tobytes() == h.Solution(k).tobytes()
        assert g.Log(k) == h.Log(k)
    assert [a.tobytes() for a in g.state_arrays()] == [a.tobytes() for a in h.state_arrays()]
    assert [a.tobytes() for a in g.outcome_arrays()] == [a.tobytes() for a in h.outcome_arrays()]
    g.destroy()
    h.destroy()


def test_form_g_above_64_kib_plain_then_grow(engine, oracle):
    """A 64 x 129 base (68 360 bytes of dynamic LDS in form G, above the 64 KiB a kernel gets
    without the dynamic-LDS attribute) first under a batch that cannot grow, then under a grow
    batch that adds a column (64 x 130, 68 888 bytes): k_sens_batch<true, false> and
    k_sens_batch<true, true> each need the attribute set for themselves."""
    from lpr_381_group_v22_amd import SensitivityBatch
    from lpr_381_group_v22_amd.sens_batch import footprint_g
    base, scripts = cases.threshold_case(63, 2, 43)
    script = scripts[0][:3]
    assert base[0].shape == (64, 129)
    assert 64 * 1024 < footprint_g(64, 129) < footprint_g(64, 130) <= 159 * 1024
    ref = cases.oracle_run(oracle, base, script)
    assert sum(ref[2]) == 3
    d = _handle(engine, base)
    b = SensitivityBatch(d, [script])
    d.destroy()
    res = b.Run(variant=VARIANT_G)
    assert res.form == FORM_G and res.finished == 1 and res.pivots == 3
    cases.same_scenario(b, 0, ref, "plain, G above 64 KiB")
    b.destroy()
    ops = [("add_activity", grow.activity(99, 1.0)), script[0], script[1]]
    g, _, refs = _run_and_check(engine, oracle, "grow, G above 64 KiB", base, [ops], form=FORM_G,
                                variant=VARIANT_G)
    assert g.Shape(0) == (64, 130) and sum(refs[0][2]) == 3
    g.destroy()


@pytest.mark.parametrize("variant", [VARIANT_G, VARIANT_H])
def test_resumption_one_pivot_per_call(engine, edit_cases, variant):
    """max_pivots = 1 per call until nothing is running: the bytes of one call.  A scenario that
    a call leaves inside an edit has applied that edit, so shape_read must give the shape the
    oracle has after it -- the grown one where the edit is an add."""
    parked_in_growth = 0
    for name, base, scripts, refs, shapes in edit_cases:
        b = _batch(engine, base, scripts)
        off = np.concatenate([[0], np.cumsum(b.nedits)])
        pivots = 0
        for _ in range(400):
            res = b.Run(max_pivots=1, variant=variant)
            pivots += res.pivots
            assert res.finished + res.running == len(scripts), name
            if res.running == 0:
                break
            oc, _ = b.outcome_arrays()
            rows, cols, _, _ = b.shape_arrays()
            for k, script in enumerate(scripts):
                mine = oc[off[k]:off[k + 1]].tolist()
                if NOT_RUN not in mine:
                    continue
                q = mine.index(NOT_RUN)                      # the edit the scenario is inside
                assert (int(rows[k]), int(cols[k])) == shapes[k][q], (name, variant, k, q)
                parked_in_growth += script[q][0] in ("add_activity", "add_constraint")
        assert res.running == 0, name
        assert pivots == sum(sum(r[2]) for r in refs), name
        _check_all(b, refs, shapes, base, ("resumed", name, variant))
        b.destroy()
    assert parked_in_growth > 0, "no call ever stopped inside the re-solve of a growth edit"


def test_against_the_single_handle(engine, oracle):
    """Three scenarios of the mixed batch replayed call by call on a fresh SensState: the same
    bytes.  An add_activity whose column is not rows - 1 long is outcome -1 in the batch (the
    single call refuses it), and nothing changes."""
    base, ops_list = grow.mixed_shapes(oracle)
    picks = [0, 3, 6]
    scripts = _follow_all(oracle, base, [ops_list[k] for k in picks])[0]
    R, Cc = base[0].shape
    wrong = [("add_activity", (7.0, [0.5] * (R - 2))), ("add_activity", (7.0, [0.5] * R)),
             ("add_activity", (7.0, []))]
    b = _batch(engine, base, scripts + [wrong])
    b.Run()
    for k, script in enumerate(scripts):
        d = _handle(engine, base)
        outs = [getattr(d, op)(*args) for op, args in script]
        T, basic, sol = d.read()
        st = b.State(k)
        assert b.Outcomes(k) == outs, k
        assert st["T"].shape == T.shape and st["T"].tobytes() == T.tobytes(), k
        assert st["basic"] == basic.tolist() and st["sol"].tobytes() == sol.tobytes(), k
        assert st["z"] == d.shape()[4] and b.Log(k) == d.log(), k
        d.destroy()
    k = len(scripts)
    d = _handle(engine, base)
    T, basic, sol = d.read()
    st = b.State(k)
    assert b.Outcomes(k) == [-1, -1, -1] and b.Pivots(k) == [0, 0, 0] and b.Shape(k) == (R, Cc)
    assert st["T"].tobytes() == T.tobytes() and st["basic"] == basic.tolist()
    assert st["sol"].tobytes() == sol.tobytes() and st["z"] == d.shape()[4] and b.Log(k) == []
    d.destroy()
    b.destroy()


def test_arguments(engine, oracle):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.engine import SensState
    base, sweep = cases.rhs_sweep(oracle)
    T, x, z, _ = base
    R, Cc = T.shape
    d = SensState.create(engine, T, x, z)
    one = (C.c_int32 * 1)(1)
    pool = (C.c_double * 64)(*([0.5] * 64))
    h = C.c_void_p()

    def edits(**kw):
        return (N.SensEdit * 1)(N.SensEdit(**kw))

    def refused(base_h, count, nedits, ed, payload=pool, npayload=64):
        rc = N.lib.lpr_sens_batch_create_grow(base_h, count, nedits, ed, payload, npayload, 0,
                                              C.byref(h))
        assert rc == N.LPR_BAD_ARGUMENT, rc
        msg = N.lib.lpr_last_error().decode()
        assert "lpr_sens_batch_create_grow" in msg, msg
        return msg

    refused(None, 1, one, edits(op=0))                             # null base
    refused(d._h, 0, one, edits(op=0))                             # count 0
    refused(d._h, 1, (C.c_int32 * 1)(-1), edits(op=0))             # negative nedits
    for op in (7, 99, -1):                                         # unknown ops
        refused(d._h, 1, one, edits(op=op))
    msg = refused(d._h, 1, one, edits(op=5, a=60, b=R - 1, v=1.0))  # past npayload
    assert "scenario 0" in msg and "edit 0" in msg, msg
    refused(d._h, 1, one, edits(op=6, a=-1, b=Cc - 1, v=1.0))      # starts below 0
    refused(d._h, 1, one, edits(op=6, a=0, b=-1, v=1.0))           # negative b
    refused(d._h, 1, one, edits(op=5, a=0, b=R - 1, v=1.0), None, 64)   # null payload
    refused(d._h, 1, one, edits(op=0), pool, 2 ** 31)              # npayload above 2^31 - 1
    tall = np.zeros((1024, 1030))
    tall[1:, :1023] = np.eye(1023)
    d2 = SensState.create(engine, tall, np.zeros(6), 0.0)
    assert "1024 x 2048" in refused(d2._h, 1, one, edits(op=6, a=0, b=0, v=1.0))   # past H
    d2.destroy()
    wide = np.zeros((3, 2048))
    wide[1, 0] = wide[2, 1] = 1.0
    d3 = SensState.create(engine, wide, np.zeros(2), 0.0)
    for op in (5, 6):
        assert "1024 x 2048" in refused(d3._h, 1, one, edits(op=op, a=0, b=0, v=1.0))
    d3.destroy()
    # the old call and the old class keep refusing the add ops
    rc = N.lib.lpr_sens_batch_create(d._h, 1, one, edits(op=5), 0, C.byref(h))
    assert rc == N.LPR_BAD_ARGUMENT and "lpr_sens_add_activity" in N.lib.lpr_last_error().decode()
    with pytest.raises(ValueError):
        pkg.SensitivityBatch(d, [[("add_constraint", [1.0], 1.0)]])
    # add_constraint of the wrong width: accepted at create, -1 at run, nothing changed
    b = pkg.SensitivityGrowBatch(d, [[("add_constraint", [1.0] * (Cc - 2), 1.0),
                                      ("add_constraint", [], 1.0)], sweep[3]])
    b.Run()
    assert b.Outcomes(0) == [-1, -1] and b.Shape(0) == (R, Cc)
    assert b.Tableau(0).tobytes() == T.tobytes()
    assert b.shape_arrays()[2:] == (R + 2, Cc + 2)                 # sized for what could be
    assert N.lib.lpr_sens_batch_shape_read(b._h, None, None, None, None) == 0
    b.destroy()
    # a log smaller than the pivots is truncated; the count stays exact
    script, ref, _ = grow.follow(oracle, base, grow.mixed_shapes(oracle)[1][0])
    assert ref[2][0] >= 2
    b = pkg.SensitivityGrowBatch(d, [script], log_cap=1)
    d.destroy()                                                    # create -> destroy the base -> run
    b.Run()
    assert b.LogCap == 1 and b.LogCount(0) == sum(ref[2])
    assert b.Log(0) == ref[0].log()[:1]
    assert b.Tableau(0).tobytes() == ref[0].state()["T"].tobytes()
    b.destroy()
