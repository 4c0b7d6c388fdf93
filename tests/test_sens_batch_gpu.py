"""GPU parity tests of the sensitivity scenario batch (lpr_sens_batch_*)
against the C oracle (oracle/oracle_sens.c): every scenario of every batch is compared with the
oracle run on that script alone -- outcome and pivots per edit, pivot log, tableau bytes,
basicVars, z, and the solution bytes and length."""
import ctypes as C

import numpy as np
import pytest

import sens_batch_cases as cases
import sens_cases

pytestmark = pytest.mark.gpu

FORM_G, FORM_H = 1, 2
VARIANT_G, VARIANT_H = 2, 3


def _batch(engine, base, scripts, **kw):
    """A batch over a fresh handle holding `base`; the handle is destroyed before the batch
    runs."""
    from lpr_381_group_v22_amd import SensitivityBatch
    from lpr_381_group_v22_amd.engine import SensState
    T, x, z, _ = base
    d = SensState.create(engine, T, x, z)
    b = SensitivityBatch(d, scripts, **kw)
    d.destroy()
    return b


def _check_all(batch, refs, name):
    for k, ref in enumerate(refs):
        cases.same_scenario(batch, k, ref, (name, k))


def _run_and_check(engine, oracle, name, base, scripts, form=None, **run_kw):
    refs = [cases.oracle_run(oracle, base, s) for s in scripts]
    b = _batch(engine, base, scripts)
    res = b.Run(**run_kw)
    assert res.finished == len(scripts) and res.running == 0, name
    if form is not None:
        assert res.form == form, (name, res.form)
    assert res.pivots == sum(sum(r[2]) for r in refs), name
    _check_all(b, refs, name)
    b.destroy()
    return refs


@pytest.fixture(scope="module")
def sweep(oracle):
    base, scripts = cases.rhs_sweep(oracle)
    return base, scripts, [cases.oracle_run(oracle, base, s) for s in scripts]


def test_all_edits_all_outcomes(engine, oracle):
    seen = set()
    for name, base, scripts in cases.all_edit_cases(oracle):
        for ref in _run_and_check(engine, oracle, name, base, scripts, form=FORM_G):
            seen |= set(ref[1])
    assert {0, 1, 2, 8, -1} <= seen, seen


def test_rhs_sweep_with_real_pivots(engine, sweep):
    base, scripts, refs = sweep
    b = _batch(engine, base, scripts)
    res = b.Run()
    assert res.finished == 32 and res.running == 0
    _check_all(b, refs, "sweep")
    oc, pv = b.outcome_arrays()
    assert int(pv.sum()) == res.pivots == 59 and int(pv.sum()) > 0
    assert (oc == 0).sum() == 23 and (oc == 8).sum() == 9
    b.destroy()


def test_largest_g_shape_and_one_column_past_it(engine, oracle):
    ne = cases.largest_g_extra(60)
    base, scripts = cases.threshold_case(60, ne, 41)
    _run_and_check(engine, oracle, "largest G", base, scripts, form=FORM_G)
    base, scripts = cases.threshold_case(60, ne + 1, 41)
    _run_and_check(engine, oracle, "first H", base, scripts, form=FORM_H)


@pytest.mark.parametrize("mode", sorted(sens_cases.TIE_MODES))
def test_h_tie_plants_cross_lane_strides(engine, oracle, mode):
    """Form H with the EPS-band plants of sens_cases two or more lane strides (64, 256) apart:
    the leaving rows on a 521 x 1081 base, the dual entering columns and the primal arg-min on
    81 x 861 bases.  The planted candidate decides the log entry the case names."""
    for name, (base, ops, expect) in [
            ("leave_rows", sens_cases.leaving_rows_script(mode, gap=300, m=520, n_extra=40)),
            ("enter_cols", sens_cases.entering_cols_script(mode, 80, 700, 300)),
            ("argmin_cols", sens_cases.argmin_cols_script(mode, 80, 700, 300))]:
        R, Cc = base[0].shape
        assert R <= 1024 and Cc <= 2048
        script = cases.keep_shape(ops)
        refs = _run_and_check(engine, oracle, (name, mode), base, [script, script[:1]],
                              form=FORM_H)
        o, outs, pivs, _ = refs[0]
        assert outs == [0] * len(script), (name, mode, outs)
        log, start = o.log(), np.concatenate([[0], np.cumsum(pivs)])
        for (op_idx, k, field, value) in expect:
            assert log[start[op_idx] + k][field] == value, (name, mode, op_idx, k, field)
    assert base[0].shape[0] <= 1024


def test_forced_forms_give_identical_bytes(engine, oracle, sweep):
    base, scripts, refs = sweep
    g = _batch(engine, base, scripts)
    h = _batch(engine, base, scripts)
    assert g.Run(variant=VARIANT_G).form == FORM_G
    assert h.Run(variant=VARIANT_H).form == FORM_H
    _check_all(g, refs, "forced G")
    _check_all(h, refs, "forced H")
    for k in range(len(scripts)):
        assert g.Tableau(k).tobytes() == h.Tableau(k).tobytes()
        assert g.Solution(k).tobytes() == h.Solution(k).tobytes()
        assert g.Log(k) == h.Log(k)
    assert [a.tobytes() for a in g.state_arrays()] == [a.tobytes() for a in h.state_arrays()]
    assert [a.tobytes() for a in g.outcome_arrays()] == [a.tobytes() for a in h.outcome_arrays()]
    g.destroy()
    h.destroy()


@pytest.mark.parametrize("variant", [VARIANT_G, VARIANT_H])
def test_resumption_one_pivot_per_call(engine, sweep, variant):
    """chunk = 1 and max_pivots = 1 per call until nothing is running: the bytes of one default
    call, on the rolled-back scenarios too (their stop falls inside ChangeRHS's dual phase)."""
    base, scripts, refs = sweep
    b = _batch(engine, base, scripts)
    calls, pivots = 0, 0
    for _ in range(200):
        res = b.Run(max_pivots=1, chunk=1, variant=variant)
        calls += 1
        pivots += res.pivots
        assert res.finished + res.running == 32
        if res.running == 0:
            break
    assert res.running == 0 and res.finished == 32
    assert pivots == 59 and calls > 2
    rolled = [k for k, r in enumerate(refs) if r[1] == [8] and r[2][0] > 0]
    assert rolled, "no rolled-back scenario with pivots: the stop never falls inside the dual"
    _check_all(b, refs, ("resumed", variant))
    b.destroy()


def pivot_attempts(ref):
    """The pivots a script asks for, in order: 'p' for one that is made, 'f' for one that fails
    (no entering column, no leaving row, a zero pivot: the edit ends with an outcome other than 0,
    which ChangeRHS reports as rolled back).  An edit that is refused (-1) asks for none."""
    _, outs, pivs, _ = ref
    return "".join("p" * n + ("f" if o not in (0, -1) else "") for o, n in zip(outs, pivs))


def expected_launches(seqs, chunk, max_pivots=0):
    """(launches of one Run call, where each scenario stands after it), from where the scenarios
    stand in their pivot_attempts (None: not in this call).

    A launch goes on until a scenario's script has ended or the scenario asks for a pivot after
    it has made `chunk` of them in this launch; a pivot that fails is asked for like any other but
    is not counted.  So a scenario that makes P pivots in a call takes max(1, ceil(P / chunk))
    launches, and one more when P is a multiple of chunk, not 0, and a failing pivot follows the
    last one made.  The pivot limit of the call is looked at after the chunk, in front of every
    pivot asked for: the scenario leaves the call there.  The call takes the maximum over its
    scenarios (one form, so one launch per round)."""
    most, after = 0, []
    for seq, pos in seqs:
        if pos is None:
            after.append(None)
            continue
        launches, done, made = 1, 0, 0
        while pos < len(seq):
            if done >= chunk:
                launches, done = launches + 1, 0
            if max_pivots > 0 and made >= max_pivots:
                break
            if seq[pos] == "p":
                done, made = done + 1, made + 1
            pos += 1
        most = max(most, launches)
        after.append(pos if pos < len(seq) else None)
    return most, after


def test_exact_launch_counts(engine, sweep):
    base, scripts, refs = sweep
    seqs = [pivot_attempts(r) for r in refs]
    assert any(q.endswith("pf") for q in seqs) and any(q.endswith("p") for q in seqs)
    assert sum(q.count("p") for q in seqs) == 59 and "" in seqs
    for chunk in (1, 3):
        b = _batch(engine, base, scripts)
        res = b.Run(chunk=chunk, variant=VARIANT_G)
        want, _ = expected_launches([(q, 0) for q in seqs], chunk)
        print("chunk", chunk, "launches", res.launches, "expected", want)
        assert res.finished == 32 and res.pivots == 59
        _check_all(b, refs, ("launch counts", chunk))
        assert res.launches == want, (chunk, res.launches, want)
        b.destroy()
    # calls of at most two pivots each, every call resuming the scenarios stopped at the limit
    b = _batch(engine, base, scripts)
    at = [(q, 0) for q in seqs]
    for call in range(2):
        want, after = expected_launches(at, 1, max_pivots=2)
        res = b.Run(max_pivots=2, chunk=1, variant=VARIANT_G)
        print("call", call, "launches", res.launches, "expected", want)
        assert res.running == sum(a is not None for a in after)
        assert res.launches == want, (call, res.launches, want)
        at = [(q, a) for q, a in zip(seqs, after)]
    assert res.running > 0  # the second call resumed scenarios and stopped some again
    b.Run()
    _check_all(b, refs, "launch counts, resumed")
    b.destroy()


def test_form_g_above_64_kib_twice(engine, oracle):
    """A 64 x 129 base (68 360 bytes of dynamic LDS in form G, above the 64 KiB a kernel gets
    without the attribute) with a three-edit script, twice: the second batch finds the attribute
    set."""
    from lpr_381_group_v22_amd.sens_batch import footprint_g
    base, scripts = cases.threshold_case(63, 2, 43)
    assert base[0].shape == (64, 129) and 64 * 1024 < footprint_g(64, 129) <= 159 * 1024
    for run in range(2):
        _run_and_check(engine, oracle, ("G above 64 KiB", run), base, [scripts[0][:3]],
                       form=FORM_G, variant=VARIANT_G)


def test_stale_base(engine, oracle):
    """The base is a handle on which a change_rhs with a pivot has run, so its basicVars were last
    written by that pivot, not by a rebuild: it stores column 9 for row 3 where a rebuild would
    take column 7, and holds a -1 for row 5.  Scenarios that start with change_nonbasic_cbar,
    change_basic or change_nonbasic_column on those columns must read the stored list: their
    outcomes differ from what a rebuilt base gives.  The oracle is brought to the same state by
    the same call."""
    from lpr_381_group_v22_amd import SensitivityBatch
    from lpr_381_group_v22_amd.engine import SensState
    base, prefix, scripts = cases.stale_base()
    stored, rebuilt, differ = cases.stale_differs(oracle, base, prefix, scripts)
    assert stored != rebuilt and -1 in stored, (stored, rebuilt)
    firsts = {scripts[q][0][0] for q in differ}
    assert {"change_nonbasic_cbar", "change_basic"} <= firsts, firsts
    T, x, z, _ = base
    d = SensState.create(engine, T, x, z)
    for op, args in prefix:
        assert getattr(d, op)(*args) == 0
    assert d.shape()[5] > 0                      # the prefix pivoted
    assert d.read(tableau=False)[1].tolist() == stored
    for variant in (VARIANT_G, VARIANT_H):
        b = SensitivityBatch(d, scripts)
        b.Run(variant=variant)
        for q, s in enumerate(scripts):
            ref = cases.oracle_run(oracle, base, s, prefix=prefix)
            cases.same_scenario(b, q, ref, ("stale", variant, q))
        for q in differ:                          # not what a rebuilt base would report
            fresh = cases.oracle_run(oracle, base, scripts[q],
                                     prefix=list(prefix) + [("resolve_all", ())])
            assert b.Outcomes(q)[0] != fresh[1][0], (variant, q)
        b.destroy()
    d.destroy()


def test_isolation(engine, oracle, sweep):
    from lpr_381_group_v22_amd import SensitivityBatch
    from lpr_381_group_v22_amd.engine import SensState
    base, scripts, refs = sweep
    T, x, z, _ = base
    d = SensState.create(engine, T, x, z)
    assert d.change_rhs(1, float(T[1, -1]) * 0.5) in (0, 8)   # the base has a log of its own
    T0, basic0, sol0 = d.read()
    z0, log0 = d.shape()[4], d.log()
    twice = [scripts[3], [], scripts[3], scripts[7]]
    b = SensitivityBatch(d, twice)
    b.Run()
    T1, basic1, sol1 = d.read()
    assert T1.tobytes() == T0.tobytes() and basic1.tolist() == basic0.tolist()
    assert sol1.tobytes() == sol0.tobytes() and d.shape()[4] == z0 and d.log() == log0
    # the same script twice: the same bytes
    s0, s2 = b.State(0), b.State(2)
    assert s0["T"].tobytes() == s2["T"].tobytes() and s0["basic"] == s2["basic"]
    assert s0["sol"].tobytes() == s2["sol"].tobytes() and s0["z"] == s2["z"]
    assert b.Log(0) == b.Log(2) and b.Outcomes(0) == b.Outcomes(2)
    # no edits: the base state
    s1 = b.State(1)
    assert s1["T"].tobytes() == T0.tobytes() and s1["basic"] == basic0.tolist()
    assert s1["sol"].tobytes() == sol0.tobytes() and s1["z"] == z0
    assert b.Log(1) == [] and b.Outcomes(1) == []
    b.destroy()
    # the base may go before the run (_batch destroys it)
    b2 = _batch(engine, base, scripts[:4])
    b2.Run()
    _check_all(b2, refs[:4], "base destroyed")
    b2.destroy()
    d.destroy()


def test_arguments(engine, oracle, sweep):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.engine import SensState
    base, scripts, refs = sweep
    T, x, z, _ = base
    d = SensState.create(engine, T, x, z)
    one = (C.c_int32 * 1)(1)
    edit = (N.SensEdit * 1)(N.SensEdit(op=0))
    h = C.c_void_p()

    def refused(base_h, count, nedits, edits):
        rc = N.lib.lpr_sens_batch_create(base_h, count, nedits, edits, 0, C.byref(h))
        assert rc == N.LPR_BAD_ARGUMENT, rc
        msg = N.lib.lpr_last_error().decode()
        assert "lpr_sens_batch_create" in msg, msg
        return msg

    refused(None, 1, one, edit)                                   # null base
    refused(d._h, 0, one, edit)                                   # count 0
    refused(d._h, 1, (C.c_int32 * 1)(-1), edit)                   # negative nedits
    for op in (5, 6, 99, -1):                                     # add ops and unknown ops
        msg = refused(d._h, 1, one, (N.SensEdit * 1)(N.SensEdit(op=op)))
        assert "lpr_sens_add_activity" in msg
    eng2 = pkg.Engine(0)
    d2 = SensState.create(eng2, T, x, z)
    eng2.close()
    refused(d2._h, 1, one, edit)                                  # orphaned base
    d2.destroy()
    wide = np.zeros((3, 2050))
    wide[1, 0] = wide[2, 1] = 1.0
    d3 = SensState.create(engine, wide, np.zeros(2), 0.0)
    assert "1024 x 2048" in refused(d3._h, 1, one, edit)          # beyond form H
    d3.destroy()
    with pytest.raises(ValueError):
        pkg.SensitivityBatch(d, [[("add_constraint", [1.0], 1.0)]])
    # a log smaller than the pivots is truncated; the count stays exact
    k = max(range(32), key=lambda q: refs[q][2][0])
    assert refs[k][2][0] >= 2
    b = pkg.SensitivityBatch(d, [scripts[k]], log_cap=1)
    b.Run()
    assert b.LogCap == 1 and b.LogCount(0) == refs[k][2][0]
    assert b.Log(0) == refs[k][0].log()[:1]
    assert b.Tableau(0).tobytes() == refs[k][0].state()["T"].tobytes()
    b.destroy()
    d.destroy()
