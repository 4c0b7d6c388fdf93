"""GPU tests of the traced revised-simplex batch (lpr_rev_batch_trace_*):
every record the device writes -- one per pivot and the "Optimal" one -- is the bytes of the
oracle's CaptureSnapshot numbers (oracle.revised_trace) for that LP alone, in every form, through
limits, resumes and the record cap, next to any neighbours; everything else a traced batch ends
with is the bytes of the untraced batch; the text is the single mirror's."""
import ctypes as C

import numpy as np
import pytest

import lp_cases
import revised_batch_cases as rc
import special_values as sv
from test_oracle_revised import flat

pytestmark = pytest.mark.gpu

FLOAT_KEYS = ("rc_pre", "z_working", "z_original", "y", "rcX", "rcS", "u_pre", "ratios_pre", "xB",
              "BInvA", "BInv")
INT_KEYS = ("entering", "leaving_row", "leaving_var")
BASIS_KEYS = ("basis_pre", "basis_post")

_TRACES = {}


def traces_of(oracle, key, models, max_iter=rc.CAP, cap=300):
    """The oracle's traces of a model list, computed once per key and left unchanged."""
    if key not in _TRACES:
        out = []
        for obj, cons, is_min in models:
            A, b = flat(cons)
            out.append(oracle.revised_trace(obj, A, b, is_min, max_iter=max_iter, cap=cap))
        _TRACES[key] = out
    return _TRACES[key]


def all_cases():
    return rc.models() + rc.degenerate_models()


def check_record(got, want, what, nan_bits=True):
    """One record against the oracle's snapshot, field by field, through bytes (nan_bits False:
    the NaN exception of DESIGN.md section 2, sv.assert_same)."""
    for key in INT_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in BASIS_KEYS:
        assert got[key].tolist() == want[key].tolist(), (what, key)
    for key in FLOAT_KEYS:
        g = np.asarray(got[key], dtype=np.float64)
        w = np.asarray(want[key], dtype=np.float64)
        assert g.shape == w.shape, (what, key)
        if nan_bits:
            assert g.tobytes() == w.tobytes(), (what, key, g.tolist(), w.tolist())
        else:
            sv.assert_same(g, w, (what, key))


def check_traces(b, traces, what="", upto=None, nan_bits=True):
    """Every kept record of every LP of a traced batch against the oracle's; the counts are exact."""
    from lpr_381_group_v22_amd.revised_batch import trace_record
    slab, snaps, off, stride = b.trace_packed()
    for k, tr in enumerate(traces):
        n, m = b.Shape(k)
        count = tr["count"] if upto is None else upto[k]
        assert int(snaps[k]) == count, (what, k, int(snaps[k]), count)
        for i in range(min(count, b.TraceCap, len(tr["snapshots"]))):
            at = int(off[k] + i * stride[k])
            check_record(trace_record(slab[at:at + int(stride[k])], m, n), tr["snapshots"][i],
                         (what, k, i), nan_bits)


def traced(engine, models, variant=0, cap=rc.CAP, trace_cap=300, **kw):
    from lpr_381_group_v22_amd import RevisedSimplexBatch
    b = RevisedSimplexBatch(models, engine=engine, log_cap=rc.CAP, trace_cap=trace_cap)
    res = b.Solve(max_pivots=cap, variant=variant, **kw)
    return b, res


def reads(b):
    """Everything the reads of an untraced batch give, as bytes."""
    st, it, z = b.status_arrays()
    out = [st.tobytes(), it.tobytes(), z.tobytes(), b.solution_packed().tobytes(),
           b.basis_packed().tobytes()]
    for k in range(b.Count):
        out += [b.PivotLog(k).tobytes(), b.BInverse(k).tobytes(), b.XB(k).tobytes()]
    return out


# --------------------------------------------------------------------- 1. one batch of every case
def test_every_case_in_one_traced_batch(engine, oracle):
    names = [n for n, _ in all_cases()]
    models = [m for _, m in all_cases()]
    traces = traces_of(oracle, "cases", models)
    counts = dict(zip(names, (t["count"] for t in traces)))
    assert counts["sample_option2"] == 7 and counts["klee_minty_8"] == 256
    assert counts["unbounded"] == 0 and counts["infeasible_basis"] == 0
    assert counts["zero_objective"] == 1 and counts["zero_A"] == 0 and counts["m1_n12"] == 3
    b, _ = traced(engine, models)
    st, it, _ = b.status_arrays()
    assert st.tolist() == [t["status"] for t in traces]
    assert it.tolist() == [t["iterations"] for t in traces]
    check_traces(b, traces)
    for k in range(b.Count):
        assert b.SnapshotCount(k) == traces[k]["count"], names[k]
    # the per-LP reads give what the one-copy read gives
    k = names.index("sample_option2")
    for i in range(7):
        check_record(b.Snapshot(k, i), traces[k]["snapshots"][i], ("Snapshot", i))
    b.destroy()


# --------------------------------------------------------------------- 2. forced forms
def test_forced_forms_give_identical_trace_bytes(engine, oracle):
    models = [m for _, m in all_cases()]
    traces = traces_of(oracle, "cases", models)
    b, _ = traced(engine, models, 0)
    want = b.trace_packed()[0].tobytes()
    b.destroy()
    for variant in (1, 2, 3):
        b, _ = traced(engine, models, variant)
        check_traces(b, traces, variant)
        slab, snaps, _, _ = b.trace_packed()
        assert slab.tobytes() == want, variant
        assert snaps.tolist() == [t["count"] for t in traces], variant
        b.destroy()


# --------------------------------------------------------------------- 3. infeasible after a pivot
def test_infeasible_after_a_pivot_keeps_complete_records(engine, oracle):
    from lpr_381_group_v22_amd import revised_batch as rb
    models = [rc.duplicated_rows(12, 5, 6, 21), rc.duplicated_rows(20, 6, 10, 16),
              rc.duplicated_rows(70, 12, 10, 2)]
    traces = traces_of(oracle, "infeasible_later", models)
    assert [rb.pick_form(len(m[1]), len(m[0])) for m in models] == [0, 0, 1]
    assert [(t["status"], t["count"]) for t in traces] == [(2, 1), (2, 2), (2, 1)]
    for variant in (0, 3):
        b, res = traced(engine, models, variant, trace_cap=4)
        assert res.infeasible == 3
        assert b.status_arrays()[0].tolist() == [2, 2, 2]
        check_traces(b, traces, variant)
        b.destroy()


# --------------------------------------------------------------------- 4. unbounded after pivots
def unbounded_later(seed):
    rng = np.random.RandomState(seed)
    A = np.round(rng.uniform(-2, 3, (3, 4)), 1)
    b = np.round(rng.uniform(1, 9, 3), 1)
    c = np.round(rng.uniform(0.5, 5, 4), 1)
    return rc.to_model(c, A, b)


def test_unbounded_after_pivots_writes_no_record_for_the_failing_pass(engine, oracle):
    models = [unbounded_later(seed) for seed in (10, 15, 24)]
    traces = traces_of(oracle, "unbounded_later", models)
    assert [(t["status"], t["count"]) for t in traces] == [(1, 3), (1, 2), (1, 2)]
    for variant in (0, 2, 3):
        b, res = traced(engine, models, variant, trace_cap=6)
        assert res.unbounded == 3
        check_traces(b, traces, variant)
        b.destroy()


# --------------------------------------------------------------------- 5. limits, resume, chunks
@pytest.mark.parametrize("chunk", [3, 1])
def test_limits_resume_and_chunks(engine, oracle, chunk):
    from lpr_381_group_v22_amd import RevisedSimplexBatch
    by = dict(rc.models())
    models = [by["klee_minty_8"], by["ties_24x30_s2"], by["ties_33x20_s3"], by["sample_option2"]]
    traces = traces_of(oracle, "limits", models)
    obj, cons, is_min = models[0]
    A, bb = flat(cons)
    at7 = oracle.revised_trace(obj, A, bb, is_min, max_iter=7, cap=16)
    assert (at7["status"], at7["count"]) == (5, 7)
    b = RevisedSimplexBatch(models, engine=engine, log_cap=rc.CAP, trace_cap=300)
    calls = 0
    while any(s in (None, 5) for s in b.Status):
        b.Solve(max_pivots=7, chunk=chunk)
        calls += 1
        st, it, _ = b.status_arrays()
        upto = [int(it[k]) + (1 if st[k] == 0 else 0) for k in range(b.Count)]
        assert [b.SnapshotCount(k) for k in range(b.Count)] == upto, calls
        check_traces(b, traces, ("call", calls), upto=upto)
        if calls == 1:
            assert (int(st[0]), upto[0]) == (5, 7)
            for i in range(7):
                check_record(b.Snapshot(0, i), at7["snapshots"][i], ("max_iter 7", i))
        assert calls < 60
    assert calls > 30
    check_traces(b, traces, "resumed")
    b.destroy()


# --------------------------------------------------------------------- 6. record cap
def test_record_cap_keeps_the_prefix_and_counts_the_rest(engine, oracle):
    from lpr_381_group_v22_amd import _native as N
    by = dict(rc.models())
    tr = traces_of(oracle, "cases", [m for _, m in all_cases()])[
        [n for n, _ in all_cases()].index("klee_minty_8")]
    b, _ = traced(engine, [by["klee_minty_8"]], trace_cap=5)
    assert b.SnapshotCount(0) == 256 and b.Status == [0]
    check_traces(b, [tr], "cap 5")
    assert len(b.trace_read(0, 0, 5)) == 5 and len(b.trace_read(0, 5, 0)) == 0
    assert len(b.IterationSnapshots(0)) == 5
    with pytest.raises(N.EngineError, match=r"keeps 5 \(trace_cap 5\)"):
        b.trace_read(0, 4, 2)
    b.destroy()


# --------------------------------------------------------------------- 7. untraced equality
def test_traced_batch_leaves_every_untraced_read_unchanged(engine):
    from lpr_381_group_v22_amd import RevisedSimplexBatch
    models = [m for _, m in all_cases()]
    u = RevisedSimplexBatch(models, engine=engine, log_cap=rc.CAP)
    ru = u.Solve(max_pivots=rc.CAP)
    t, rt = traced(engine, models)
    assert reads(t) == reads(u)
    for f, _ in ru._fields_:
        assert getattr(rt, f) == getattr(ru, f), f
    u.destroy()
    t.destroy()


# --------------------------------------------------------------------- 8. mixed forms
def test_mixed_forms_shuffled_neighbours(engine, oracle):
    from lpr_381_group_v22_amd import revised_batch as rb
    models = rc.mixed_models()
    order = np.random.RandomState(0).permutation(len(models)).tolist()
    assert order != sorted(order)
    models = [models[k] for k in order]
    forms = [rb.pick_form(len(m[1]), len(m[0])) for m in models]
    assert sorted(set(forms)) == [0, 1, 2]
    traces = traces_of(oracle, "mixed_shuffled", models, cap=4)
    b, _ = traced(engine, models, trace_cap=4)
    _, snaps, off, stride = b.trace_packed()
    assert stride.tolist() == [rb.trace_stride(len(m[1]), len(m[0])) for m in models]
    assert len(set(stride.tolist())) > 3
    assert off.tolist() == [0] + np.cumsum(4 * stride)[:-1].tolist()
    assert any(int(s) > 4 for s in snaps)
    check_traces(b, traces, "mixed")
    b.destroy()


def test_forms_g_and_h_above_64_kib(engine, oracle):
    """One LP each at the smallest shapes that take more than the 64 KiB of dynamic LDS a kernel
    gets without the attribute: 61 x 64 in form G (66 304 bytes; 61 x 63 takes 65 312) and
    64 x 1578 in form H (vectors and tile: 65 552 bytes; 64 x 1577 takes 65 536).  Three passes,
    every record against the oracle's; the untraced batch gives the same reads."""
    from lpr_381_group_v22_amd import RevisedSimplexBatch, revised_batch as rb
    def h_bytes(m, n):
        return 8 * (rb.footprint(m, n) - m * (m | 1) - m * (n | 1) + 256 * 17)
    assert 8 * rb.footprint(61, 63) <= 64 * 1024 < 8 * rb.footprint(61, 64) <= rb.MAX_LDS_G
    assert h_bytes(64, 1577) <= 64 * 1024 < h_bytes(64, 1578)
    for (m, n), form in (((61, 64), rb.FORM_G), ((64, 1578), rb.FORM_H)):
        assert rb.pick_form(m, n) == form
        models = [lp_cases.random_dense(m, n, 17)[:2] + (False,)]
        traces = traces_of(oracle, ("above 64 KiB", form), models, max_iter=3, cap=5)
        assert (traces[0]["status"], traces[0]["iterations"], traces[0]["count"]) == (5, 3, 3)
        b, res = traced(engine, models, cap=3, trace_cap=5)
        assert res.limit == 1
        check_traces(b, traces, ("above 64 KiB", form))
        u = RevisedSimplexBatch(models, engine=engine, log_cap=rc.CAP)
        u.Solve(max_pivots=3)
        assert reads(u) == reads(b), form
        b.destroy()
        u.destroy()


# --------------------------------------------------------------------- 9. special values, division
def test_special_values_against_the_oracle_trace(engine, oracle):
    cases = sv.revised_cases()
    models = [rc.to_model(c, A, b) for _, c, A, b in cases]
    traces = [oracle.revised_trace(c, A, b, False, max_iter=sv.REVISED_CAP,
                                   cap=sv.REVISED_CAP + 2) for _, c, A, b in cases]
    b, _ = traced(engine, models, cap=sv.REVISED_CAP, trace_cap=sv.REVISED_CAP + 2)
    assert b.status_arrays()[0].tolist() == [t["status"] for t in traces]
    check_traces(b, traces, "special", nan_bits=False)
    b.destroy()


def test_negative_zero_of_A_prints_as_positive_zero_and_ieee_division(engine, oracle):
    neg = rc.to_model([0.0, 0.0], [[-0.0, 1.0], [2.0, -0.0]], [1.0, 1.0])
    div = rc.ieee_div_model()
    traces = traces_of(oracle, "negzero_ieee", [neg, div])
    assert (traces[0]["status"], traces[0]["count"]) == (0, 1)
    for variant in (1, 2, 3):
        b, _ = traced(engine, [neg, div], variant, trace_cap=3)
        check_traces(b, traces, variant)
        opt = b.Snapshot(0, 0)
        assert opt["entering"] == -1 and opt["BInv"].tolist() == [[1.0, 0.0], [0.0, 1.0]]
        assert not np.signbit(opt["BInvA"]).any()  # 0.0 + 1.0 * -0.0 is +0.0
        assert opt["BInvA"].tolist() == [[0.0, 1.0], [2.0, 0.0]]
        first = b.Snapshot(1, 0)
        assert float(first["BInv"][1][0]).hex() == "-0x1.6666666666667p-2"
        b.destroy()


# --------------------------------------------------------------------- 10. text
def test_iteration_snapshots_text(engine, tmp_path):
    from lpr_381_group_v22_amd import (Constraint, RevisedPrimalSimplexSolver,
                                       RevisedSimplexBatch, SolverException)
    from lpr_381_group_v22_amd.program import write_full_results
    from ref_py import PyRevised, parse_model_text, py_snapshot_text
    from ref_py_text import mask_timestamp
    import lp_cases
    cases = rc.models()[:9]
    models = [(obj, [Constraint(list(c.Coefficients), c.Relation, c.RHS) for c in cons], mn)
              for _, (obj, cons, mn) in cases]
    b = RevisedSimplexBatch(models, engine=engine, trace_cap=64)
    b.Solve(max_pivots=60)
    singles = []
    for k, ((name, (obj, cons, mn)), (_, pcons, _)) in enumerate(zip(cases, models)):
        s = RevisedPrimalSimplexSolver(obj, pcons, mn, engine=engine, snapshots="all")
        try:
            s.Solve(max_pivots=60)
        except SolverException:
            pass
        singles.append(s)
        p = PyRevised(obj, cons, mn)
        p.solve(max_iter=60, capture=True)
        want = [py_snapshot_text(q, len(obj), len(cons), mn) for q in p.snapshots]
        got = b.IterationSnapshots(k)
        assert len(got) == len(want) == len(s.IterationSnapshots) > 0, name
        for i, g in enumerate(got):
            assert g == s.IterationSnapshots[i], (name, i, "single mirror")
            assert g == want[i], (name, i, "restatement")
    # the option-2 result file of the sample model, from the batch's LP
    assert cases[0][0] == "sample_option2"
    ptype, _, _, signs = parse_model_text(lp_cases.SAMPLE_MODEL)
    obj, cons, _ = models[0]
    files = []
    for tag, snaps, z, x in (("batch", b.IterationSnapshots(0), b.FinalZ[0], b.SolutionVector[0]),
                             ("single", singles[0].IterationSnapshots, singles[0].FinalZ,
                              singles[0].SolutionVector)):
        path = str(tmp_path / (tag + ".txt"))
        write_full_results(path, "Revised Primal Simplex Algorithm (T-*)", ptype, obj, cons, signs,
                           snaps, z, x)
        files.append(mask_timestamp(open(path, "rb").read()))
    assert files[0] == files[1] and b"--- Iteration 7 ---" in files[0]
    b.destroy()


# --------------------------------------------------------------------- 11. arguments, lifecycle
def test_trace_arguments_and_lifecycle():
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import RevisedSimplexBatch, _native as N
    eng = pkg.Engine(0)
    L = N.lib
    i64, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    mdl = rc.to_model([1.0, 1.0], [[1.0, 1.0]], [1.0])

    def refused(rc_, text):
        assert rc_ == N.LPR_BAD_ARGUMENT
        assert text in L.lpr_last_error().decode(), L.lpr_last_error().decode()

    out = np.zeros(64)
    three = [np.zeros(1, dtype=np.int64) for _ in range(3)]
    # an untraced handle: every trace read is refused, then too late to reserve
    u = RevisedSimplexBatch([mdl], engine=eng)
    refused(L.lpr_rev_batch_trace_info(u._h, *[p(a, i64) for a in three]), "not traced")
    refused(L.lpr_rev_batch_trace_read(u._h, 0, 0, 0, p(out, dp)), "not traced")
    refused(L.lpr_rev_batch_trace_read_all(u._h, p(out, dp), 64), "not traced")
    for cap in (0, -2):
        refused(L.lpr_rev_batch_trace_reserve(u._h, cap), f"trace_cap {cap} < 1")
    u.Solve()
    refused(L.lpr_rev_batch_trace_reserve(u._h, 2), "only before the handle's first")
    with pytest.raises(N.EngineError, match="not traced"):
        u.IterationSnapshots(0)
    u.destroy()

    t = RevisedSimplexBatch([mdl], engine=eng, trace_cap=2)
    refused(L.lpr_rev_batch_trace_reserve(t._h, 2), "already traced (trace_cap 2)")
    t.Solve()
    assert t.Status == [0] and t.SnapshotCount(0) == 2  # one pivot and "Optimal"
    stride = 6 + 7 + 2 + 2 + 1
    assert [a.tolist() for a in t.trace_info()] == [[2], [0], [stride]]
    for k in (-1, 1):
        refused(L.lpr_rev_batch_trace_read(t._h, k, 0, 1, p(out, dp)),
                f"LP {k} out of range (0..0)")
    refused(L.lpr_rev_batch_trace_read(t._h, 0, 0, 3, p(out, dp)), "keeps 2")
    refused(L.lpr_rev_batch_trace_read(t._h, 0, -1, 1, p(out, dp)), "keeps 2")
    refused(L.lpr_rev_batch_trace_read(t._h, 0, 0, 1, None), "null output")
    refused(L.lpr_rev_batch_trace_read_all(t._h, p(out, dp), 2 * stride - 1), "cap_doubles 35")
    refused(L.lpr_rev_batch_trace_read_all(t._h, None, 64), "null output")
    assert L.lpr_rev_batch_trace_read_all(t._h, p(out, dp), 2 * stride) == 0
    assert out[0] == 0.0 and out[stride] == -1.0 and not out[2 * stride:].any()
    assert L.lpr_rev_batch_trace_info(t._h, None, None, None) == 0

    eng.close()  # the handle is orphaned: every call but destroy is refused
    refused(L.lpr_rev_batch_trace_reserve(t._h, 2), "orphaned")
    refused(L.lpr_rev_batch_trace_info(t._h, None, None, None), "orphaned")
    refused(L.lpr_rev_batch_trace_read(t._h, 0, 0, 1, p(out, dp)), "orphaned")
    refused(L.lpr_rev_batch_trace_read_all(t._h, p(out, dp), 64), "orphaned")
    t.destroy()
