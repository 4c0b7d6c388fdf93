"""GPU tests of the traced primal batch (lpr_batch_trace_*): every record the
device writes -- the tableau after every pivot, with the pivot in its header -- is the bytes of the
oracle stepped on that LP alone (oracle.find_entering / find_leaving / pivot), in every form,
through limits, resumes and the record cap, next to any neighbours; everything else a traced batch
ends with is the bytes of the untraced batch; the text is the single mirror's and the
restatement's."""
import ctypes as C

import numpy as np
import pytest

import batch_trace_cases as tc
import lp_cases
import special_values as sv

pytestmark = pytest.mark.gpu


def traced(engine, cases, trace_cap=tc.TRACE_CAP, max_pivots=tc.CAP, **kw):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    b = PrimalSimplexBatch(tc.models_of(cases), engine=engine, log_cap=tc.CAP, trace_cap=trace_cap)
    res = b.Solve(max_pivots=max_pivots, **kw)
    return b, res


def check_slab(b, refs, what="", nan_bits=True):
    """The whole slab of a traced batch against the oracle's records: exact counts, every kept
    record (header and tableau) through bytes (nan_bits False: NaN positions equal, everything
    else by bits, special_values.same), and every double no kept record covers +0.0."""
    slab, recs, off, stride = b.trace_packed()
    assert slab.size == b.TraceCap * int(stride.sum()), what
    covered = np.zeros(slab.size, dtype=bool)
    for k, ref in enumerate(refs):
        rows, cols, _ = b.Shape(k)
        assert int(stride[k]) == 2 + rows * cols, (what, k)
        assert int(recs[k]) == 1 + ref["pivots"], (what, k, int(recs[k]), ref["pivots"])
        kept = min(int(recs[k]), b.TraceCap)
        assert len(ref["records"]) >= kept, (what, k, "the reference keeps too few records")
        for i in range(kept):
            at = int(off[k] + i * stride[k])
            got = slab[at:at + int(stride[k])]
            r, e, T = ref["records"][i]
            assert got[:2].tolist() == [float(r), float(e)], (what, k, i, got[:2].tolist(), r, e)
            if nan_bits:
                assert got[2:].tobytes() == T.tobytes(), (what, k, i,
                                                          sv.first_difference(got[2:], T))
            else:
                sv.assert_same(got[2:], T.reshape(-1), (what, k, i))
            covered[at:at + int(stride[k])] = True
    assert not slab[~covered].view(np.uint64).any(), (what, "a double past the kept records")
    return slab, recs


def built_list(oracle, cases):
    return [tc.built(oracle, c) for c in cases]


def case_refs(oracle):
    return tc.refs_of(oracle, "cases", built_list(oracle, [c for _, c in tc.all_cases()]))


# ------------------------------------------------------------------- 1. one batch of every case
def test_every_case_in_one_traced_batch(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    cases = [c for _, c in tc.all_cases()]
    refs = case_refs(oracle)
    b = PrimalSimplexBatch(tc.models_of(cases), engine=engine, log_cap=tc.CAP,
                           trace_cap=tc.TRACE_CAP)
    # after the reserve: one record per LP, the built tableau under a -1, -1 header
    assert b.trace_info()[0].tolist() == [1] * b.Count
    for k, ref in enumerate(refs):
        assert b.trace_read(k, 0, 1)[0].tobytes() == tc.record_bytes(ref["records"][0]), k
    b.Solve(max_pivots=tc.CAP)
    st, piv, _ = b.status_arrays()
    assert st.tolist() == [r["status"] for r in refs]
    assert piv.tolist() == [r["pivots"] for r in refs]
    assert {tc.OPTIMAL, tc.UNBOUNDED} <= set(st.tolist())
    check_slab(b, refs, "cases")
    for k, ref in enumerate(refs):
        final = b.GetFinalTableau(k)
        assert final.tobytes() == ref["T"].tobytes(), k
        if ref["pivots"] < tc.TRACE_CAP:  # record `iterations` is the final tableau
            r, e, T = b.Snapshot(k, ref["pivots"])
            assert T.tobytes() == final.tobytes(), k
            assert (r, e) == ref["records"][-1][:2], k
        assert b.SnapshotCount(k) == 1 + ref["pivots"] + 1, k
        # the per-LP read gives what the one-copy read gives
        got = b.trace_read(k, 0, min(2, 1 + ref["pivots"]))
        for i, rec in enumerate(got):
            assert rec.tobytes() == tc.record_bytes(ref["records"][i]), (k, i)
    b.destroy()


# ------------------------------------------------------------------- 2. forced forms
def test_forced_forms_give_identical_trace_bytes(engine, oracle):
    cases = [c for _, c in tc.all_cases()]
    refs = case_refs(oracle)
    slabs = []
    for variant in (0, 1, 2, 3):
        b, _ = traced(engine, cases, variant=variant)
        slab, recs = check_slab(b, refs, variant)
        slabs.append((slab.tobytes(), recs.tobytes()))
        b.destroy()
    for s in slabs[1:]:
        assert s == slabs[0]


# ------------------------------------------------------------------- 3. threshold shapes
@pytest.mark.parametrize("m,n", tc.THRESHOLDS)
def test_threshold_shapes(engine, oracle, m, n):
    case = lp_cases.random_dense(m, n, 100 + n)
    ref = tc.refs_of(oracle, ("threshold", m, n), [tc.built(oracle, case)],
                     max_pivots=tc.SHAPE_PIVOTS, keep=tc.SHAPE_PIVOTS + 2)
    assert ref[0]["pivots"] >= 1
    want = None
    for variant in (0, 1, 2, 3):
        b, _ = traced(engine, [case], trace_cap=tc.SHAPE_PIVOTS + 2, max_pivots=tc.SHAPE_PIVOTS,
                      variant=variant)
        assert b.Status == [ref[0]["status"]]
        slab, _ = check_slab(b, ref, (m, n, variant))
        want = want or slab.tobytes()
        assert slab.tobytes() == want, (m, n, variant)
        b.destroy()


# ------------------------------------------------------------------- 4. record cap
def test_record_cap_keeps_the_prefix_and_counts_the_rest(engine, oracle):
    from lpr_381_group_v22_amd import _native as N
    cases = [lp_cases.readme_option1(), tc.cap_lp(), tc.zero_pivot_lp(), lp_cases.sample_option1()]
    refs = tc.refs_of(oracle, "cap", built_list(oracle, cases), keep=tc.SMALL_TRACE_CAP)
    assert refs[1]["pivots"] + 1 > tc.SMALL_TRACE_CAP and refs[2]["pivots"] == 0
    for variant in (0, 2, 3):
        b, _ = traced(engine, cases, trace_cap=tc.SMALL_TRACE_CAP, variant=variant)
        # exact counts, the prefix, the neighbours on both sides, +0.0 everywhere else
        check_slab(b, refs, ("cap", variant))
        assert b.SnapshotCount(1) == 1 + refs[1]["pivots"] + 1
        assert len(b.trace_read(1, 0, tc.SMALL_TRACE_CAP)) == tc.SMALL_TRACE_CAP
        assert len(b.trace_read(1, tc.SMALL_TRACE_CAP, 0)) == 0
        with pytest.raises(N.EngineError, match=r"keeps 3 \(trace_cap 3\)"):
            b.trace_read(1, tc.SMALL_TRACE_CAP - 1, 2)
        # the final entry is formatted from the batch slab, so it survives the cap
        snaps = b.IterationSnapshots(1)
        assert len(snaps) == tc.SMALL_TRACE_CAP + 1
        assert ("Final Tableau (Optimal)" in snaps[-1]) == (refs[1]["status"] == tc.OPTIMAL)
        assert b.GetFinalTableau(1).tobytes() == refs[1]["T"].tobytes()
        # the console text has no gaps: refused where records were dropped, whole elsewhere
        with pytest.raises(ValueError, match="TraceCap keeps 3"):
            b.ConsoleText(1)
        assert b.ConsoleText(2).startswith("Optimal Solution Found!")
        assert b.trace_info() is b.trace_info()  # one read per solve
        b.destroy()


# ------------------------------------------------------------------- 5. resume and chunking
def test_resume_and_chunking(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    by = dict(tc.all_cases())
    cases = [by["klee_minty_6"], by["ties_12x9_s1"], by["sample_option1"], by["zero_pivot"],
             by["unbounded_later"], by["dense_16x32_s1"]]
    refs = tc.refs_of(oracle, "resume", built_list(oracle, cases))
    most = max(r["pivots"] for r in refs)
    assert 6 <= most < tc.TRACE_CAP
    one, _ = traced(engine, cases)
    want_slab, want_recs = check_slab(one, refs, "one call")
    one.destroy()
    # chunk = 1: one pivot per LP per launch
    b, res = traced(engine, cases, chunk=1)
    assert res.launches > most
    slab, recs = check_slab(b, refs, "chunk 1")
    assert slab.tobytes() == want_slab.tobytes() and recs.tolist() == want_recs.tolist()
    b.destroy()
    # max_pivots = 1, called until nothing is left
    b = PrimalSimplexBatch(tc.models_of(cases), engine=engine, log_cap=tc.CAP,
                           trace_cap=tc.TRACE_CAP)
    calls = 0
    while any(s in (None, tc.LIMIT) for s in b.Status):
        b.Solve(max_pivots=1)
        calls += 1
        recs = b.trace_info()[0]
        for k, ref in enumerate(refs):
            assert b.Iterations[k] == min(calls, ref["pivots"]), (calls, k)
            assert int(recs[k]) == 1 + b.Iterations[k], (calls, k)
            if b.Status[k] == tc.LIMIT:  # 1 + iter records and no final entry
                assert b.SnapshotCount(k) == 1 + b.Iterations[k]
                if calls in (1, 4):
                    snaps = b.IterationSnapshots(k)
                    assert len(snaps) == 1 + b.Iterations[k]
                    assert "After pivot" in snaps[-1] and "Final" not in snaps[-1]
                    last = b.Snapshot(k, b.Iterations[k])
                    assert last[2].tobytes() == ref["records"][b.Iterations[k]][2].tobytes()
        assert calls <= most
    assert calls == most  # the pass after an LP's last pivot finds it optimal or unbounded
    slab, recs = check_slab(b, refs, "resumed")
    assert slab.tobytes() == want_slab.tobytes() and recs.tolist() == want_recs.tolist()
    b.destroy()


# ------------------------------------------------------------------- 6. untraced equality
def untraced_reads(b):
    st, it, z = b.status_arrays()
    out = [st.tobytes(), it.tobytes(), z.tobytes(), b.solution_packed().tobytes(),
           b.basis_packed().tobytes()]
    for k in range(b.Count):
        out += [b.PivotLog(k).tobytes(), b.GetFinalTableau(k).tobytes()]
    return out


def test_traced_batch_leaves_every_untraced_read_unchanged(engine):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    cases = [c for _, c in tc.all_cases()]
    u = PrimalSimplexBatch(tc.models_of(cases), engine=engine, log_cap=tc.CAP)
    ru = u.Solve(max_pivots=tc.CAP)
    t, rt = traced(engine, cases)
    assert untraced_reads(t) == untraced_reads(u)
    for f, _ in ru._fields_:
        assert getattr(rt, f) == getattr(ru, f), f
    assert t.Status == u.Status and t.FinalZ == u.FinalZ and t.SolutionVector == u.SolutionVector
    u.destroy()
    t.destroy()


def test_scenario_batch_from_a_traced_batch(engine, oracle):
    """lpr_sens_batch_from_batch reads a traced, solved batch as it reads the untraced one."""
    from lpr_381_group_v22_amd import PrimalSimplexBatch, SensitivityModelBatch
    import ref_py_ranging as ref
    import sens_model_batch_cases as mc
    models, bases, items, ops_list = mc.mixed_case(oracle)
    scripts, _, _ = mc.follow_all(oracle, bases, items, ops_list)
    reports = []
    for trace_cap in (0, 4):
        lps = PrimalSimplexBatch(models, engine=engine, trace_cap=trace_cap)
        lps.Solve()
        assert lps.TraceCap == trace_cap
        b = SensitivityModelBatch(lps, scripts, items=items)
        res = b.Run()
        rng = b.ranging_arrays()
        reports.append(dict(
            run=[getattr(res, f) for f, _ in res._fields_],
            outcomes=[a.tobytes() for a in b.outcome_arrays()],
            state=[a.tobytes() for a in b.state_arrays()],
            tableaux=[b.Tableau(k).tobytes() for k in range(b.Count)],
            solutions=[b.Solution(k).tobytes() for k in range(b.Count)],
            ranging={f: np.asarray(getattr(rng, f)) for f in ref.FIELDS}))
        b.destroy()
        lps.destroy()
    for key in ("run", "outcomes", "state", "tableaux", "solutions"):
        assert reports[0][key] == reports[1][key], key
    for f in ref.FIELDS:
        sv.assert_same(reports[0]["ranging"][f].astype(np.float64),
                       reports[1]["ranging"][f].astype(np.float64), f)


# ------------------------------------------------------------------- 7. from_tableaux
def test_from_tableaux_keeps_the_uploaded_bytes(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    T, basis = tc.negative_zero_tableau()
    T2 = tc.built(oracle, lp_cases.sample_option1())
    basis2 = np.arange(T2.shape[1] - T2.shape[0], T2.shape[1] - 1, dtype=np.int32)
    refs = tc.refs_of(oracle, "tableaux", [T2, T, T2])
    assert refs[1]["pivots"] == 1
    for variant in (1, 2, 3):
        b = PrimalSimplexBatch.from_tableaux([T2, T, T2], [basis2, basis, basis2], engine=engine,
                                             trace_cap=8)
        assert b.TraceCap == 8
        first = b.Snapshot(1, 0)
        assert first[:2] == (-1, -1) and first[2].tobytes() == T.tobytes()
        assert np.signbit(first[2][2, 1])
        b.Solve(max_pivots=tc.CAP, variant=variant)
        check_slab(b, refs, ("tableaux", variant))
        r, e, after = b.Snapshot(1, 1)
        assert (r, e) == refs[1]["records"][1][:2] == (1, 0)
        assert not np.signbit(after[2, 1]) and after[2, 1] == 0.0
        assert np.signbit(b.Snapshot(1, 0)[2][2, 1])  # record 0 keeps the uploaded sign
        b.destroy()


# ------------------------------------------------------------------- 8. non-finite data
def test_fuzz_tableaux_against_the_stepped_oracle(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    fuzz = sv.primal_fuzz()
    refs = tc.refs_of(oracle, "fuzz", [T for T, _, _ in fuzz], max_pivots=sv.FUZZ_CAP,
                      keep=sv.FUZZ_CAP + 1)
    assert any(sv.has_nan(r["T"]) for r in refs) and any(sv.has_inf(r["T"]) for r in refs)
    b = PrimalSimplexBatch.from_tableaux([T for T, _, _ in fuzz], [bs for _, bs, _ in fuzz],
                                         engine=engine, trace_cap=sv.FUZZ_CAP + 1)
    b.Solve(max_pivots=sv.FUZZ_CAP)
    assert b.status_arrays()[0].tolist() == [r["status"] for r in refs]
    check_slab(b, refs, "fuzz", nan_bits=False)
    b.destroy()


# ------------------------------------------------------------------- 9. text
def test_iteration_snapshots_console_text_and_result_file(engine, tmp_path):
    from lpr_381_group_v22_amd import PrimalSimplexSolver
    from lpr_381_group_v22_amd.program import write_full_results
    from ref_py import parse_model_text, program_option1_constraints
    from ref_py_text import PyPrimalText, mask_timestamp, py_write_full_results
    named = [("sample", lp_cases.sample_option1()), ("readme", lp_cases.readme_option1()),
             ("unbounded", lp_cases.unbounded_lp()), ("unbounded_later", tc.unbounded_later_lp()),
             ("zero_pivot", tc.zero_pivot_lp())]
    cases = [c for _, c in named]
    models = tc.models_of(cases)
    b, _ = traced(engine, cases, trace_cap=16)
    texts = []
    for k, ((name, (obj, cons, mx)), (_, pcons, _)) in enumerate(zip(named, models)):
        ref = PyPrimalText(obj, cons, mx)
        snaps, console = ref.solve_text()
        s = PrimalSimplexSolver(obj, pcons, mx, engine=engine, snapshots="all")
        s.Solve()
        got = b.IterationSnapshots(k)
        assert len(got) == len(snaps) == b.SnapshotCount(k), name
        assert got == s.IterationSnapshots, (name, "single mirror")
        assert got == snaps, (name, "restatement")
        assert b.ConsoleText(k) == console, name
        texts.append((ref, snaps))
    assert b.Status == [0, b.Status[1], 1, 1, 0] and b.Iterations[4] == 0
    assert "Unbounded Tableau" in b.IterationSnapshots(3)[-1] and b.Iterations[3] >= 1
    # the option-1 result file of the sample model, from the batch's LP
    ptype, obj, cons, signs = parse_model_text(lp_cases.SAMPLE_MODEL)
    cons1 = program_option1_constraints(len(obj), cons)
    ref, snaps = texts[0]
    want = py_write_full_results("Primal Simplex Algorithm", ptype, obj, cons1, signs, snaps,
                                 ref.FinalZ, ref.SolutionVector)
    path = str(tmp_path / "batch.txt")
    write_full_results(path, "Primal Simplex Algorithm", ptype, obj, models[0][1], signs,
                       b.IterationSnapshots(0), b.FinalZ[0], b.SolutionVector[0])
    assert mask_timestamp(open(path, "rb").read()) == want
    assert b"Iteration 6 - After pivot" in want
    b.destroy()


# ------------------------------------------------------------------- 10. arguments, lifecycle
def test_trace_arguments_and_lifecycle():
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import PrimalSimplexBatch, _native as N
    eng = pkg.Engine(0)
    L = N.lib
    i64, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    mdl = ([1.0, 1.0], [pkg.Constraint([1.0, 1.0], "<=", 1.0)], True)  # 2 x 4, one pivot

    def refused(rc_, text):
        assert rc_ == N.LPR_BAD_ARGUMENT
        assert text in L.lpr_last_error().decode(), L.lpr_last_error().decode()

    out = np.zeros(64)
    three = [np.zeros(1, dtype=np.int64) for _ in range(3)]
    # an untraced handle: every trace call is refused, and it still solves; then too late
    u = PrimalSimplexBatch([mdl], engine=eng)
    refused(L.lpr_batch_trace_info(u._h, *[p(a, i64) for a in three]), "not traced")
    refused(L.lpr_batch_trace_read(u._h, 0, 0, 0, p(out, dp)), "not traced")
    refused(L.lpr_batch_trace_read_all(u._h, p(out, dp), 64), "not traced")
    for cap in (0, -1):
        refused(L.lpr_batch_trace_reserve(u._h, cap), f"trace_cap {cap} < 1")
    u.Solve()
    assert u.Status == [0] and u.Iterations == [1]
    refused(L.lpr_batch_trace_reserve(u._h, 2), "only before the handle's first")
    with pytest.raises(N.EngineError, match="not traced"):
        u.IterationSnapshots(0)
    u.Solve()
    assert u.Status == [0]
    u.destroy()

    t = PrimalSimplexBatch([mdl], engine=eng, trace_cap=2)
    refused(L.lpr_batch_trace_reserve(t._h, 2), "already traced (trace_cap 2)")
    t.Solve()
    assert t.Status == [0] and t.SnapshotCount(0) == 3  # start, one pivot, the final block
    stride = 2 + 2 * 4
    assert [a.tolist() for a in t.trace_info()] == [[2], [0], [stride]]
    for k in (-1, 1):
        refused(L.lpr_batch_trace_read(t._h, k, 0, 1, p(out, dp)), f"LP {k} out of range (0..0)")
    refused(L.lpr_batch_trace_read(t._h, 0, 0, 3, p(out, dp)), "keeps 2")
    refused(L.lpr_batch_trace_read(t._h, 0, 2, 1, p(out, dp)), "keeps 2")
    refused(L.lpr_batch_trace_read(t._h, 0, -1, 1, p(out, dp)), "keeps 2")
    refused(L.lpr_batch_trace_read(t._h, 0, 0, 1, None), "null output")
    refused(L.lpr_batch_trace_read_all(t._h, p(out, dp), 2 * stride - 1), "cap_doubles 19")
    refused(L.lpr_batch_trace_read_all(t._h, None, 64), "null output")
    assert L.lpr_batch_trace_read_all(t._h, p(out, dp), 2 * stride) == 0
    assert out[:2].tolist() == [-1.0, -1.0] and out[stride:stride + 2].tolist() == [1.0, 0.0]
    assert not out[2 * stride:].any()
    assert L.lpr_batch_trace_info(t._h, None, None, None) == 0
    t.Solve()  # the handle still solves (nothing is left to do) and keeps its records
    assert t.Status == [0] and t.trace_info()[0].tolist() == [2]

    eng.close()  # the handle is orphaned: every call but destroy is refused
    refused(L.lpr_batch_trace_reserve(t._h, 2), "orphaned")
    refused(L.lpr_batch_trace_info(t._h, None, None, None), "orphaned")
    refused(L.lpr_batch_trace_read(t._h, 0, 0, 1, p(out, dp)), "orphaned")
    refused(L.lpr_batch_trace_read_all(t._h, p(out, dp), 64), "orphaned")
    t.destroy()
