"""GPU tests of the batched revised simplex (lpr_rev_batch_*): every LP of a
batch ends with the bytes the oracle (oracle.revised_solve) gives for it alone -- status,
iterations, log, basis, B^-1, the last x_B, and x / Z on the optimal exit -- in every form,
through limits and resumes, next to any neighbours."""
import ctypes as C

import numpy as np
import pytest

import revised_batch_cases as rc
import special_values as sv

pytestmark = pytest.mark.gpu

_REFS = {}


def refs_of(oracle, key, models, cap=rc.CAP):
    """The oracle's solves of a model list, computed once per key and left unchanged."""
    if key not in _REFS:
        _REFS[key] = [rc.oracle_ref(oracle, mdl, cap) for mdl in models]
    return _REFS[key]


def snapshot(b):
    """Everything the batch reads give, as bytes."""
    st, it, z = b.status_arrays()
    out = [st.tobytes(), it.tobytes(), z.tobytes(), b.solution_packed().tobytes(),
           b.basis_packed().tobytes()]
    for k in range(b.Count):
        out += [b.PivotLog(k).tobytes(), b.BInverse(k).tobytes(), b.XB(k).tobytes()]
    return out


def check_lp(b, k, ref, what=""):
    st, it, z = b.status_arrays()
    assert (int(st[k]), int(it[k])) == (ref["status"], ref["iterations"]), (what, k)
    cap = b._log_caps[k]
    assert b.PivotLog(k).tolist() == ref["log"][:cap].tolist(), (what, k)
    assert b.BasicVariables(k) == ref["basis"].tolist(), (what, k)
    assert b.BInverse(k).tobytes() == ref["Binv"].tobytes(), (what, k)
    assert b.XB(k).tobytes() == ref["xB"].tobytes(), (what, k)
    n = b.Shape(k)[0]
    x = b.solution_packed()[int(b._x_at[k]):int(b._x_at[k]) + n]
    if ref["status"] == 0:
        assert x.tobytes() == ref["x"].tobytes(), (what, k)
        assert np.float64(z[k]).tobytes() == np.float64(ref["z"]).tobytes(), (what, k)
    else:
        assert not x.any() and z[k] == 0.0, (what, k)


def check_batch(b, refs, what=""):
    for k, ref in enumerate(refs):
        check_lp(b, k, ref, what)


def solved(engine, models, variant=0, cap=rc.CAP, **kw):
    from lpr_381_group_v22_amd import RevisedSimplexBatch
    b = RevisedSimplexBatch(models, engine=engine, log_cap=kw.pop("log_cap", rc.CAP))
    res = b.Solve(max_pivots=cap, variant=variant, **kw)
    return b, res


def expected_launches(forms, iters, chunk):
    """The running-list rule: per form, the most passes an LP of it needs
    in the call, P // chunk + 1 (the pass that ends the LP is one of them); every round launches
    each form that still has an LP once."""
    return sum(max(p // chunk + 1 for ff, p in zip(forms, iters) if ff == f) for f in set(forms))


# --------------------------------------------------------------------- 1. the oracle's cases
def test_all_revised_cases_in_one_batch(engine, oracle):
    names = [n for n, _ in rc.models()]
    models = [m for _, m in rc.models()]
    refs = refs_of(oracle, "cases", models)
    assert len(models) == 13
    by = dict(zip(names, refs))
    assert by["sample_option2"]["iterations"] == 6 and by["klee_minty_8"]["iterations"] == 255
    assert (by["unbounded"]["status"], by["unbounded"]["iterations"]) == (1, 0)
    assert (by["infeasible_basis"]["status"], by["infeasible_basis"]["iterations"]) == (2, 0)
    b, res = solved(engine, models)
    check_batch(b, refs)
    assert res.iterations == sum(r["iterations"] for r in refs)
    assert (res.optimal, res.unbounded, res.infeasible, res.other, res.limit) == (11, 1, 1, 0, 0)
    b.destroy()


# --------------------------------------------------------------------- 2. forced forms
def test_forced_forms_give_identical_bytes(engine, oracle):
    models = [m for _, m in rc.models()]
    refs = refs_of(oracle, "cases", models)
    snaps = []
    for variant in (0, 1, 2, 3):
        b, _ = solved(engine, models, variant)
        check_batch(b, refs, variant)
        snaps.append(snapshot(b))
        b.destroy()
    assert snaps[1] == snaps[0] and snaps[2] == snaps[0] and snaps[3] == snaps[0]


# --------------------------------------------------------------------- 3. thresholds
def test_threshold_shapes(engine, oracle):
    from lpr_381_group_v22_amd import revised_batch as rb
    shapes = rc.threshold_shapes()
    assert [f for _, _, _, f in shapes] == [rb.FORM_W, rb.FORM_G, rb.FORM_G,
                                            rb.FORM_G, rb.FORM_H, rb.FORM_H]
    models = [m for _, m in rc.threshold_models()]
    refs = refs_of(oracle, "thresholds", models)
    assert all(r["status"] == 0 and r["iterations"] > 0 for r in refs)
    b, res = solved(engine, models)
    check_batch(b, refs)
    # one form per side of each boundary: every form launched at least once
    assert res.launches >= 3
    b.destroy()


# --------------------------------------------------------------------- 4. the H limit
def test_h_limit_shape_and_refusals(engine, oracle):
    from lpr_381_group_v22_amd import RevisedSimplexBatch, _native as N
    c, A, bb = oracle.gen_dense_lp(1023, 1024, 0)
    ref = oracle.revised_solve(c, A, bb, False, max_iter=4)
    assert (ref["status"], ref["iterations"]) == (5, 4)
    b, res = solved(engine, [rc.to_model(c, A, bb)], cap=4)
    check_lp(b, 0, ref)
    assert res.limit == 1
    b.destroy()
    for m, n in ((1024, 4), (1000, 1048)):
        assert m > 1023 or n + m == 2048
        with pytest.raises(N.EngineError, match="lpr_revised_solve"):
            RevisedSimplexBatch([rc.to_model(np.ones(n), np.ones((m, n)), np.ones(m))],
                                engine=engine)


# --------------------------------------------------------------------- 5. degenerate shapes
def test_degenerate_shapes(engine, oracle):
    models = [m for _, m in rc.degenerate_models()]
    refs = refs_of(oracle, "degenerate", models)
    by = dict(zip([n for n, _ in rc.degenerate_models()], refs))
    assert (by["zero_objective"]["status"], by["zero_objective"]["iterations"]) == (0, 0)
    assert (by["zero_A"]["status"], by["zero_A"]["iterations"]) == (1, 0)
    b, _ = solved(engine, models)
    check_batch(b, refs)
    b.destroy()
    for k, mdl in enumerate(models):  # count = 1
        b, _ = solved(engine, [mdl])
        check_lp(b, 0, refs[k], "alone")
        b.destroy()


# --------------------------------------------------------------------- 6. mixed and shuffled
def test_mixed_forms_and_shuffle(engine, oracle):
    from lpr_381_group_v22_amd import revised_batch as rb
    models = rc.mixed_models()
    refs = refs_of(oracle, "mixed", models)
    forms = [rb.pick_form(len(m[1]), len(m[0])) for m in models]
    assert sorted(set(forms)) == [0, 1, 2] and forms[:3] == [0, 1, 2]
    b, _ = solved(engine, models)
    check_batch(b, refs)
    b.destroy()
    order = np.random.RandomState(0).permutation(len(models)).tolist()
    assert order != sorted(order)
    b, _ = solved(engine, [models[k] for k in order])
    check_batch(b, [refs[k] for k in order], "shuffled")
    b.destroy()


# --------------------------------------------------------------------- 7. limits and launches
def test_limits_resume_chunks_and_launch_counts(engine, oracle):
    from lpr_381_group_v22_amd import RevisedSimplexBatch, revised_batch as rb
    by = dict(rc.models())
    models = [by["klee_minty_8"], by["ties_24x30_s2"], by["ties_33x20_s3"], by["sample_option2"]]
    refs = refs_of(oracle, "limits", models)
    total = [r["iterations"] for r in refs]
    forms = [rb.pick_form(len(m[1]), len(m[0])) for m in models]
    b = RevisedSimplexBatch(models, engine=engine, log_cap=rc.CAP)
    left = list(total)
    for call in range(max(total) // 7 + 2):
        alive = [k for k in range(len(models)) if b.Status[k] in (None, 5)]
        if not alive:
            break
        step = [min(7, left[k]) for k in alive]
        res = b.Solve(max_pivots=7, chunk=3)
        _, it, _ = b.status_arrays()
        for k, d in zip(alive, step):
            left[k] -= d
            assert it[k] == total[k] - left[k], (call, k)
        assert res.iterations == sum(step)
        assert res.launches == expected_launches([forms[k] for k in alive], step, 3), call
    assert left == [0] * len(models) and call > 30
    check_batch(b, refs, "resumed")
    again = b.Solve(max_pivots=7, chunk=3)  # finished LPs stay finished
    assert again.iterations == 0 and again.launches == 0
    check_batch(b, refs, "again")
    b.destroy()


# --------------------------------------------------------------------- 8. short log
def test_log_cap_keeps_the_prefix(engine, oracle):
    by = dict(rc.models())
    ref = refs_of(oracle, "klee", [by["klee_minty_8"]])[0]
    b, _ = solved(engine, [by["klee_minty_8"]], log_cap=5)
    assert b.PivotLog(0).tolist() == ref["log"][:5].tolist() and len(b.PivotLog(0)) == 5
    assert b.Iterations[0] == 255
    check_lp(b, 0, ref)
    b.destroy()


# --------------------------------------------------------------------- 9. the tie clause
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_ratio_tie_clause(engine, oracle, variant):
    models = rc.tie_models()
    refs = refs_of(oracle, "ties", models)
    assert len(models) == 256 and all(r["status"] == 0 for r in refs)
    b, res = solved(engine, models, variant)
    assert res.optimal == 256
    check_batch(b, refs, variant)
    b.destroy()


# --------------------------------------------------------------------- 10. infeasible later
def test_basis_turns_infeasible_after_a_pivot(engine, oracle):
    models = [rc.duplicated_rows(70, 12, 10, 2), rc.duplicated_rows(130, 9, 13, 4)]
    refs = refs_of(oracle, "dup", models)
    assert (refs[0]["status"], refs[0]["iterations"]) == (2, 1)
    assert (refs[1]["status"], refs[1]["iterations"]) == (0, 11)
    assert rc.tie_stats(models[1])[3] == 1
    for variant in (0, 3):
        b, res = solved(engine, models, variant)
        check_batch(b, refs, variant)
        assert (res.infeasible, res.optimal) == (1, 1)
        b.destroy()


# --------------------------------------------------------------------- 11. IEEE division
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_ieee_division(engine, oracle, variant):
    mdl = rc.ieee_div_model()
    ref = refs_of(oracle, "ieee", [mdl])[0]
    assert float(ref["Binv"][1][0]).hex() == "-0x1.6666666666667p-2"
    assert float(ref["Binv"][0][0]).hex() == "0x1.0000000000003p-2"
    b, _ = solved(engine, [mdl], variant)
    assert b.PivotLog(0).tolist() == [[0, 0, 1]]
    Binv = b.BInverse(0)
    assert float(Binv[1][0]).hex() == "-0x1.6666666666667p-2"
    assert float(Binv[0][0]).hex() == "0x1.0000000000003p-2"
    check_lp(b, 0, ref)
    b.destroy()


# --------------------------------------------------------------------- 12. zero skip and -0
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_zero_skip_and_negative_zero(engine, oracle, variant):
    models = rc.zero_skip_models()
    refs = refs_of(oracle, "zero_skip", models, 500)
    b, _ = solved(engine, models, variant, cap=500)
    check_batch(b, refs, variant)
    b.destroy()


# --------------------------------------------------------------------- 13. special values
def test_special_values(engine, oracle):
    cases = sv.revised_cases()
    models = [rc.to_model(c, A, b) for _, c, A, b in cases]
    refs = [oracle.revised_solve(c, A, b, False, max_iter=sv.REVISED_CAP) for _, c, A, b in cases]
    bt, _ = solved(engine, models, cap=sv.REVISED_CAP)
    st, it, z = bt.status_arrays()
    x = bt.solution_packed()
    for k, (ref, (name, _, _, _)) in enumerate(zip(refs, cases)):
        assert (int(st[k]), int(it[k])) == (ref["status"], ref["iterations"]), name
        assert bt.PivotLog(k).tolist() == ref["log"].tolist(), name
        assert bt.BasicVariables(k) == ref["basis"].tolist(), name
        sv.assert_same(bt.BInverse(k), ref["Binv"], (name, "Binv"))
        sv.assert_same(bt.XB(k), ref["xB"], (name, "xB"))
        if ref["status"] == 0:
            sv.assert_same(x[int(bt._x_at[k]):int(bt._x_at[k + 1])], ref["x"], (name, "x"))
            sv.assert_same(z[k], ref["z"], (name, "z"))
    bt.destroy()


# --------------------------------------------------------------------- 14. the mirror
def test_mirror_against_the_single_model_mirror(engine):
    from lpr_381_group_v22_amd import (Constraint, RevisedPrimalSimplexSolver,
                                       RevisedSimplexBatch, SolverException)
    models = [(obj, [Constraint(list(c.Coefficients), c.Relation, c.RHS) for c in cons], mn)
              for _, (obj, cons, mn) in rc.models()]
    b = RevisedSimplexBatch(models, engine=engine, log_cap=rc.CAP)
    b.Solve(max_pivots=rc.CAP)
    raised = 0
    for k, (obj, cons, mn) in enumerate(models):
        s = RevisedPrimalSimplexSolver(obj, cons, mn, engine=engine, snapshots="none")
        err = None
        try:
            s.Solve(max_pivots=rc.CAP)
        except SolverException as ex:
            err = ex
        assert b.Status[k] == s.Status, k
        assert np.float64(b.FinalZ[k]).tobytes() == np.float64(s.FinalZ).tobytes(), k
        assert b.SolutionVector[k] == s.SolutionVector, k
        assert b.BasicVariables(k) == s.BasicVariables, k
        assert b.PivotLog(k).tolist() == s.PivotLog.tolist(), k
        if err is None:
            b.Raise(k)
        else:
            raised += 1
            with pytest.raises(SolverException) as got:
                b.Raise(k)
            assert str(got.value) == str(err) and got.value.status == err.status
    assert raised == 2
    b.destroy()


# --------------------------------------------------------------------- 15. arguments, lifecycle
def test_bad_arguments_and_lifecycle(oracle):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import RevisedSimplexBatch, _native as N
    eng = pkg.Engine(0)
    L = N.lib
    n = np.array([2], dtype=np.int32)
    m = np.array([1], dtype=np.int32)
    obj, A, b = np.ones(2), np.ones(2), np.ones(1)
    mn = np.zeros(1, dtype=np.int8)
    i32, dp, i8 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int8)
    p = lambda a, t: a.ctypes.data_as(t)
    h = C.c_void_p()

    def create(count=1, n_=n, m_=m, obj_=obj, A_=A, b_=b, mn_=mn, log_cap=0):
        args = [None if a is None else p(a, t) for a, t in
                ((n_, i32), (m_, i32), (obj_, dp), (A_, dp), (b_, dp), (mn_, i8))]
        return L.lpr_rev_batch_create(eng._h, count, *args, log_cap, C.byref(h))

    def refused(rc_, text):
        assert rc_ == N.LPR_BAD_ARGUMENT
        assert text in L.lpr_last_error().decode(), L.lpr_last_error().decode()

    refused(create(count=0), "count=0")
    refused(create(count=-3), "count=-3")
    for hole in ("n_", "m_", "obj_", "A_", "b_", "mn_"):
        refused(create(**{hole: None}), "null")
    refused(create(log_cap=-1), "log_cap=-1")
    refused(create(n_=np.array([0], dtype=np.int32)), "LP 0 has n=0 m=1")
    refused(create(m_=np.array([0], dtype=np.int32)), "LP 0 has n=2 m=0")
    refused(create(m_=np.array([1024], dtype=np.int32)), "lpr_revised_solve")
    refused(create(n_=np.array([2047], dtype=np.int32)), "n + m <= 2047")

    bt = RevisedSimplexBatch([rc.to_model([1.0, 1.0], [[1.0, 1.0]], [1.0])], engine=eng)
    res = N.RevBatchResult()
    for variant, chunk in ((4, 0), (-1, 0), (0, -1)):
        opts = N.RevBatchOpts(max_pivots=0, chunk=chunk, variant=variant)
        refused(L.lpr_rev_batch_solve(bt._h, C.byref(opts), C.byref(res)),
                f"variant {variant} (0 auto, 1 W, 2 G, 3 H) / chunk {chunk}")
    refused(L.lpr_rev_batch_solve(bt._h, None, None), "null result")
    out = np.zeros(4)
    cnt = C.c_int64()
    for k in (-1, 1):
        refused(L.lpr_rev_batch_binv_read(bt._h, k, p(out, dp)), f"LP {k} out of range (0..0)")
        refused(L.lpr_rev_batch_xb_read(bt._h, k, p(out, dp)), f"LP {k} out of range (0..0)")
        refused(L.lpr_rev_batch_shape(bt._h, k, None, None), f"LP {k} out of range (0..0)")
        refused(L.lpr_rev_batch_log_read(bt._h, k, None, None, None, 4, C.byref(cnt)),
                f"LP {k} out of range (0..0)")
    refused(L.lpr_rev_batch_log_read(bt._h, 0, None, None, None, -1, C.byref(cnt)), "cap -1")
    refused(L.lpr_rev_batch_solution_read(bt._h, None), "null x")
    refused(L.lpr_rev_batch_basis_read(bt._h, None), "null basis")
    refused(L.lpr_rev_batch_binv_read(bt._h, 0, None), "null output")
    bt.Solve()
    assert bt.Status == [0] and bt.Shape(0) == (2, 1)
    nn, mm = C.c_int32(), C.c_int32()
    assert L.lpr_rev_batch_shape(bt._h, 0, C.byref(nn), C.byref(mm)) == 0
    assert (nn.value, mm.value) == (2, 1)

    eng.close()  # the handle is orphaned: every call but destroy is refused
    refused(L.lpr_rev_batch_solve(bt._h, None, C.byref(res)), "orphaned")
    refused(L.lpr_rev_batch_status_read(bt._h, None, None, None), "orphaned")
    refused(L.lpr_rev_batch_shape(bt._h, 0, None, None), "orphaned")
    bt.destroy()
    bt.destroy()  # harmless
