"""GPU tests of the batched primal simplex (lpr_batch_*): every LP of a batch
against the CPU oracle run on that LP alone -- built tableau, status, pivot count, pivot log, basis,
final tableau, Z and x, all as bits -- across the three forms, their thresholds, resumed and
chunked solves, short logs, and the bad-argument paths."""
import ctypes as C

import numpy as np
import pytest

import lp_cases
from ref_py import PyConstraint

pytestmark = pytest.mark.gpu

CAP = 5000  # tie-heavy LPs can cycle: every solve is capped, here and in the oracle


def oracle_from_model(oracle, obj, cons, is_max, max_pivots=CAP, log_cap=1 << 16):
    o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
    T, basis = oracle.primal_build(o, A, rel, rhs, is_max, ncoef)
    return oracle_from_tableau(oracle, T, basis, len(obj), max_pivots, log_cap)


def oracle_from_tableau(oracle, T, basis, n, max_pivots=CAP, log_cap=1 << 16):
    T = np.ascontiguousarray(T, dtype=np.float64).copy()
    T0 = T.copy()
    basis = np.ascontiguousarray(basis, dtype=np.int32).copy()
    st, piv, log = oracle.primal_solve(T, basis, max_pivots, log_cap)
    x, z = oracle.extract_solution(T, n)
    return dict(T0=T0, T=T, basis=basis, status=st, pivots=piv, log=log, x=x, z=z)


def assert_lp_equal(batch, k, ref, x_packed=None, z_all=None, st_all=None, piv_all=None):
    assert batch.GetFinalTableau(k).tobytes() == ref["T"].tobytes(), f"LP {k}: final tableau"
    assert batch.BasicVariables(k) == [int(v) for v in ref["basis"]], f"LP {k}: basis"
    log = batch.PivotLog(k)
    assert np.array_equal(log, ref["log"][: len(log)]), f"LP {k}: pivot log"
    if st_all is not None:
        assert st_all[k] == ref["status"], (k, st_all[k], ref["status"])
        assert piv_all[k] == ref["pivots"], (k, piv_all[k], ref["pivots"])
        assert np.float64(z_all[k]).tobytes() == np.float64(ref["z"]).tobytes(), f"LP {k}: z"


def check_batch(batch, refs, exact_log=True):
    st, piv, z = batch.status_arrays()
    x = batch.solution_packed()
    at = 0
    for k, ref in enumerate(refs):
        assert_lp_equal(batch, k, ref, z_all=z, st_all=st, piv_all=piv)
        if exact_log:
            assert len(batch.PivotLog(k)) == min(ref["pivots"], len(ref["log"]))
        n = batch.Shape(k)[2]
        if ref["status"] == 0:
            assert x[at:at + n].tobytes() == ref["x"].tobytes(), f"LP {k}: x"
        else:
            assert not np.any(x[at:at + n]), f"LP {k}: x of a non-optimal LP is 0"
        at += n


def models_of(cases):
    from lpr_381_group_v22_amd import Constraint
    return [(obj, [Constraint(list(c.Coefficients), c.Relation, c.RHS) for c in cons], mx)
            for obj, cons, mx in cases]


# ------------------------------------------------------------------------------ 1. all cases
def test_all_cases_in_one_batch(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch, Tableau
    cases = [c for _, c in lp_cases.all_cases()]
    b = PrimalSimplexBatch(models_of(cases), engine=engine, log_cap=CAP)
    refs = []
    for k, (obj, cons, mx) in enumerate(cases):
        o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
        single = Tableau.from_lp(engine, o, A, rel, rhs, is_max=mx, ncoef=ncoef)
        assert b.GetFinalTableau(k).tobytes() == single.read().tobytes(), f"LP {k}: built bytes"
        single.destroy()
        ref = oracle_from_model(oracle, obj, cons, mx)
        assert b.GetFinalTableau(k).tobytes() == ref["T0"].tobytes()
        refs.append(ref)
    res = b.Solve(max_pivots=CAP)
    assert res.launches >= 1 and res.pivots == sum(r["pivots"] for r in refs)
    statuses = {r["status"] for r in refs}
    assert 0 in statuses and 1 in statuses  # optimal and unbounded both covered
    check_batch(b, refs)


# ------------------------------------------------------------------------------ 2. forms
def test_forced_forms_give_identical_bytes(engine):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    models = models_of([c for _, c in lp_cases.all_cases()])
    snaps = []
    for variant in (0, 1, 2, 3):
        b = PrimalSimplexBatch(models, engine=engine, log_cap=CAP)
        b.Solve(max_pivots=CAP, variant=variant)
        snaps.append(([b.GetFinalTableau(k).tobytes() for k in range(b.Count)],
                      [b.PivotLog(k).tobytes() for k in range(b.Count)],
                      b.basis_packed().tobytes(), [s.tobytes() for s in b.status_arrays()],
                      b.solution_packed().tobytes()))
        b.destroy()
    for s in snaps[1:]:
        assert s == snaps[0]


def _dense_model(m, n, seed):
    obj, cons, mx = lp_cases.random_dense(m, n, seed)
    return obj, cons, mx


# (m, n) at each threshold and one column past it: W holds rows * (cols + 1) <= 2016 doubles,
# G <= 20352, H rows <= 1024 and cols <= 2048
THRESHOLDS = [(31, 30), (31, 31), (63, 253), (63, 254)]


@pytest.mark.parametrize("m,n", THRESHOLDS)
def test_threshold_shapes(engine, oracle, m, n):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    R, Cc = m + 1, n + m + 1
    assert R * (Cc + 1) in (2016, 2048, 20352, 20416)
    obj, cons, mx = _dense_model(m, n, 100 + n)
    ref = oracle_from_model(oracle, obj, cons, mx)
    for variant in (0, 1, 2, 3):
        b = PrimalSimplexBatch(models_of([(obj, cons, mx)]), engine=engine, log_cap=CAP)
        b.Solve(max_pivots=CAP, variant=variant)
        check_batch(b, [ref])
        b.destroy()


def test_form_h_limit_shape(engine, oracle):
    """The largest shape form H takes (1024 x 2048), capped at 16 pivots (then the limit)."""
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    obj, cons, mx = _dense_model(1023, 1024, 7)
    ref = oracle_from_model(oracle, obj, cons, mx, max_pivots=16)
    b = PrimalSimplexBatch(models_of([(obj, cons, mx)]), engine=engine)
    b.Solve(max_pivots=16)
    assert ref["status"] == 5 and ref["pivots"] == 16
    check_batch(b, [ref], exact_log=False)


def test_degenerate_shapes(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    models = [([1.0, 2.0, 3.0], [], True),                            # m = 0: unbounded at once
              ([-1.0, -2.0], [], True),                              # m = 0: optimal at once
              ([], [PyConstraint([], "<=", 4.0), PyConstraint([], ">=", 2.0)], True),  # n = 0
              ([2.0], [PyConstraint([1.0], "<=", 3.0)], False)]      # min
    refs = [oracle_from_model(oracle, *mdl) for mdl in models]
    b = PrimalSimplexBatch(models_of(models), engine=engine)
    b.Solve(max_pivots=CAP)
    check_batch(b, refs)
    # cols = 2 (one column besides the RHS), from ready tableaux
    rng = np.random.RandomState(3)
    tabs = [np.array([[-1.0, 0.0], [2.0, 4.0], [0.5, 3.0]]),
            np.array([[1.0, 5.0]]), rng.rand(5, 2) - 0.5]
    bases = [[7, 8], [], [0, 0, 0, 0]]
    b = PrimalSimplexBatch.from_tableaux(tabs, bases, engine=engine)
    b.Solve(max_pivots=CAP)
    refs = [oracle_from_tableau(oracle, t, np.asarray(bs, dtype=np.int32),
                                max(0, t.shape[1] - t.shape[0])) for t, bs in zip(tabs, bases)]
    check_batch(b, refs)


# ------------------------------------------------------------------------------ 3. mixed batch
def _mixed_models(count, seed):
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        m = int(rng.randint(0, 97))
        n = int(rng.randint(1, 161))
        if rng.rand() < 0.5:
            out.append(lp_cases.random_dense(m, n, 1000 + k))
        else:
            out.append(lp_cases.tie_heavy(m, n, 1000 + k))
    return out


def test_mixed_batch_and_shuffle(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    cases = _mixed_models(3000, 11)
    refs = [oracle_from_model(oracle, *c) for c in cases]
    b = PrimalSimplexBatch(models_of(cases), engine=engine, log_cap=64)
    res = b.Solve(max_pivots=CAP)
    assert res.optimal + res.unbounded + res.limit == len(cases)
    check_batch(b, refs, exact_log=False)
    perm = np.random.RandomState(5).permutation(len(cases))
    b2 = PrimalSimplexBatch(models_of([cases[i] for i in perm]), engine=engine, log_cap=64)
    b2.Solve(max_pivots=CAP)
    for k2, k in enumerate(perm):
        assert b2.GetFinalTableau(k2).tobytes() == b.GetFinalTableau(int(k)).tobytes()
        assert b2.PivotLog(k2).tobytes() == b.PivotLog(int(k)).tobytes()


# ------------------------------------------------------------------------------ 4. caps
def _cap_models():
    cases = dict(lp_cases.all_cases())
    return [cases["klee_minty_10"], cases["dense_16x32_s1"], cases["ties_24x30_s2"],
            cases["unbounded"], cases["dense_64x128_s3"]]


def test_max_pivots_resume_and_chunk(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    models = models_of(_cap_models())
    full = PrimalSimplexBatch(models, engine=engine, log_cap=CAP)
    rf = full.Solve(max_pivots=CAP)
    assert rf.launches >= 1
    want = [full.GetFinalTableau(k).tobytes() for k in range(full.Count)]
    want_log = [full.PivotLog(k).tobytes() for k in range(full.Count)]
    piv_full = full.status_arrays()[1]
    for step in (1, 7):
        b = PrimalSimplexBatch(models, engine=engine, log_cap=CAP)
        r = b.Solve(max_pivots=step)
        st, piv, _ = b.status_arrays()
        for k in range(b.Count):
            if piv_full[k] > step:
                assert st[k] == 5 and piv[k] == step, (k, st[k], piv[k])
        assert r.limit >= 1
        for _ in range(int(max(piv_full)) // step + 2):
            if b.Solve(max_pivots=step).limit == 0:
                break
        assert [b.GetFinalTableau(k).tobytes() for k in range(b.Count)] == want
        assert [b.PivotLog(k).tobytes() for k in range(b.Count)] == want_log
        assert np.array_equal(b.status_arrays()[1], piv_full)
        again = b.Solve(max_pivots=step)  # finished LPs stay finished
        assert again.pivots == 0 and again.launches == 0
    b = PrimalSimplexBatch(models, engine=engine, log_cap=CAP)
    r = b.Solve(max_pivots=CAP, chunk=1)
    assert r.launches >= int(max(piv_full))  # a relaunch after every pivot
    assert [b.GetFinalTableau(k).tobytes() for k in range(b.Count)] == want
    assert [b.PivotLog(k).tobytes() for k in range(b.Count)] == want_log


def _mixed_form_models():
    """LPs of all three forms: W (m 3-6, n 3-8), G (m = 32, n = 64: rows * (cols + 1) = 3234
    doubles) and H (m = 100, n = 120: 22 422 > 20 352), tie-heavy and dense."""
    return [lp_cases.tie_heavy(4, 6, 1), lp_cases.random_dense(5, 8, 2), lp_cases.tie_heavy(6, 3, 3),
            lp_cases.random_dense(32, 64, 5), lp_cases.tie_heavy(32, 64, 6),
            lp_cases.random_dense(100, 120, 7)]


def _form_of(ref):
    R, Cc = ref["T"].shape
    doubles = R * (Cc + 1)
    return 0 if doubles <= 2016 else (1 if doubles <= 20352 else 2)


def expected_launches(forms, pivots, chunk):
    """Launches of one Solve call: the sum over the forms of max over the form's LPs of
    P // chunk + 1, P the pivots the LP makes in the call.  A launch runs at most `chunk`
    iterations of the Solve() loop per LP, the iteration that ends the LP -- it finds no entering
    column or no leaving row, or meets max_pivots in front of a pivot -- is one of them, so an LP
    needs P + 1 iterations; every round launches each form that still has an LP once."""
    total = 0
    for f in set(forms):
        total += max(p // chunk + 1 for ff, p in zip(forms, pivots) if ff == f)
    return total


def test_exact_launch_counts_through_mixed_forms(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    cases = _mixed_form_models()
    refs = [oracle_from_model(oracle, *c) for c in cases]
    forms = [_form_of(r) for r in refs]
    P = [r["pivots"] for r in refs]
    assert forms == [0, 0, 0, 1, 1, 2] and max(P) < CAP and all(r["status"] == 0 for r in refs)
    for chunk in (1, 3):
        b = PrimalSimplexBatch(models_of(cases), engine=engine, log_cap=CAP)
        res = b.Solve(max_pivots=CAP, chunk=chunk)
        print("chunk", chunk, "launches", res.launches, "pivots", res.pivots)
        check_batch(b, refs)
        assert res.pivots == sum(P)
        assert res.launches == expected_launches(forms, P, chunk), (chunk, res.launches)
        b.destroy()
    # two calls of at most two pivots each, the second resuming the LPs stopped at the limit
    b = PrimalSimplexBatch(models_of(cases), engine=engine, log_cap=CAP)
    left = list(P)
    for call in range(2):
        alive = [k for k in range(len(P)) if call == 0 or P[k] > 2 * call]
        step = [min(left[k], 2) for k in alive]
        res = b.Solve(max_pivots=2, chunk=1)
        print("call", call, "launches", res.launches, "pivots", res.pivots)
        assert res.pivots == sum(step)
        assert res.launches == expected_launches([forms[k] for k in alive], step, 1), call
        for k, d in zip(alive, step):
            left[k] -= d
    check_batch(b, [oracle_from_model(oracle, *c, max_pivots=4) for c in cases])
    b.destroy()


# ------------------------------------------------------------------------------ 5. short log
def test_log_cap_keeps_the_prefix(engine, oracle):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    cases = _cap_models()
    b = PrimalSimplexBatch(models_of(cases), engine=engine, log_cap=3)
    b.Solve(max_pivots=CAP)
    piv = b.status_arrays()[1]
    for k, c in enumerate(cases):
        ref = oracle_from_model(oracle, *c)
        log = b.PivotLog(k)
        assert len(log) == min(piv[k], 3) and piv[k] == ref["pivots"]
        assert np.array_equal(log, ref["log"][:3][: len(log)])


# ------------------------------------------------------------------------------ 6. -0.0
def test_zero_factor_meets_negative_zero(engine, oracle):
    """Row 2 has factor +0 and a -0.0 under the pivot row's -2: the C# writes -0.0 - (+0 * -2) =
    +0.0 there; a kernel that skipped zero-factor rows would leave -0.0."""
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    T = np.array([[-1.0, 0.0, 0.0, 0.0],
                  [2.0, -4.0, 1.0, 6.0],
                  [0.0, -0.0, 0.0, 5.0]])
    basis = np.array([2, 3], dtype=np.int32)
    ref = oracle_from_tableau(oracle, T, basis, 1)
    assert np.signbit(T[2, 1]) and not np.signbit(ref["T"][2, 1])
    for variant in (1, 2, 3):
        b = PrimalSimplexBatch.from_tableaux([T], [basis], engine=engine)
        b.Solve(max_pivots=CAP, variant=variant)
        check_batch(b, [ref])
        assert not np.signbit(b.GetFinalTableau(0)[2, 1])


# ------------------------------------------------------------------------------ 7. the mirror
def test_batch_mirror_equals_single_solver(engine, tmp_path):
    from lpr_381_group_v22_amd import InputFileParser, PrimalSimplexBatch, PrimalSimplexSolver
    cases = [c for _, c in lp_cases.all_cases()]
    models = models_of(cases)
    b = PrimalSimplexBatch(models, engine=engine, log_cap=CAP)
    b.Solve(max_pivots=CAP)
    for k, (obj, cons, mx) in enumerate(models):
        s = PrimalSimplexSolver(obj, cons, mx, engine=engine, snapshots="none")
        s.Solve(max_pivots=CAP)
        assert b.Status[k] == s.Status
        assert np.float64(b.FinalZ[k]).tobytes() == np.float64(s.FinalZ).tobytes()
        if s.SolutionVector is None:
            assert b.SolutionVector[k] is None
        else:
            assert np.asarray(b.SolutionVector[k]).tobytes() == \
                np.asarray(s.SolutionVector).tobytes()
        assert b.Iterations[k] == s.iteration
        assert b.BasicVariables(k) == s.BasicVariables
        assert np.array_equal(b.PivotLog(k), s.PivotLog)
        assert b.GetFinalTableau(k).tobytes() == s.GetFinalTableau().tobytes()
        if s.Status == 1:
            assert b.FinalZ[k] == 0.0 and b.SolutionVector[k] is None
    parsers = []
    for i, text in enumerate((lp_cases.SAMPLE_MODEL, lp_cases.README_MODEL)):
        path = tmp_path / f"model{i}.txt"
        path.write_text(text)
        p = InputFileParser()
        p.ReadInputFile(str(path))
        parsers.append(p)
    pb = PrimalSimplexBatch.from_parsers(parsers, engine=engine)
    pb.Solve(max_pivots=CAP)
    for k, p in enumerate(parsers):
        s = PrimalSimplexSolver(p.ObjectiveCoefficients, p.Constraints,
                                (p.ProblemType or "").lower() != "min", engine=engine,
                                snapshots="none")
        s.Solve(max_pivots=CAP)
        assert pb.Status[k] == s.Status and pb.FinalZ[k] == s.FinalZ
        assert pb.GetFinalTableau(k).tobytes() == s.GetFinalTableau().tobytes()


# ------------------------------------------------------------------------------ 8. bad arguments
def _arr(a, t):
    a = np.ascontiguousarray(a, dtype=t)
    return a, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(t)))


def _from_lps(engine, n, m, obj, A, ncoef, rel, rhs, is_max, count=None, log_cap=0):
    from lpr_381_group_v22_amd import _native as N
    keep = []

    def p(a, t):
        if a is None:
            return None
        arr, ptr = _arr(a, t)
        keep.append(arr)
        return ptr
    h = C.c_void_p()
    rc = N.lib.lpr_batch_from_lps(engine._h, len(n) if count is None else count,
                                  p(n, np.int32), p(m, np.int32), p(obj, np.float64),
                                  p(A, np.float64), p(ncoef, np.int32), p(rel, np.int8),
                                  p(rhs, np.float64), p(is_max, np.int8), log_cap, C.byref(h))
    return rc, h, N.lib.lpr_last_error().decode()


def test_bad_arguments(engine):
    from lpr_381_group_v22_amd import _native as N
    ok = dict(n=[2], m=[1], obj=[1.0, 1.0], A=[1.0, 1.0], ncoef=[2], rel=[0], rhs=[4.0],
              is_max=[1])
    rc, h, _ = _from_lps(engine, **ok)
    assert rc == 0
    assert N.lib.lpr_batch_destroy(h) == 0
    bad = [
        (dict(ok, count=0), "count=0"),
        (dict(ok, n=None, count=1), "null"),
        (dict(ok, n=[-1]), "n=-1"),
        (dict(ok, m=[-2]), "m=-2"),
        (dict(ok, ncoef=[3]), "ncoef=3 outside"),
        (dict(ok, ncoef=[-1]), "ncoef=-1 outside"),
        (dict(ok, rel=[3]), "relation code 3"),
        (dict(ok, rhs=None), "null objective / A / relation / rhs"),
        (dict(ok, n=[0], m=[0], obj=[], A=[], ncoef=[], rel=[], rhs=[]), "cols >= 2"),
        (dict(ok, n=[1], m=[1024], obj=[1.0], A=[1.0] * 1024, ncoef=[1] * 1024,
              rel=[0] * 1024, rhs=[1.0] * 1024), "lpr_primal_solve"),
        (dict(ok, n=[2 ** 31 - 1], m=[1]), "lpr_primal_solve"),
        (dict(ok, log_cap=-1), "log_cap=-1"),
    ]
    for kw, text in bad:
        rc, h, err = _from_lps(engine, **kw)
        assert rc == N.LPR_BAD_ARGUMENT, (kw, rc)
        assert text in err, (text, err)
    # ready tableaux
    T, Tp = _arr(np.zeros(6), np.float64)
    for rows, cols, text in (([0], [2], "rows >= 1"), ([3], [1], "cols >= 2"),
                             ([1025], [4], "lpr_primal_solve"), ([2], [2049], "lpr_primal_solve")):
        r, rp = _arr(rows, np.int32)
        c, cp = _arr(cols, np.int32)
        h = C.c_void_p()
        assert N.lib.lpr_batch_create(engine._h, 1, rp, cp, Tp, None, 0, C.byref(h)) == \
            N.LPR_BAD_ARGUMENT
        assert text in N.lib.lpr_last_error().decode()
    # reads and options
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    b = PrimalSimplexBatch(models_of([lp_cases.min_lp()]), engine=engine)
    cnt = C.c_int64()
    for k in (-1, 1):
        assert N.lib.lpr_batch_log_read(b._h, k, None, None, 4, C.byref(cnt)) == \
            N.LPR_BAD_ARGUMENT
        assert "out of range" in N.lib.lpr_last_error().decode()
        out = np.zeros(64)
        assert N.lib.lpr_batch_tableau_read(b._h, k, out.ctypes.data_as(C.POINTER(C.c_double))) \
            == N.LPR_BAD_ARGUMENT
    opts = N.BatchOpts(max_pivots=0, chunk=0, variant=9)
    res = N.BatchResult()
    assert N.lib.lpr_batch_solve(b._h, C.byref(opts), C.byref(res)) == N.LPR_BAD_ARGUMENT


def test_handle_after_engine_close_is_orphaned():
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    eng = pkg.Engine(0)
    b = pkg.PrimalSimplexBatch(models_of([lp_cases.min_lp()]), engine=eng)
    eng.close()
    with pytest.raises(N.EngineError, match="orphaned"):
        b.Solve()
    res = N.BatchResult()
    assert N.lib.lpr_batch_solve(b._h, None, C.byref(res)) == N.LPR_BAD_ARGUMENT
    b.destroy()  # still safe
