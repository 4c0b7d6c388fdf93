"""GPU parity tests of the cutting-plane batch (lpr_cut_batch_*): every item
of a batch ends with the exit code / status, the cuts, the log, the shape and the tableau bits the
oracle gives for that item alone."""
import ctypes

import numpy as np
import pytest

import cut_batch_cases as cb
import cut_cases
import special_values as sv

pytestmark = pytest.mark.gpu


def check_item(batch, k, ref, res=None, what="", nan=False, log_prefix=()):
    """Item k against one reference (cut_batch_cases.reference); log_prefix: the triples earlier
    calls on the handle have left."""
    res = batch.result_arrays() if res is None else res
    what = (what, k)
    assert int(res["code"][k]) == ref["code"], what
    assert int(res["cuts"][k]) == ref["cuts"], what
    want = list(log_prefix) + [tuple(t) for t in ref["log"]]
    assert int(res["log_count"][k]) == len(want), what
    cap = batch.LogCap(k)
    assert batch.Log(k) == want[:cap], what
    assert batch.LogCount(k) == len(want), what
    T = batch.Tableau(k)
    assert batch.Shape(k) == ref["T"].shape == T.shape, what
    assert int(res["rows"][k]) == ref["T"].shape[0], what
    if nan:
        sv.assert_same(T, ref["T"], what)
    else:
        assert T.tobytes() == ref["T"].tobytes(), what
    assert sv.same(res["z"][k], ref["T"][0, -1]), what


def check_batch(batch, refs, what="", **kw):
    res = batch.result_arrays()
    for k, ref in enumerate(refs):
        check_item(batch, k, ref, res=res, what=what, **kw)


# ------------------------------------------------------------------ 1. every exit, both forms
@pytest.fixture(scope="module")
def textbook(oracle):
    return cb.textbook_items(oracle)


@pytest.fixture(scope="module")
def textbook_refs(oracle, textbook):
    """(max_cuts, hard_cap) -> references per item; computed once, never changed."""
    return {(mc, hc): [cb.reference(oracle, cb.MODE_CUT, T, max_cuts=mc, hard_cap=hc)
                       for _, T in textbook]
            for mc in (1, 6) for hc in (2000, 2, 1)}


@pytest.mark.parametrize("variant", [0, 2, 3])
def test_every_exit_both_forms(engine, textbook, textbook_refs, variant):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    names = [n for n, _ in textbook]
    exits = set()
    for (mc, hc), refs in textbook_refs.items():
        batch = CuttingPlaneBatch.from_arrays(engine, [T for _, T in textbook], max_cuts=mc)
        res = batch.Run(hard_cap=hc, variant=variant)
        check_batch(batch, refs, (variant, mc, hc))
        assert list(res.by_code) == [sum(r["code"] == c for r in refs) for c in range(8)]
        assert res.cuts == sum(r["cuts"] for r in refs)
        assert res.pivots == sum(r["pivots"] for r in refs)
        assert (res.items_g, res.items_h) == ((0, len(refs)) if variant == 3 else (len(refs), 0))
        exits |= {r["code"] for r in refs}
        if mc == 6:
            code = {n: r["code"] for n, r in zip(names, refs)}
            cuts = {n: r["cuts"] for n, r in zip(names, refs)}
            if hc == 2000:
                assert code["huge_relaxation_value"] == 5
                assert (code["binary_10v2c_s4"], cuts["binary_10v2c_s4"]) == (0, 6)
            if hc == 1:
                assert code["huge_relaxation_value"] == 4
                assert (code["binary_10v2c_s4"], cuts["binary_10v2c_s4"]) == (4, 1)
        batch.destroy()
    assert exits == {0, 1, 2, 4, 5, 6}


# ------------------------------------------------------------------ 2. modes 1 and 2
@pytest.mark.parametrize("mode", [cb.MODE_DUAL, cb.MODE_PRIMAL2])
def test_solver_modes_match_the_single_solvers(engine, oracle, mode):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    tabs = (cut_cases.dual_tableaux if mode == cb.MODE_DUAL else cut_cases.primal2_tableaux)(oracle)
    T0 = [T for _, T in tabs]
    seen = set()
    for kw in (dict(hard_cap=3000), dict(max_iters=1, print_steps=True, hard_cap=3000),
               dict(max_iters=1, print_steps=False, hard_cap=3000)):
        refs = [cb.reference(oracle, mode, T, **kw) for T in T0]
        for variant in (0, 3):
            batch = CuttingPlaneBatch.from_arrays(engine, T0, max_cuts=2)
            res = batch.Run(mode=mode, variant=variant, **kw)
            check_batch(batch, refs, (mode, kw, variant))
            assert res.pivots == sum(r["pivots"] for r in refs)
            assert res.cuts == 0
            assert list(res.by_code) == [sum(r["code"] == c for r in refs) for c in range(8)]
            batch.destroy()
        seen |= {r["code"] for r in refs}
        if kw.get("max_iters") == 1 and kw["print_steps"]:   # the `iter` quirk
            assert all(r["pivots"] <= 1 for r in refs) and 5 in {r["code"] for r in refs}
    assert {0, 5} <= seen and (mode == cb.MODE_DUAL or 1 in seen)


# ------------------------------------------------------------------ 3. lane and walk strides
@pytest.mark.parametrize("form", ["G", "H"])
@pytest.mark.parametrize("gen_name", list(cb.STRIDE_GENS))
def test_lane_and_walk_strides(engine, oracle, gen_name, form):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    mode, field, items = cb.stride_group(gen_name, form)
    refs = [cb.stride_reference(oracle, mode, T) for _, T, _ in items]
    batch = CuttingPlaneBatch.from_arrays(engine, [T for _, T, _ in items], max_cuts=1)
    res = batch.Run(mode=mode, hard_cap=cb.STRIDE_HARD_CAP)
    n = len(items)
    assert (res.items_g, res.items_h) == ((n, 0) if form == "G" else (0, n))
    a = batch.result_arrays()
    for k, ((name, _, planted), ref) in enumerate(zip(items, refs)):
        assert ref["log"][0][field] == planted, name
        assert batch.Log(k)[0][field] == planted, name
        check_item(batch, k, ref, res=a, what=name)
    batch.destroy()


# ------------------------------------------------------------------ 4. mixed shapes and forms
@pytest.fixture(scope="module")
def larger_refs(oracle):
    (Tg, mg), (Th, mh) = cb.g_item(), cb.h_item()
    rg = cb.reference(oracle, cb.MODE_CUT, Tg, max_cuts=mh)   # the handle's capacity, not mg
    rh = cb.reference(oracle, cb.MODE_CUT, Th, max_cuts=mh)
    assert (rh["code"], rh["cuts"], rh["pivots"]) == cb.H_ITEM_OUTCOME
    return rg, rh


def test_mixed_shapes_and_forms_in_one_batch(engine, oracle, textbook, larger_refs):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    (Tg, _), (Th, mh) = cb.g_item(), cb.h_item()
    rg, rh = larger_refs
    small = [T for _, T in textbook[:6]]
    small_refs = [cb.reference(oracle, cb.MODE_CUT, T, max_cuts=mh) for T in small]
    tabs, refs = [], []
    for q in range(3):   # interleaved: textbook, H, textbook, G, ...
        tabs += [small[2 * q], Th, small[2 * q + 1], Tg]
        refs += [small_refs[2 * q], rh, small_refs[2 * q + 1], rg]
    batch = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=mh)
    res = batch.Run()
    assert (res.items_g, res.items_h) == (9, 3)
    check_batch(batch, refs, "mixed")
    assert res.cuts == sum(r["cuts"] for r in refs)
    batch.destroy()


# ------------------------------------------------------------------ 5. the launch bound
@pytest.mark.parametrize("which,chunk", [("H", 16), ("H", 15), ("G", 8)])
def test_launch_bound(engine, oracle, which, chunk):
    """an item stops only in front of a pivot with its chunk used up, so an
    item that ends with no refused pivot pending takes max(1, ceil(pivots / chunk)) launches."""
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    from lpr_381_group_v22_amd.cut_batch import launches_for
    T, mc = cb.h_item() if which == "H" else cb.g_item()
    ref = cb.reference(oracle, cb.MODE_CUT, T, max_cuts=mc)
    assert (ref["code"], ref["cuts"], ref["pivots"]) == (cb.H_ITEM_OUTCOME if which == "H"
                                                         else cb.G_ITEM_OUTCOME)
    bits = []
    for ch in (chunk, 0):
        batch = CuttingPlaneBatch.from_arrays(engine, [T], max_cuts=mc)
        res = batch.Run(chunk=ch)
        check_item(batch, 0, ref, what=(which, ch))
        assert res.pivots == ref["pivots"]
        default = 16 if which == "H" else 128
        assert res.launches == launches_for(ref["pivots"], ch or default), (which, ch)
        bits.append(batch.Tableau(0).tobytes())
        batch.destroy()
    assert bits[0] == bits[1]
    assert launches_for(ref["pivots"], chunk) == {("H", 16): 4, ("H", 15): 4, ("G", 8): 3}[
        (which, chunk)]


# ------------------------------------------------------------------ 6. calls in sequence
def test_calls_in_sequence_on_one_handle(engine, oracle, textbook):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    T0 = [T for _, T in textbook]
    batch = CuttingPlaneBatch.from_arrays(engine, T0, max_cuts=6)
    first = [cb.reference(oracle, cb.MODE_CUT, T, max_cuts=1, hard_cap=2000) for T in T0]
    batch.Run(max_cuts=1, hard_cap=2000)
    check_batch(batch, first, "first call")
    second = [cb.reference(oracle, cb.MODE_CUT, r["T"], max_cuts=5, hard_cap=2000,
                           rcap=T.shape[0] + 6) for r, T in zip(first, T0)]
    batch.Run(max_cuts=5, hard_cap=2000)
    res = batch.result_arrays()
    for k, (a, b) in enumerate(zip(first, second)):
        check_item(batch, k, b, res=res, what="second call", log_prefix=a["log"])
    assert any(b["cuts"] > 0 for b in second) and any(a["log"] and b["log"]
                                                      for a, b in zip(first, second))
    batch.destroy()


def test_no_capacity_left_gives_exit_6_or_1(engine, oracle, textbook):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    T0 = [T for _, T in textbook]
    batch = CuttingPlaneBatch.from_arrays(engine, T0, max_cuts=1)
    first = [cb.reference(oracle, cb.MODE_CUT, T, max_cuts=1, hard_cap=2000) for T in T0]
    batch.Run(hard_cap=2000)
    check_batch(batch, first, "first call")
    for asked in (0, 3):   # no capacity left whatever the call asks for
        second = [cb.reference(oracle, cb.MODE_CUT, r["T"], max_cuts=asked, hard_cap=2000,
                               rcap=T.shape[0] + 1) for r, T in zip(first, T0)]
        batch.Run(max_cuts=asked, hard_cap=2000)
        res = batch.result_arrays()
        for k, (a, b) in enumerate(zip(first, second)):
            check_item(batch, k, b, res=res, what=("no capacity", asked), log_prefix=a["log"])
            if a["cuts"] == 1:
                assert b["code"] in (1, 6) and b["cuts"] == 0
        full = [b["code"] for a, b in zip(first, second) if a["cuts"] == 1]
        assert 6 in full and 1 in [b["code"] for b in second]
    batch.destroy()


def test_dual_mode_then_cutting_plane(engine, oracle):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    T0 = [T for _, T in cut_cases.dual_tableaux(oracle)]
    batch = CuttingPlaneBatch.from_arrays(engine, T0, max_cuts=3)
    first = [cb.reference(oracle, cb.MODE_DUAL, T, hard_cap=2000) for T in T0]
    batch.Run(mode=cb.MODE_DUAL, hard_cap=2000)
    check_batch(batch, first, "dual")
    second = [cb.reference(oracle, cb.MODE_CUT, r["T"], max_cuts=3, hard_cap=2000) for r in first]
    batch.Run(hard_cap=2000)
    res = batch.result_arrays()
    for k, (a, b) in enumerate(zip(first, second)):
        check_item(batch, k, b, res=res, what="cut after dual", log_prefix=a["log"])
    assert any(a["log"] and b["log"] for a, b in zip(first, second))
    batch.destroy()


# ------------------------------------------------------------------ 7. the form boundary
def test_form_boundary(engine, oracle):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    from lpr_381_group_v22_amd import cut_batch as pycb
    m, mc = 40, 8
    n_fit, n_over = cb.boundary_shapes(m, mc)
    tabs = [cut_cases.side_base(m, n_fit, 11), cut_cases.side_base(m, n_over, 11)]
    assert pycb.footprint_g(m + 1, n_fit + m + 1, mc) <= pycb.MAX_LDS_G
    assert pycb.footprint_g(m + 1, n_over + m + 1, mc) > pycb.MAX_LDS_G
    refs = [cb.reference(oracle, cb.MODE_CUT, T, max_cuts=mc) for T in tabs]
    assert all(r["cuts"] == mc for r in refs)   # the capacity is used up: every row of LDS is
    batch = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=mc)
    res = batch.Run()
    assert (res.items_g, res.items_h) == (1, 1)
    check_batch(batch, refs, "boundary, auto")
    batch.destroy()
    batch = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=mc)
    res = batch.Run(variant=pycb.VARIANT_H)
    assert (res.items_g, res.items_h) == (0, 2)
    check_batch(batch, refs, "boundary, H")
    batch.destroy()
    batch = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=mc)
    res = batch.Run(variant=pycb.VARIANT_G)   # the second does not fit G: it stays in H
    assert (res.items_g, res.items_h) == (1, 1)
    check_batch(batch, refs, "boundary, G forced")
    batch.destroy()


# ------------------------------------------------------------------ 8. against the single handle
@pytest.mark.parametrize("max_cuts,hard_cap", [(1, 2000), (6, 2000), (6, 1)])
def test_against_the_single_handle(engine, textbook, max_cuts, hard_cap):
    from lpr_381_group_v22_amd import CuttingPlaneBatch, Tableau
    T0 = [T for _, T in textbook]
    batch = CuttingPlaneBatch.from_arrays(engine, T0, max_cuts=max_cuts)
    batch.Run(hard_cap=hard_cap)
    res = batch.result_arrays()
    for k, (name, T) in enumerate(textbook):
        tab = Tableau.from_array(engine, T)
        ex, cuts = tab.cutting_plane(max_cuts=max_cuts, hard_cap=hard_cap)
        assert (int(res["code"][k]), int(res["cuts"][k])) == (ex, cuts), name
        assert batch.Log(k) == tab.cut_log(), name
        got, one = batch.Tableau(k), tab.read()
        assert got.shape == one.shape and got.tobytes() == one.tobytes(), name
        tab.destroy()
    batch.destroy()


# ------------------------------------------------------------------ 9. from a solved LP batch
def _models():
    import bb_cases
    from lpr_381_group_v22_amd import Constraint
    return [(list(obj), [Constraint(list(c.Coefficients), c.Relation, c.RHS) for c in cons], True)
            for _, (obj, cons) in bb_cases.all_bb_cases()]


def test_from_primal_batch(engine, oracle):
    from lpr_381_group_v22_amd import CuttingPlaneBatch, PrimalSimplexBatch
    lp = PrimalSimplexBatch(_models(), engine=engine)
    lp.Solve()
    batch = CuttingPlaneBatch.from_primal_batch(lp, max_cuts=6)
    lp.destroy()   # the new handle does not depend on it
    roots = cut_cases.cutting_plane_tableaux(oracle)   # the oracle's final tableaux
    assert batch.Count == len(roots)
    for k, (name, T) in enumerate(roots):
        assert batch.Tableau(k).tobytes() == T.tobytes(), name
    refs = [cb.reference(oracle, cb.MODE_CUT, T, max_cuts=6, hard_cap=2000) for _, T in roots]
    batch.Run(hard_cap=2000)
    check_batch(batch, refs, "from_primal_batch")
    batch.destroy()


def test_lp_at_pivot_limit_is_refused_by_name(engine):
    from lpr_381_group_v22_amd import CuttingPlaneBatch, PrimalSimplexBatch, _native as N
    lp = PrimalSimplexBatch(_models()[:3], engine=engine)
    with pytest.raises(N.EngineError) as ei:   # never solved
        CuttingPlaneBatch.from_primal_batch(lp)
    assert ei.value.status == N.LPR_BAD_ARGUMENT
    assert "LP 0 " in N.lib.lpr_last_error().decode()
    lp.Solve(max_pivots=1)
    bad = [k for k in range(lp.Count) if lp.Status[k] == N.LPR_PIVOT_LIMIT]
    assert bad
    with pytest.raises(N.EngineError) as ei:
        CuttingPlaneBatch.from_primal_batch(lp)
    assert ei.value.status == N.LPR_BAD_ARGUMENT
    assert f"LP {bad[0]} " in N.lib.lpr_last_error().decode()
    lp.destroy()


# ------------------------------------------------------------------ 10. a NaN factor
def test_nan_factor(engine, oracle):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    for mode, T, victim, col in cb.nan_factor_cases(oracle):
        ref = cb.reference(oracle, mode, T, hard_cap=50)
        one = cb.reference(oracle, mode, T, hard_cap=1)
        for variant in (0, 3):
            batch = CuttingPlaneBatch.from_arrays(engine, [T, T], max_cuts=1)
            batch.Run(mode=mode, hard_cap=1, variant=variant)
            check_item(batch, 0, one, what=(mode, "one pivot"), nan=True)
            row = batch.Tableau(0)[victim]
            if mode == cb.MODE_PRIMAL2:   # `|f| <= EPS` is false for NaN: the row is rewritten
                assert np.isnan(row).all()
            else:                         # `|f| > EPS` is false for NaN: the row stays
                assert np.isnan(row).sum() == 1 and np.isnan(row[col])
            batch.destroy()
            batch = CuttingPlaneBatch.from_arrays(engine, [T, T], max_cuts=1)
            batch.Run(mode=mode, hard_cap=50, variant=variant)
            check_batch(batch, [ref, ref], (mode, "hard_cap 50"), nan=True)
            batch.destroy()


# ------------------------------------------------------------------ 11. arguments
def test_arguments(engine, oracle, textbook):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import CuttingPlaneBatch, _native as N
    lib = N.lib
    I32, D = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)

    def create(shape, max_cuts):
        T = np.zeros(shape)
        r, c = (np.asarray([v], dtype=np.int32) for v in shape)
        h = ctypes.c_void_p()
        rc = lib.lpr_cut_batch_create(engine._h, 1, r.ctypes.data_as(I32), c.ctypes.data_as(I32),
                                      T.ctypes.data_as(D), max_cuts, 0, ctypes.byref(h))
        return rc, lib.lpr_last_error().decode()

    for shape, mc, word in (((1, 5), 1, "rows >= 2"), ((3, 1), 1, "cols >= 2"),
                            ((1000, 5), 25, "lpr_cutting_plane"),
                            ((961, 5), 0, "lpr_cutting_plane"),
                            ((3, 2049), 1, "lpr_cutting_plane")):
        rc, msg = create(shape, mc)
        assert rc == N.LPR_BAD_ARGUMENT and word in msg and "item 0" in msg, (shape, msg)

    name, T = textbook[0]
    ref = cb.reference(oracle, cb.MODE_CUT, T, max_cuts=2, hard_cap=2000)
    batch = CuttingPlaneBatch.from_arrays(engine, [T], max_cuts=2)
    res = N.CutBatchResult()
    out = np.zeros(T.size + 4 * T.shape[1])
    cnt = ctypes.c_int64()
    r4 = [ctypes.c_int32() for _ in range(4)]
    calls = [
        ("null handle", lambda: lib.lpr_cut_batch_run(None, None, ctypes.byref(res)), "null"),
        ("null result", lambda: lib.lpr_cut_batch_run(batch._h, None, None), "null result"),
        ("unknown mode", lambda: lib.lpr_cut_batch_run(
            batch._h, ctypes.byref(N.CutBatchOpts(mode=3)), ctypes.byref(res)), "mode 3"),
        ("unknown variant", lambda: lib.lpr_cut_batch_run(
            batch._h, ctypes.byref(N.CutBatchOpts(variant=1)), ctypes.byref(res)), "variant 1"),
        ("k past the end", lambda: lib.lpr_cut_batch_tableau_read(
            batch._h, 1, out.ctypes.data_as(D)), "item 1"),
        ("k negative", lambda: lib.lpr_cut_batch_log_read(
            batch._h, -1, None, 0, ctypes.byref(cnt)), "item -1"),
        ("k past the end (shape)", lambda: lib.lpr_cut_batch_shape(
            batch._h, 7, *[ctypes.byref(v) for v in r4]), "item 7"),
    ]
    for what, call, word in calls:
        assert call() == N.LPR_BAD_ARGUMENT, what
        assert word in lib.lpr_last_error().decode(), (what, lib.lpr_last_error())
    batch.Run(hard_cap=2000)   # the handle is still usable
    check_item(batch, 0, ref, what="after refused calls")
    batch.destroy()

    # a handle whose engine has been closed is orphaned: refused, and destroy stays safe
    eng2 = pkg.Engine(0)
    orphan = CuttingPlaneBatch.from_arrays(eng2, [T], max_cuts=2)
    eng2.close()
    assert lib.lpr_cut_batch_run(orphan._h, None, ctypes.byref(res)) == N.LPR_BAD_ARGUMENT
    assert "orphaned" in lib.lpr_last_error().decode()
    assert lib.lpr_cut_batch_z_read(orphan._h, out.ctypes.data_as(D)) == N.LPR_BAD_ARGUMENT
    orphan.destroy()
