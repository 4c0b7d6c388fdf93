"""GPU tests of the batched Branch & Bound (lpr_bb_batch_*): every IP of a batch
against the CPU oracle's orc_bb_solve on that root alone -- status, found, processed, best_node, the
bits of z and x, every node record, the pop order and the pivot trace -- and its pivot and node
counts against lpr_bb_run; across the three forms, node caps, pruning, resumed launches, short
traces, repeated runs, the from-batch path of option 3, the child pivot limit and bad arguments."""
import ctypes as C

import numpy as np
import pytest

import bb_cases

pytestmark = pytest.mark.gpu

PIV_CAP = 1 << 16
W_MAX, G_MAX = (64 * 1024 - 1024) // 4, 160 * 1024 - 1024  # kBatchMaxLdsW / kBatchMaxLdsG


def footprint_bytes(T, cap):
    r, c = T.shape[0] + cap, T.shape[1] + cap
    return 8 * (2 * r * c + r)


def form_of(T, cap):
    b = footprint_bytes(T, cap)
    return 0 if b <= W_MAX else (1 if b <= G_MAX else 2)


def bits(v):
    return np.float64(v).tobytes()


_ROOTS = {}


def bb_roots(oracle):
    """(name, root, nvars) for every B&B case, the sample knapsack first: Program.cs option 3 up to
    the primal FinalTableau, nvars as SolveFromPrimal sets it."""
    if "bb" not in _ROOTS:
        out = []
        for name, (obj, cons) in bb_cases.all_bb_cases():
            st, T, n = bb_cases.primal_final_tableau(oracle, obj, cons)
            out.append((name, T, n if st == 0 else max(1, T.shape[1] - 1)))
        _ROOTS["bb"] = out
    return _ROOTS["bb"]


def edge_roots(oracle, cap):
    """The edge and big-value instances whose full depth stays within form H."""
    out = []
    for c in bb_cases.edge_cases(oracle, widest=False):
        T = c["T"]
        if T.shape[0] + cap <= 1024 and T.shape[1] + cap <= 2048:
            out.append((c["name"], T, c["nvars"]))
    return out


def big_roots(oracle):
    return [(c["name"], c["T"], c["nvars"]) for c in bb_cases.big_value_cases(oracle)]


def check_ip(bb, k, T, nv, oracle, cap, pruning=False, trace_cap=None, arrays=None, xs=None,
             ref=None):
    ref = ref or oracle.bb_solve(T, nv, enable_pruning=pruning, node_cap=cap, piv_cap=PIV_CAP)
    a = arrays if arrays is not None else bb.result_arrays()
    x = xs if xs is not None else bb.solution_packed()
    assert a["status"][k] == ref["status"], (k, a["status"][k], ref["status"])
    assert bool(a["found"][k]) == ref["found"], k
    assert a["processed"][k] == ref["processed"], k
    assert a["best_node"][k] == ref["best_node"], k
    assert bits(a["z"][k]) == bits(ref["z"]), (k, a["z"][k], ref["z"])
    at = sum(bb.nvars[:k])
    xk = x[at:at + nv]
    if ref["found"]:
        assert xk.tobytes() == np.asarray(ref["x"], dtype=np.float64).tobytes(), f"IP {k}: x"
    else:
        assert not np.any(xk), f"IP {k}: x without an incumbent is 0"
    recs = bb.Records(k)
    assert len(recs) == len(ref["records"]) == a["nodes_created"][k], k
    for q, (g, r) in enumerate(zip(recs, ref["records"])):
        for f in ("parent", "kind", "depth", "var", "status"):
            assert g[f] == r[f], (k, q, f, g, r)
        assert bits(g["bound"]) == bits(r["bound"]) and bits(g["z"]) == bits(r["z"]), (k, q, g, r)
    assert bb.PopOrder(k) == ref["pop_order"], k
    assert a["pivots"][k] == len(ref["trace"]), (k, a["pivots"][k], len(ref["trace"]))
    tr = bb.Trace(k)
    keep = len(ref["trace"]) if trace_cap is None else min(trace_cap, len(ref["trace"]))
    assert tr == [tuple(t) for t in ref["trace"][:keep]], f"IP {k}: trace"
    return ref


def check_batch(bb, roots, oracle, cap, pruning=False, trace_cap=None, refs=None):
    a = bb.result_arrays()
    x = bb.solution_packed()
    out = []
    for k, (_, T, nv) in enumerate(roots):
        out.append(check_ip(bb, k, T, nv, oracle, cap, pruning, trace_cap, a, x,
                            refs[k] if refs else None))
    return out


def make(engine, roots, cap, trace_cap=PIV_CAP):
    from lpr_381_group_v22_amd import BranchAndBoundBatch
    return BranchAndBoundBatch.from_tableaux([T for _, T, _ in roots], [n for _, _, n in roots],
                                             node_cap=cap, trace_cap=trace_cap, engine=engine)


# ------------------------------------------------------------------------- 1. one mixed batch
def test_mixed_batch_spans_all_forms_and_matches_lpr_bb_run(engine, oracle):
    from lpr_381_group_v22_amd import BranchBoundTree
    cap = 20
    roots = bb_roots(oracle) + edge_roots(oracle, cap)
    assert {form_of(T, cap) for _, T, _ in roots} == {0, 1, 2}
    assert form_of(bb_roots(oracle)[0][1], cap) == 0  # the sample model takes W
    bb = make(engine, roots, cap)
    res = bb.Run()
    assert res.done + res.node_cap + res.pivot_limit == len(roots) and res.pivot_limit == 0
    check_batch(bb, roots, oracle, cap)
    a = bb.result_arrays()
    for k, (name, T, nv) in enumerate(roots):
        tree = BranchBoundTree.from_array(engine, T, nv, max_depth=cap)
        r, _ = tree.run(enable_pruning=False, node_cap=cap)
        assert a["pivots"][k] == r.pivots and a["nodes_created"][k] == r.nodes_created, name
        tree.destroy()
    assert res.pops == int(a["processed"].sum()) and res.pivots == int(a["pivots"].sum())
    bb.destroy()


# ------------------------------------------------------------------ 2. node caps and pruning
@pytest.mark.parametrize("cap", [1, 20, 64])
@pytest.mark.parametrize("pruning", [False, True])
def test_node_caps_and_pruning(engine, oracle, cap, pruning):
    roots = bb_roots(oracle) + big_roots(oracle)
    bb = make(engine, roots, cap)
    bb.Run(enable_pruning=pruning)
    check_batch(bb, roots, oracle, cap, pruning)
    bb.destroy()


# ------------------------------------------------------------------------- 3. every form
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_every_form_it_fits(engine, oracle, variant):
    cap = 20
    roots = bb_roots(oracle) + big_roots(oracle) + edge_roots(oracle, cap)
    lim = {1: W_MAX, 2: G_MAX, 3: None}[variant]
    roots = [r for r in roots if lim is None or footprint_bytes(r[1], cap) <= lim]
    assert roots
    bb = make(engine, roots, cap)
    bb.Run(variant=variant)
    check_batch(bb, roots, oracle, cap)
    bb.destroy()


# ------------------------------------------- 4. resumed launches, short trace, a second run
def test_chunk_one_short_trace_and_second_run(engine, oracle):
    cap = 20
    roots = bb_roots(oracle) + big_roots(oracle)
    refs = [oracle.bb_solve(T, nv, node_cap=cap, piv_cap=PIV_CAP) for _, T, nv in roots]
    bb = make(engine, roots, cap, trace_cap=3)
    r1 = bb.Run(chunk=1)
    assert r1.launches >= max(r["processed"] for r in refs)
    check_batch(bb, roots, oracle, cap, trace_cap=3, refs=refs)
    first = bb.result_arrays()
    r2 = bb.Run()  # from the roots again
    assert r2.pops == r1.pops and r2.pivots == r1.pivots
    check_batch(bb, roots, oracle, cap, trace_cap=3, refs=refs)
    second = bb.result_arrays()
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), key
    bb.destroy()


def _optimal_roots(oracle):
    """IPs of all three forms at node cap 20 whose search ends by emptying its stack: neither the
    node cap nor a child pivot limit is met.  Form H: a product-route root made tall."""
    if "optimal" not in _ROOTS:
        keep = ("knapsack_sample", "binary_4v1c_s0", "frac_4v2c_s10", "tall_frac6x3_nv_all",
                "tall_bin8x3_nv_all")
        out = [r for r in bb_roots(oracle) + edge_roots(oracle, 20) if r[0] in keep]
        T, _ = bb_cases._product_root(oracle, bb_cases.fractional_program, 6, 3, 11)
        t = bb_cases._tall(T, 270, 0)
        out.append(("tall_frac6x3_280_rows", t, t.shape[1] - 1))
        T, _ = bb_cases._product_root(oracle, bb_cases.random_binary_program, 8, 3, 3)
        t = bb_cases._tall(T, 300, 1)
        out.append(("tall_bin8x3_312_rows", t, t.shape[1] - 1))
        _ROOTS["optimal"] = out
    return _ROOTS["optimal"]


def expected_launches(forms, processed, chunk):
    """Launches of one Run call: the sum over the forms of max over the form's IPs of
    processed // chunk + 1.  A launch runs at most `chunk` iterations of the DFS loop per IP; an
    iteration pops one node, and the one that finds the stack empty ends the IP, so an IP needs
    processed + 1 iterations; every round launches each form that still has an IP once.  (A run
    always starts from the roots, so there is no resumed call to count.)"""
    total = 0
    for f in set(forms):
        total += max(p // chunk + 1 for ff, p in zip(forms, processed) if ff == f)
    return total


def test_exact_launch_counts_through_mixed_forms(engine, oracle):
    cap = 20
    roots = _optimal_roots(oracle)
    refs = [oracle.bb_solve(T, nv, node_cap=cap, piv_cap=PIV_CAP) for _, T, nv in roots]
    forms = [form_of(T, cap) for _, T, _ in roots]
    pops = [r["processed"] for r in refs]
    assert sorted(set(forms)) == [0, 1, 2] and all(r["status"] == 0 for r in refs)
    assert all(rec["status"] != 5 for r in refs for rec in r["records"])  # no child pivot limit
    assert len(set(pops)) > 3
    bb = make(engine, roots, cap)
    for chunk in (1, 3):
        res = bb.Run(chunk=chunk)
        print("chunk", chunk, "launches", res.launches, "pops", res.pops)
        assert res.done == len(roots) and res.node_cap == 0 and res.pivot_limit == 0
        check_batch(bb, roots, oracle, cap, refs=refs)
        assert res.pops == sum(pops) and res.pivots == sum(len(r["trace"]) for r in refs)
        assert res.launches == expected_launches(forms, pops, chunk), (chunk, res.launches)
    bb.destroy()


# ------------------------------------------------------------------- 5. the from-batch path
def _parser(obj, cons):
    from lpr_381_group_v22_amd import Constraint, InputFileParser
    return InputFileParser(ProblemType="max", ObjectiveCoefficients=list(obj),
                           Constraints=[Constraint(list(c.Coefficients), c.Relation, c.RHS)
                                        for c in cons], SignRestrictions=["bin"] * len(obj))


def _models():
    """The B&B cases as raw models (objective, constraints): option 3 adds the unit rows."""
    return [(name, obj, cons[:len(cons) - len(obj)]) for name, (obj, cons) in
            bb_cases.all_bb_cases()]


def test_from_primal_batch_matches_solve_from_primal(engine, oracle):
    from lpr_381_group_v22_amd import (BranchAndBoundAdapter, BranchAndBoundBatch, Constraint,
                                       PrimalSimplexBatch, PrimalSimplexSolver)
    from lpr_381_group_v22_amd.bb_batch import option3_models
    parsers = [_parser(obj, cons) for _, obj, cons in _models()]
    models = option3_models(parsers)
    models.append(([1.0, 1.0], [Constraint([1.0, -1.0], "<=", 1.0)], True))  # unbounded
    lp = PrimalSimplexBatch(models, engine=engine)
    lp.Solve()
    assert lp.Status[-1] == 1  # LPR_UNBOUNDED
    cap = 20
    bb = BranchAndBoundBatch.from_primal_batch(lp, node_cap=cap, trace_cap=PIV_CAP)
    roots = [("m%d" % k, lp.GetFinalTableau(k), bb.nvars[k]) for k in range(lp.Count)]
    assert bb.nvars[-1] == roots[-1][1].shape[1] - 1
    lp.destroy()  # the B&B batch does not depend on it
    bb.Run()
    check_batch(bb, roots, oracle, cap)
    a = bb.result_arrays()
    x = bb.solution_packed()
    at = 0
    for k, (obj, cons, mx) in enumerate(models):
        s = PrimalSimplexSolver(obj, cons, mx, engine=engine)
        s.Solve()
        xr, zr = BranchAndBoundAdapter.SolveFromPrimal(s, node_cap=cap, narrate=False)
        n = bb.nvars[k]
        assert bits(a["z"][k]) == bits(zr), k
        if xr:
            assert np.asarray(xr, dtype=np.float64).tobytes() == x[at:at + n].tobytes(), k
        else:
            assert not a["found"][k]
        at += n
    bb.destroy()


def test_solve_integer_programs_is_option3(engine):
    from lpr_381_group_v22_amd import (BranchAndBoundAdapter, PrimalSimplexSolver,
                                       solve_integer_programs)
    from lpr_381_group_v22_amd.program import _append_unit_bound_rows
    parsers = [_parser(obj, cons) for _, obj, cons in _models()]
    before = [len(p.Constraints) for p in parsers]
    got = solve_integer_programs(parsers, engine=engine)
    assert [len(p.Constraints) for p in parsers] == before  # the caller's parsers are untouched
    for p, (x, z) in zip(parsers, got):
        _append_unit_bound_rows(p)
        s = PrimalSimplexSolver(p.ObjectiveCoefficients, p.Constraints, engine=engine)
        s.Solve()
        xr, zr = BranchAndBoundAdapter.SolveFromPrimal(s, narrate=False)
        assert bits(z) == bits(zr) and np.asarray(x).tobytes() == np.asarray(xr).tobytes()


def test_lp_at_pivot_limit_is_refused(engine):
    from lpr_381_group_v22_amd import BranchAndBoundBatch, PrimalSimplexBatch, _native as N
    from lpr_381_group_v22_amd.bb_batch import option3_models
    parsers = [_parser(obj, cons) for _, obj, cons in _models()[:3]]
    lp = PrimalSimplexBatch(option3_models(parsers), engine=engine)
    lp.Solve(max_pivots=1)
    bad = [k for k in range(lp.Count) if lp.Status[k] == N.LPR_PIVOT_LIMIT]
    assert bad
    with pytest.raises(N.EngineError) as ei:
        BranchAndBoundBatch.from_primal_batch(lp)
    assert ei.value.status == N.LPR_BAD_ARGUMENT
    assert f"LP {bad[0]} " in N.lib.lpr_last_error().decode()
    lp.destroy()


# --------------------------------------------------------------------- 6. limits and errors
def test_max_child_pivots_ends_only_those_ips(engine, oracle):
    cap = 20
    roots = bb_roots(oracle) + big_roots(oracle)
    bb = make(engine, roots, cap)
    bb.Run(max_child_pivots=1)
    a = bb.result_arrays()
    limited = 0
    for k, (_, T, nv) in enumerate(roots):
        ref = oracle.bb_solve(T, nv, node_cap=cap, piv_cap=PIV_CAP)
        per = {}
        for node, phase, _, _ in ref["trace"]:
            if phase in (0, 1):
                per[node] = per.get(node, 0) + 1
        if any(v > 1 for v in per.values()):
            assert a["status"][k] == 5, k  # LPR_PIVOT_LIMIT
            limited += 1
        else:
            check_ip(bb, k, T, nv, oracle, cap, arrays=a, ref=ref)
    assert 0 < limited < len(roots)
    bb.destroy()


def test_bad_arguments(engine, oracle):
    from lpr_381_group_v22_amd import BranchAndBoundBatch, _native as N
    T = bb_roots(oracle)[0][1]
    r, c = T.shape

    def create(rows, cols, nv, cap, tab=T):
        h = C.c_void_p()
        R = np.asarray([rows], dtype=np.int32)
        Cc = np.asarray([cols], dtype=np.int32)
        n = np.asarray([nv], dtype=np.int32)
        t = np.ascontiguousarray(tab, dtype=np.float64).reshape(-1)
        st = N.lib.lpr_bb_batch_create(engine._h, 1, R.ctypes.data_as(C.POINTER(C.c_int32)),
                                       Cc.ctypes.data_as(C.POINTER(C.c_int32)),
                                       t.ctypes.data_as(C.POINTER(C.c_double)),
                                       n.ctypes.data_as(C.POINTER(C.c_int32)), cap, 0, C.byref(h))
        if h.value:
            N.lib.lpr_bb_batch_destroy(h)
        return st

    assert create(r, c, 6, 20) == N.LPR_OK_OPTIMAL
    assert create(r, c, 6, 65) == N.LPR_BAD_ARGUMENT           # node cap above 64
    assert create(r, c, c, 20) == N.LPR_BAD_ARGUMENT           # nvars > cols - 1
    assert create(r, c, -1, 20) == N.LPR_BAD_ARGUMENT
    wide = np.zeros((2, 2040))
    assert create(2, 2040, 1, 20, wide) == N.LPR_BAD_ARGUMENT  # beyond form H at full depth
    assert create(2, 2028, 1, 20, wide[:, :2028]) == N.LPR_OK_OPTIMAL
    bb = make(engine, bb_roots(oracle)[:1], 20)
    for kw in (dict(variant=4), dict(chunk=-1), dict(max_child_pivots=-1)):
        with pytest.raises(N.EngineError):
            bb.Run(**kw)
    cnt = C.c_int64()
    assert N.lib.lpr_bb_batch_trace_read(bb._h, 1, None, 0, C.byref(cnt)) == N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_bb_batch_run(bb._h, None, None) == N.LPR_BAD_ARGUMENT
    bb.destroy()
    with pytest.raises(ValueError):
        BranchAndBoundBatch.from_tableaux([np.zeros((2, 2040))], [1], engine=engine)


def test_orphaned_by_engine_close(oracle):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    eng = pkg.Engine(0)
    bb = make(eng, bb_roots(oracle)[:2], 20)
    eng.close()
    res = N.BBBatchResult()
    assert N.lib.lpr_bb_batch_run(bb._h, None, C.byref(res)) == N.LPR_BAD_ARGUMENT
    assert "orphaned" in N.lib.lpr_last_error().decode()
    assert N.lib.lpr_bb_batch_destroy(bb._h) == N.LPR_OK_OPTIMAL
    bb._h = None
