"""GPU tests of the narrated Branch & Bound batch (lpr_bb_batch_narrate_*):
what the search kernel keeps for the console text of ExecuteBranchAndBound -- every tableau of
every child's DoDualSimplex list, the score of every pop, the incumbent's tableau -- against the
independent Python restatement (tests/ref_py_bb.py, tests/ref_py_bb_text.py), the CPU oracle and
the single-handle path (lpr_bb_node_info, lpr_bb_expand_traced, lpr_bb_node_read), through bytes;
the text against ExecuteNarrated; across forms, chunks, caps, pruning and node caps; and that
everything an un-narrated batch gives is unchanged."""
import ctypes as C

import numpy as np
import pytest

import bb_cases
from special_values import same
from test_bb_batch_gpu import (G_MAX, PIV_CAP, W_MAX, bb_roots, edge_roots, footprint_bytes,
                               form_of, make)

pytestmark = pytest.mark.gpu

CAP = 20
H_ROOT = "flag_over_bin3x120s1_nv126_md17"  # the smallest edge root that takes form H at cap 20


def same_tab(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and (a.tobytes() == b.tobytes() or
                                   all(same(x, y) for x, y in zip(a.ravel(), b.ravel())))


def last_error():
    from lpr_381_group_v22_amd import _native as N
    return (N.lib.lpr_last_error() or b"").decode(errors="replace")


_REF = {}


def ref_walk(name, T, nv, cap=CAP, pruning=False):
    """ExecuteNarrated of the restatement on this root: its result (text included) and, per
    record id, the list DoDualSimplex returned (None where it threw).  Computed once per case."""
    key = (name, cap, pruning)
    if key not in _REF:
        from ref_py_bb_text import NarratedBranchAndBound
        b = NarratedBranchAndBound(nv, cap)
        lists = [None]  # record 0 is the root
        inner = b.solver.DoDualSimplex

        def spy(adj):
            lists.append(None)
            tabs, opt = inner(adj)
            lists[-1] = [np.array(t, dtype=np.float64) for t in tabs]
            return tabs, opt

        b.solver.DoDualSimplex = spy
        res = b.ExecuteNarrated([[float(v) for v in row] for row in T], enable_pruning=pruning)
        _REF[key] = (res, lists)
    return _REF[key]


def lf(text):
    """print() ends lines with "\n" where Console.WriteLine writes Environment.NewLine."""
    from ref_py_text import CRLF
    return text.replace(CRLF, "\n")


def ref_text(res):
    return lf(res["text"])


def narrated(engine, roots, cap=CAP, pruning=False, **run_opts):
    bb = make(engine, roots, cap)
    bb.Narrate(enable_pruning=pruning, **run_opts)
    return bb


def slices(bb):
    """Per IP the kept doubles of its slice, from one read of the whole slab."""
    info, slab = bb.narration_info(), bb.narration_packed()
    return [slab[int(o):int(o) + int(n)].tobytes()
            for o, n in zip(info.offset, info.doubles_kept)]


@pytest.fixture(scope="module")
def batch(engine, oracle):
    roots = bb_roots(oracle)
    bb = narrated(engine, roots)
    yield bb, roots
    bb.destroy()


# ---------------------------------------------------------------------------------- 1. records
def test_child_tableaux_equal_the_restatement(batch):
    bb, roots = batch
    info = bb.narration_info()
    assert info.doubles_kept.tolist() == info.doubles_made.tolist()
    dropped = primal = 0
    for k, (name, T, nv) in enumerate(roots):
        res, lists = ref_walk(name, T, nv)
        recs = bb.Records(k)
        off, nt = bb.Children(k)
        assert len(recs) == len(lists) == len(nt), name
        assert nt[0] == 0 and off[0] == 0
        at = 0
        for rid in range(1, len(recs)):
            want = lists[rid] or []
            assert nt[rid] == len(want) and off[rid] == at, (name, rid)
            got = bb.ChildTableaux(k, rid)
            assert len(got) == len(want)
            for i, (g, w) in enumerate(zip(got, want)):
                assert same_tab(g, w), (name, rid, i)
                at += g.size
        assert info.tableaux[k] == sum(len(x or []) for x in lists), name
        assert info.doubles_made[k] == at, name
        tr = bb.Trace(k)
        dropped += sum(ph == 2 for _, ph, _, _ in tr)
        primal += sum(ph == 1 for _, ph, _, _ in tr)
    assert dropped > 0 and primal > 0  # the inputs reach the step back and the primal phase


def test_records_pops_and_incumbent_equal_the_single_path(batch, engine, oracle):
    from lpr_381_group_v22_amd import BranchBoundTree
    from lpr_381_group_v22_amd.branch_and_bound import gather_branch_and_bound_numbers
    bb, roots = batch
    for k, (name, T, nv) in enumerate(roots):
        tree = BranchBoundTree.from_array(engine, T, nv, max_depth=CAP)
        pops, tab, capped = gather_branch_and_bound_numbers(tree, T.shape, False, CAP)
        tree.destroy()
        got, gtab, gcapped = bb.NarrationNumbers(k)
        assert gcapped == capped and len(got) == len(pops), name
        for i, (g, w) in enumerate(zip(got, pops)):
            assert same(g.z, w.z) and same_tab(g.vals, w.vals), (name, i)
            assert (g.children is None) == (w.children is None), (name, i)
            for cg, cw in zip(g.children or [], w.children or []):
                assert cg.status == cw.status and cg.pivots == cw.pivots, (name, i)
                assert len(cg.tableaux) == len(cw.tableaux), (name, i)
                assert all(same_tab(a, b) for a, b in zip(cg.tableaux, cw.tableaux)), (name, i)
        assert (gtab is None) == (tab is None), name
        if tab is not None:
            assert same_tab(gtab, tab), name


def test_pop_scores_and_flags_equal_the_oracle(batch, oracle):
    """z and the decision values of every pop against orc_bb_node_info on the node the pop took
    (the root, or the last tableau of its record's list, rounded by :1124 / :1187), and the flags
    against the incumbent rule replayed on those."""
    bb, roots = batch
    for k, (name, T, nv) in enumerate(roots):
        best, found, best_tab = -np.inf, False, None
        for pop in bb.PopInfo(k):
            node = T if pop["id"] == 0 else oracle.bb_round_tableau(
                bb.ChildTableaux(k, pop["id"])[-1])
            rounded, z, vals = oracle.bb_node_info(node, nv)
            assert same(pop["z"], z) and same_tab(pop["vals"], vals), (name, pop)
            integer = all(oracle_is_integer(v) for v in vals)
            improves = integer and z > best
            assert pop["flags"] == 1 | (2 if integer else 0) | (4 if improves else 0), (name, pop)
            if improves:
                best, found, best_tab = z, True, rounded
        r = bb.Result(k)
        assert bool(r["found"]) == found and (not found or same(r["z"], best)), name
        tab = bb.IncumbentTableau(k)
        assert (tab is None) == (best_tab is None) and (tab is None or same_tab(tab, best_tab))


def oracle_is_integer(v):
    from ref_py_bb import round4, round_int
    r = round4(v)
    return abs(r - round_int(r)) <= 1e-6


# ------------------------------------------------------------------------------------- 2. text
def test_narration_text_equals_execute_narrated(batch):
    bb, roots = batch
    seen = ""
    for k, (name, T, nv) in enumerate(roots):
        res, _ = ref_walk(name, T, nv)
        assert "failed:" not in res["text"], name
        text = bb.NarrationText(k)
        assert lf(text) == ref_text(res), name
        seen += text
    for line in ("Infeasible tableau", "Potential infinite loop detected", "final tableau",
                 "pivot @ constraint"):
        assert line in seen, line


@pytest.mark.parametrize("name", ["binary_4v1c_s0", "frac_4v2c_s10", "binary_8v3c_s3",
                                  "binary_6v2c_s2"])
def test_narration_text_equals_solve_from_primal(engine, name, capsys):
    import lpr_381_group_v22_amd as pkg
    obj, cons = dict(bb_cases.all_bb_cases())[name]
    s = pkg.PrimalSimplexSolver(obj, [pkg.Constraint(list(c.Coefficients), c.Relation, c.RHS)
                                      for c in cons], True, engine=engine, snapshots="none")
    s.Solve()
    capsys.readouterr()
    x1, z1 = pkg.BranchAndBoundAdapter.SolveFromPrimal(s, narrate=True)
    want = capsys.readouterr().out
    bb = pkg.BranchAndBoundBatch.from_tableaux([s.FinalTableau], [len(s.SolutionVector)],
                                               trace_cap=PIV_CAP, engine=engine)
    bb.Narrate()
    assert bb.NarrationText(0) == want
    assert (bb.Solution(0).tolist() if bb.Result(0)["found"] else []) == x1
    bb.destroy()


# ------------------------------------------------------------------------------------ 3. forms
def _h_root(oracle):
    return [r for r in edge_roots(oracle, CAP) if r[0] == H_ROOT]


def test_form_h_by_size_equals_the_single_path(engine, oracle):
    from lpr_381_group_v22_amd import BranchBoundTree
    from lpr_381_group_v22_amd.branch_and_bound import (format_branch_and_bound,
                                                         gather_branch_and_bound_numbers)
    roots = _h_root(oracle)
    assert len(roots) == 1 and form_of(roots[0][1], CAP) == 2
    _, T, nv = roots[0]
    bb = narrated(engine, roots)
    tree = BranchBoundTree.from_array(engine, T, nv, max_depth=CAP)
    pops, tab, capped = gather_branch_and_bound_numbers(tree, T.shape, False, CAP)
    tree.destroy()
    got, gtab, gcapped = bb.NarrationNumbers(0)
    assert gcapped == capped and len(got) == len(pops)
    assert sum(len(c.tableaux) for p in got for c in p.children or []) > 0
    for g, w in zip(got, pops):
        assert same(g.z, w.z) and same_tab(g.vals, w.vals)
        for cg, cw in zip(g.children or [], w.children or []):
            assert cg.status == cw.status and cg.pivots == cw.pivots
            assert len(cg.tableaux) == len(cw.tableaux)
            assert all(same_tab(a, b) for a, b in zip(cg.tableaux, cw.tableaux))
    assert (gtab is None) == (tab is None) and (tab is None or same_tab(gtab, tab))
    assert bb.NarrationText(0) == format_branch_and_bound(nv, pops, tab, capped)[0]
    bb.destroy()


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_every_form_keeps_the_same_slab_and_text(batch, engine, oracle, variant):
    base, all_roots = batch
    lim = {1: W_MAX, 2: G_MAX, 3: None}[variant]
    pick = [k for k, r in enumerate(all_roots)
            if lim is None or footprint_bytes(r[1], CAP) <= lim]
    assert pick
    want = slices(base)
    bb = narrated(engine, [all_roots[k] for k in pick], variant=variant)
    got = slices(bb)
    for q, k in enumerate(pick):
        assert got[q] == want[k], all_roots[k][0]
        assert bb.NarrationText(q) == base.NarrationText(k), all_roots[k][0]
    bb.destroy()


# ----------------------------------------------------------------------------------- 4. resume
def test_chunk_one_and_a_second_run_give_the_same(batch, engine):
    base, roots = batch
    want, winfo = slices(base), base.narration_info()
    bb = make(engine, roots, CAP)
    bb.narrate_reserve(winfo.doubles_made)
    for run in (dict(chunk=1), dict()):
        bb.Run(**run)
        info = bb.narration_info()
        for a, b in zip(info, winfo):
            assert a.tolist() == b.tolist(), run
        assert slices(bb) == want, run
        for k in range(bb.Count):
            assert bb.PopInfo(k) == base.PopInfo(k), (run, k)
            t0, t1 = bb.IncumbentTableau(k), base.IncumbentTableau(k)
            assert (t0 is None) == (t1 is None) and (t0 is None or same_tab(t0, t1))
    bb.destroy()


# ------------------------------------------------------------------------------------- 5. caps
def test_caps_keep_a_prefix_and_exact_totals(batch, engine):
    from lpr_381_group_v22_amd import _native as N
    base, roots = batch
    want, winfo = slices(base), base.narration_info()
    need = winfo.doubles_made
    first = [(T.shape[0] + 1) * (T.shape[1] + 1) for _, T, _ in roots]  # a depth-1 tableau
    for label, caps in (("zero", [0] * len(roots)), ("one", first),
                        ("short", [max(int(n) - 1, 0) for n in need]), ("exact", need)):
        bb = make(engine, roots, CAP)
        bb.narrate_reserve(caps)
        bb.Run()
        info = bb.narration_info()
        assert info.tableaux.tolist() == winfo.tableaux.tolist(), label
        assert info.doubles_made.tolist() == need.tolist(), label
        got = slices(bb)
        for k in range(bb.Count):
            kept = int(info.doubles_kept[k])
            assert kept <= int(caps[k]) and got[k] == want[k][:8 * kept], (label, k)
            if label == "one" and need[k]:
                assert kept == first[k], (label, k)
            if label == "short" and need[k]:
                # everything but the last tableau, which is as deep as the last record
                last = bb.Records(k)[-1]["depth"]
                assert kept == need[k] - (roots[k][1].shape[0] + last) * (
                    roots[k][1].shape[1] + last), (label, k)
            if kept < need[k]:
                with pytest.raises(ValueError, match="would miss tableaux"):
                    bb.NarrationText(k)
                out = np.zeros(8)
                rc = N.lib.lpr_bb_batch_narrate_tableaux_read(
                    bb._h, k, kept, 1, out.ctypes.data_as(C.POINTER(C.c_double)))
                assert rc == N.LPR_BAD_ARGUMENT, (label, k)  # past what is kept: refused
            else:
                assert bb.NarrationText(k) == base.NarrationText(k), (label, k)
        bb.destroy()


def test_short_trace_raises(batch, engine):
    base, roots = batch
    bb = make(engine, roots, CAP, trace_cap=1)
    bb.Narrate()
    k = next(k for k in range(bb.Count) if bb.Result(k)["pivots"] > 1)
    with pytest.raises(ValueError, match="would miss pivots"):
        bb.NarrationText(k)
    bb.destroy()


def test_pivot_limit_raises_and_keeps_its_counts(batch, engine):
    base, roots = batch
    bb = make(engine, roots, CAP)
    bb.Narrate(max_child_pivots=1)
    a = bb.result_arrays()
    from lpr_381_group_v22_amd import _native as N
    hit = [k for k in range(bb.Count) if a["status"][k] == N.LPR_PIVOT_LIMIT]
    assert hit
    info, want = bb.narration_info(), slices(base)
    got = slices(bb)
    for k in hit:
        assert info.tableaux[k] > 0 and got[k] == want[k][:len(got[k])]
        with pytest.raises(ValueError, match="LPR_PIVOT_LIMIT"):
            bb.NarrationText(k)
    bb.destroy()


# ------------------------------------------------------------------ 6. pruning and node caps
@pytest.mark.parametrize("cap", [1, 20, 64])
@pytest.mark.parametrize("pruning", [False, True])
def test_pruning_and_node_caps(engine, oracle, cap, pruning):
    roots = bb_roots(oracle)[:4] + [r for r in bb_roots(oracle) if r[0] == "frac_4v2c_s10"]
    bb = narrated(engine, roots, cap=cap, pruning=pruning)
    pruned = 0
    for k, (name, T, nv) in enumerate(roots):
        res, lists = ref_walk(name, T, nv, cap, pruning)
        assert lf(bb.NarrationText(k)) == ref_text(res), (name, cap, pruning)
        assert bb.Result(k)["processed"] == res["processed"]
        pruned += sum(p["flags"] == 0 and p["vals"] is None for p in bb.PopInfo(k))
    if pruning and cap == 20:
        assert pruned > 0 and bb.Result(0)["processed"] == 5  # the sample model prunes
    if not pruning:
        assert pruned == 0
    bb.destroy()


# ------------------------------------------------------------------------- 7. unchanged batch
def test_a_narrated_batch_gives_the_bytes_of_an_unnarrated_one(batch, engine):
    from lpr_381_group_v22_amd import _native as N
    base, roots = batch
    u = make(engine, roots, CAP)
    u.Run()
    a, b = base.result_arrays(), u.result_arrays()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert base.solution_packed().tobytes() == u.solution_packed().tobytes()
    for k in range(u.Count):
        assert base.Records(k) == u.Records(k) or all(
            same(x[f], y[f]) for x, y in zip(base.Records(k), u.Records(k)) for f in x)
        assert base.PopOrder(k) == u.PopOrder(k) and base.Trace(k) == u.Trace(k)
    # an un-narrated handle refuses the narrate reads
    L, i64, dp, i32 = N.lib, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    n, out = C.c_int64(), np.zeros(64)
    r, c = C.c_int32(), C.c_int32()
    for rc in (L.lpr_bb_batch_narrate_info(u._h, None, None, None, None),
               L.lpr_bb_batch_narrate_pops_read(u._h, 0, None, None, None, 1, C.byref(n)),
               L.lpr_bb_batch_narrate_children_read(u._h, 0, None, None, 1, C.byref(n)),
               L.lpr_bb_batch_narrate_tableaux_read(u._h, 0, 0, 1, out.ctypes.data_as(dp)),
               L.lpr_bb_batch_narrate_read_all(u._h, out.ctypes.data_as(dp), 64),
               L.lpr_bb_batch_narrate_best_read(u._h, 0, None, C.byref(r), C.byref(c))):
        assert rc == N.LPR_BAD_ARGUMENT and "not narrated" in last_error()
    u.destroy()


def test_form_g_above_64_kib_unnarrated_then_narrated(engine, oracle):
    """One IP whose node cap of 64 puts its form-G footprint (85 768 bytes) above the 64 KiB a
    kernel gets without the dynamic-LDS attribute, first on an un-narrated handle, then on a
    narrated one: k_bb_batch<256, true> and k_bb_batch_narr<256, true> each need the attribute
    set for themselves.  Same bytes from both, and the restatement's text."""
    cap = 64
    roots = [r for r in bb_roots(oracle) if r[0] == "frac_4v2c_s10"]
    name, T, nv = roots[0]
    assert 64 * 1024 < footprint_bytes(T, cap) <= G_MAX
    u = make(engine, roots, cap)
    u.Run()
    n = narrated(engine, roots, cap=cap)
    a, b = u.result_arrays(), n.result_arrays()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert u.solution_packed().tobytes() == n.solution_packed().tobytes()
    assert u.PopOrder(0) == n.PopOrder(0) and u.Trace(0) == n.Trace(0)
    assert lf(n.NarrationText(0)) == ref_text(ref_walk(name, T, nv, cap)[0])
    u.destroy()
    n.destroy()


# ------------------------------------------------------------------------------- 8. option 3
def test_option3_texts_equal_the_files_option3_writes(engine, tmp_path):
    """option3_texts / write_option3_files on the sample model file and on the B&B cases as
    parsers against the file run_option(p, "3") writes for each model alone, timestamp masked."""
    import os
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd.program import run_option
    from ref_py_text import mask_timestamp
    from test_bb_batch_gpu import _models, _parser
    sample = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "TextFile.txt")

    def parsers():
        p = pkg.InputFileParser()
        p.ReadInputFile(sample)
        return [p] + [_parser(obj, cons) for _, obj, cons in _models()[:6]]

    mine = parsers()
    before = [len(p.Constraints) for p in mine]
    paths = [str(tmp_path / ("batch_%d.txt" % k)) for k in range(len(mine))]
    got = pkg.write_option3_files(mine, paths, engine=engine)
    assert [len(p.Constraints) for p in mine] == before  # the caller's parsers are untouched
    for k, p in enumerate(parsers()):
        one = str(tmp_path / ("single_%d.txt" % k))
        r = run_option(p, "3", one, engine=engine)
        want, have = open(one, "rb").read(), open(paths[k], "rb").read()
        assert mask_timestamp(have) == mask_timestamp(want), k
        assert got[k][0] == r["x"] and same(got[k][1], r["z"]), k
    assert b"Total branchs processed: 20" in open(paths[0], "rb").read()


# --------------------------------------------------------------------------- 9. bad arguments
def test_bad_arguments_and_engine_closed_under_a_narrated_handle(oracle):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    eng = pkg.Engine(0)
    roots = bb_roots(oracle)[:2]
    bb = make(eng, roots, CAP)
    L, i64, dp = N.lib, C.POINTER(C.c_int64), C.POINTER(C.c_double)

    def refused(rc, what):
        assert rc == N.LPR_BAD_ARGUMENT and what in last_error(), (rc, last_error())

    refused(L.lpr_bb_batch_narrate_reserve(bb._h, None), "null cap_doubles")
    caps = np.asarray([4, -1], dtype=np.int64)
    refused(L.lpr_bb_batch_narrate_reserve(bb._h, caps.ctypes.data_as(i64)), "cap_doubles[1] = -1")
    refused(L.lpr_bb_batch_narrate_info(bb._h, None, None, None, None), "not narrated")
    huge = np.asarray([1 << 45, 1 << 45], dtype=np.int64)
    assert L.lpr_bb_batch_narrate_reserve(bb._h, huge.ctypes.data_as(i64)) == N.LPR_OUT_OF_MEMORY
    assert "narration slab" in last_error()
    refused(L.lpr_bb_batch_narrate_info(bb._h, None, None, None, None), "not narrated")
    bb.Run()  # still usable, un-narrated
    bb.Narrate()
    assert L.lpr_bb_batch_narrate_info(bb._h, None, None, None, None) == 0
    out, n = np.zeros(8), C.c_int64()
    kept = int(bb.narration_info().doubles_kept[0])
    refused(L.lpr_bb_batch_narrate_tableaux_read(bb._h, 0, kept, 1, out.ctypes.data_as(dp)),
            f"keeps {kept}")
    refused(L.lpr_bb_batch_narrate_tableaux_read(bb._h, 2, 0, 1, out.ctypes.data_as(dp)),
            "IP 2 out of range")
    refused(L.lpr_bb_batch_narrate_tableaux_read(bb._h, 0, 0, 1, None), "null output")
    refused(L.lpr_bb_batch_narrate_read_all(bb._h, out.ctypes.data_as(dp), 1), "cap_doubles 1")
    refused(L.lpr_bb_batch_narrate_pops_read(bb._h, 0, None, None, None, -1, C.byref(n)), "cap -1")
    k = next((k for k in range(bb.Count) if not bb.Result(k)["found"]), None)
    if k is not None:
        refused(L.lpr_bb_batch_narrate_best_read(bb._h, k, None, None, None), "no incumbent")
    text = bb.NarrationText(0)
    assert text.startswith("Initiating Branch and Bound Algorithm\n")
    eng.close()
    refused(L.lpr_bb_batch_narrate_reserve(bb._h, caps.ctypes.data_as(i64)), "orphaned")
    refused(L.lpr_bb_batch_narrate_info(bb._h, None, None, None, None), "orphaned")
    refused(L.lpr_bb_batch_narrate_read_all(bb._h, out.ctypes.data_as(dp), 8), "orphaned")
    bb.destroy()
