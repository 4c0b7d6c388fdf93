"""GPU parity tests on non-finite and extreme-magnitude data (tests/special_values.py): the primal
paths (batch forms, every single-tableau path, inside a block of 16), the revised solver, Branch
& Bound (single engine, batch, rounding helpers), cut / dual / primal2 and the sensitivity edits
(single engine, scenario batch) against the CPU oracle on data that holds +-inf, NaN, -0.0,
subnormals, +-1e308, DBL_MAX and 1e-9 +- 1 ulp.  Integers (status, pivot counts, logs,
bases, node records) are compared exactly; doubles with the comparator of DESIGN.md section 2 (NaN
positions identical, every other element identical in all 64 bits).  That the oracle is the truth
on these cases, and that the cases reach the branches they are meant for, is established on the
CPU in test_special_values_cpu.py."""
import numpy as np
import pytest

import special_values as sv

pytestmark = pytest.mark.gpu

SEQ, OV, INPLACE, OV2 = 0x4008, 0x5008, 0x6008, 0x3008
SPREAD, MEMSIDE = 0x20000, 0x40000
SMALL = 0x2000
# (variant, block): the one-pivot paths (two kernels / fused), the K-pivot forms, the
# cache-resident small path
PATHS = [(0x7fff, 1), (0x7ffe, 1), (SEQ, 4), (SEQ, 16), (OV, 4), (OV, 16), (OV2, 4), (OV2, 16),
         (INPLACE, 4), (INPLACE, 16), (SMALL, 0)]
PATH_IDS = ["two-kernel", "fused", "seq4", "seq16", "ov4", "ov16", "ov2-4", "ov2-16", "inplace4",
            "inplace16", "small"]


# ------------------------------------------------------------------------------ primal helpers
def _oracle_legs(oracle, T0, b0, legs):
    """[(status, pivots, log, basis, T, x, z)] after each leg, on copies."""
    T = np.ascontiguousarray(T0, dtype=np.float64).copy()
    basis = np.ascontiguousarray(b0, dtype=np.int32).copy()
    n = T.shape[1] - T.shape[0]
    out = []
    for leg in legs:
        st, piv, log = oracle.primal_solve(T, basis, leg)
        x, z = oracle.extract_solution(T, max(n, 0))
        out.append((st, piv, log.tolist(), basis.tolist(), T.copy(), x, z))
        if st != 5:
            break
    return out


def _run_legs(engine, T0, b0, states, legs, variant, block, tag, want_block=None):
    from lpr_381_group_v22_amd import Tableau
    tab = Tableau.from_array(engine, T0, b0)
    n = T0.shape[1] - T0.shape[0]
    total = 0
    for leg, (st, piv, log, basis, T, x, z) in zip(legs, states):
        res = tab.solve(max_pivots=leg, block=block, variant=variant)
        total += piv
        t = (tag, leg, hex(variant), block)
        if want_block is not None:
            assert res.block == want_block, t
        assert res.status == st and res.pivots == piv and res.total_pivots == total, \
            (t, res.status, st, res.pivots, piv)
        assert tab.pivot_log(1 << 12).tolist()[total - piv:] == log, t
        assert tab.basis().tolist() == basis, t
        sv.assert_same(tab.read(), T, t)
        sv.assert_same(res.z, T[0, -1], t)
        if n > 0 and x is not None:
            gx, gz = tab.extract_solution(n)
            sv.assert_same(gx, x, t)
            sv.assert_same(gz, z, t)
    tab.destroy()


@pytest.fixture(scope="module")
def fuzz_cases():
    return sv.primal_fuzz()


@pytest.fixture(scope="module")
def fuzz_refs(oracle, fuzz_cases):
    return [sv.oracle_primal(oracle, T, b, T.shape[1] - T.shape[0]) for T, b, _ in fuzz_cases]


ONE_CALL = (sv.FUZZ_CAP,)
CUT_LEGS = (1, 2, 3, sv.FUZZ_CAP)   # block 4 is cut after 1 and 3 of its pivots, block 16 by all


@pytest.fixture(scope="module")
def subset(oracle, fuzz_cases, fuzz_refs):
    """About 40 fuzz cases for the single-tableau paths: the first 28 that make three or more
    pivots (so that legs can cut a block of 4) and the first four each that end after 0, 1 and 2
    pivots (a NaN ratio in every row, an immediate unbounded exit), with the oracle's states
    after ONE_CALL and after CUT_LEGS."""
    out = []
    room = {0: 4, 1: 4, 2: 4, 3: 28}
    for k, ((T, b, _), ref) in enumerate(zip(fuzz_cases, fuzz_refs)):
        kind = min(int(ref["pivots"]), 3)
        if room[kind] > 0:
            room[kind] -= 1
            out.append((k, T, b, _oracle_legs(oracle, T, b, ONE_CALL),
                        _oracle_legs(oracle, T, b, CUT_LEGS)))
    assert len(out) == 40
    finals = np.concatenate([one[-1][4].reshape(-1) for _, _, _, one, _ in out])
    assert sv.has_nan(finals) and sv.has_inf(finals)
    assert {0, 1} <= {one[-1][0] for _, _, _, one, _ in out}
    return out


# ------------------------------------------------------------------------------ primal, small fuzz
@pytest.mark.parametrize("variant", [1, 2, 3], ids=["W", "G", "H"])
def test_small_fuzz_batch_forms(engine, fuzz_cases, fuzz_refs, variant):
    """All fuzz tableaux in one PrimalSimplexBatch.from_tableaux call per form."""
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    b = PrimalSimplexBatch.from_tableaux([T for T, _, _ in fuzz_cases],
                                         [bs for _, bs, _ in fuzz_cases], engine=engine,
                                         log_cap=sv.FUZZ_CAP)
    b.Solve(max_pivots=sv.FUZZ_CAP, variant=variant)
    st, piv, z = b.status_arrays()
    x = b.solution_packed()
    at = 0
    for k, ref in enumerate(fuzz_refs):
        assert st[k] == ref["status"] and piv[k] == ref["pivots"], (k, st[k], ref["status"])
        assert b.PivotLog(k).tolist() == ref["log"].tolist(), k
        assert b.BasicVariables(k) == ref["basis"].tolist(), k
        sv.assert_same(b.GetFinalTableau(k), ref["T"], k)
        sv.assert_same(z[k], ref["T"][0, -1], k)
        n = b.Shape(k)[2]
        if ref["status"] == 0:
            sv.assert_same(x[at:at + n], ref["x"], k)
        else:
            sv.assert_same(x[at:at + n], np.zeros(n), k)
        at += n
    b.destroy()


@pytest.mark.parametrize("variant,block", PATHS, ids=PATH_IDS)
def test_small_fuzz_subset_single_paths(engine, subset, variant, block):
    """Each subset case once in a single call, then in legs that cut a block in the middle, the
    state compared after every leg."""
    want = 16 if variant == SMALL else block
    for k, T, b, one, legs in subset:
        _run_legs(engine, T, b, one, ONE_CALL, variant, block, k, want)
        _run_legs(engine, T, b, legs, CUT_LEGS, variant, block, k, want)


# ------------------------------------------------------------------------------ primal, constructed
@pytest.fixture(scope="module")
def constructed(oracle):
    out = []
    for name, (T, b, n) in sv.constructed_primal().items():
        out.append((name, T, b, _oracle_legs(oracle, T, b, (16,)),
                    _oracle_legs(oracle, T, b, (1, 1, 16))))
    return out


@pytest.mark.parametrize("variant,block", PATHS, ids=PATH_IDS)
def test_constructed_primal_single_paths(engine, constructed, variant, block):
    for name, T, b, one, legs in constructed:
        _run_legs(engine, T, b, one, (16,), variant, block, name)
        _run_legs(engine, T, b, legs, (1, 1, 16), variant, block, name)


@pytest.mark.parametrize("variant", [1, 2, 3], ids=["W", "G", "H"])
def test_constructed_primal_batch_forms(engine, constructed, variant):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    b = PrimalSimplexBatch.from_tableaux([T for _, T, _, _, _ in constructed],
                                         [bs for _, _, bs, _, _ in constructed], engine=engine)
    b.Solve(max_pivots=16, variant=variant)
    st, piv, z = b.status_arrays()
    x = b.solution_packed()
    at = 0
    for k, (name, _, _, one, _) in enumerate(constructed):
        rst, rpiv, rlog, rbasis, rT, rx, rz = one[-1]
        assert st[k] == rst and piv[k] == rpiv, name
        assert b.PivotLog(k).tolist() == rlog and b.BasicVariables(k) == rbasis, name
        sv.assert_same(b.GetFinalTableau(k), rT, name)
        n = b.Shape(k)[2]
        sv.assert_same(x[at:at + n], rx if rst == 0 else np.zeros(n), name)
        at += n
    b.destroy()


# ------------------------------------------------------------------------------ primal, in a block
IN_BLOCK_VARIANTS = [OV2, OV2 | SPREAD, OV2 | MEMSIDE, SEQ, INPLACE]
IN_BLOCK_ONE = (sv.IN_BLOCK_CAP,)
IN_BLOCK_LEGS = (16, 23, 9, 17)   # ov_step_cases.LEGS: limits fall inside a block


@pytest.mark.parametrize("variant", IN_BLOCK_VARIANTS,
                         ids=["ov2", "ov2-spread", "ov2-memside", "seq", "inplace"])
@pytest.mark.parametrize("value", sv.IN_BLOCK_VALUES, ids=["inf", "nan", "1e308"])
@pytest.mark.parametrize("m,n", sv.IN_BLOCK_SHAPES)
def test_value_inside_a_block_of_16(engine, oracle, m, n, value, variant):
    """One inf / NaN / 1e308 that becomes a pivot-row or pivot-column entry at a pivot that is not
    the first of its block of 16, in a row >= 64 and the last column strip: the arithmetic happens
    in the heads' chains through the staged pivots and in a tile's recomputed pivot rows."""
    for legs in (IN_BLOCK_ONE, IN_BLOCK_LEGS):
        T0, b0, states = sv.in_block_reference(oracle, m, n, value, legs)
        _run_legs(engine, T0, b0, [(st, piv, log, basis, T, None, None)
                                   for st, piv, log, basis, T in states],
                  legs, variant, 16, (m, n, value), 16)


# ------------------------------------------------------------------------------ revised
REV_IDS = [k[0] for k in sv.revised_cases()]


@pytest.mark.parametrize("name,c,A,b", sv.revised_cases(), ids=REV_IDS)
def test_revised_batched_solve(engine, oracle, name, c, A, b):
    """lpr_revised_solve on (c, A, b) with planted values: status, iterations, log, basis, B^-1,
    x_B, and x / Z on the optimal exit."""
    from lpr_381_group_v22_amd import RevisedState
    ref = oracle.revised_solve(c, A, b, False, max_iter=sv.REVISED_CAP)
    st = RevisedState.create(engine, c, A, b, False)
    res = st.solve(max_pivots=sv.REVISED_CAP)
    assert res.status == ref["status"] and res.iterations == ref["iterations"], \
        (res.status, ref["status"], res.iterations, ref["iterations"])
    assert st.log().tolist() == ref["log"].tolist()
    assert st.basis().tolist() == ref["basis"].tolist()
    sv.assert_same(st.binv(), ref["Binv"], "Binv")
    sv.assert_same(st.xb(), ref["xB"], "xB")
    if ref["status"] == 0:
        x, z = st.solution()
        sv.assert_same(x, ref["x"], "x")
        sv.assert_same(z, ref["z"], "z")
        sv.assert_same(res.z, ref["z"], "res.z")
    st.destroy()


@pytest.mark.parametrize("name,c,A,b", sv.revised_cases(), ids=REV_IDS)
def test_revised_steps_with_snapshots(engine, oracle, name, c, A, b):
    """One lpr_revised_step per iteration against the oracle's CaptureSnapshot trace: y, reduced
    costs, direction, ratios, x_B, B^-1 A in the C#'s own order and B^-1 after every step."""
    from lpr_381_group_v22_amd import RevisedState
    m, n = A.shape
    tr = oracle.revised_trace(c, A, b, False, max_iter=sv.REVISED_CAP, cap=sv.REVISED_CAP + 2)
    st = RevisedState.create(engine, c, A, b, False)
    got, status = 0, 5
    while got < sv.REVISED_CAP:
        info = st.step()
        status = info.status
        if status not in (0, 5):
            break
        a = tr["snapshots"][got]
        y, rc, u, ratios, bpre, xb = st.snapshot()
        assert info.entering == a["entering"], got
        sv.assert_same(info.z_working, a["z_working"], (got, "z_working"))
        sv.assert_same(info.z_original, a["z_original"], (got, "z_original"))
        sv.assert_same(y, a["y"], (got, "y"))
        sv.assert_same(xb, a["xB"], (got, "xB"))
        sv.assert_same(rc[:n], a["rcX"], (got, "rcX"))
        sv.assert_same(rc[n:], a["rcS"], (got, "rcS"))
        assert st.basis().tolist() == a["basis_post"].tolist(), got
        sv.assert_same(st.binv_a_exact(), a["BInvA"], (got, "BInvA"))
        sv.assert_same(st.binv(), a["BInv"], (got, "BInv"))
        if status == 5:
            assert (info.leaving_row, info.leaving_var) == (a["leaving_row"], a["leaving_var"])
            sv.assert_same(info.entering_rc_pre, a["rc_pre"], (got, "rc_pre"))
            sv.assert_same(u, a["u_pre"], (got, "u"))
            sv.assert_same(ratios, a["ratios_pre"], (got, "ratios"))
            assert bpre.tolist() == a["basis_pre"].tolist(), got
        got += 1
        if status == 0:
            break
    assert got == tr["count"]
    if got < sv.REVISED_CAP:
        assert status == tr["status"]
    st.destroy()


# ------------------------------------------------------------------------------ B&B rounding
def test_bb_rounding_helpers_on_the_value_classes(engine, oracle):
    """The device's Math.Round(x, 4) (RoundTableau at node creation) and the node scoring on an
    array that holds every value class, through lpr_bb_create / lpr_bb_node_info / node_read as
    test_bb_edges_gpu.py::test_rows_plus_depth_limit uses them."""
    from lpr_381_group_v22_amd import BranchBoundTree
    T = sv.rounding_tableau()
    want_T, want_z, want_v = oracle.bb_node_info(T, 2)
    tree = BranchBoundTree.from_array(engine, T, 2, max_depth=4)
    z, vals = tree.node_info([0])
    root = tree.node_read(0)
    tree.destroy()
    sv.assert_same(root, want_T, "rounded root")
    sv.assert_same(z[0], want_z, "z")
    sv.assert_same(vals[0], want_v, "decision values")


# ------------------------------------------------------------------------------ Branch & Bound
def _same_bb(ref, status, found, z, x, processed, best_node, records, pop_order, trace, tag):
    assert status == ref["status"] and processed == ref["processed"], tag
    assert pop_order == ref["pop_order"], tag
    assert sv.same_records(records, ref["records"]), tag
    assert trace == ref["trace"], tag
    assert bool(found) == ref["found"], tag
    sv.assert_same(z, ref["z"], tag)
    if ref["found"]:
        sv.assert_same(x, ref["x"], tag)
        assert best_node == ref["best_node"], tag


@pytest.fixture(scope="module")
def bb_cases_refs(oracle):
    cases = sv.bb_device_cases(oracle)
    assert any(c[3] for c in cases) and any(c[4] for c in cases)   # pivot-row and factor hits
    return [(c, oracle.bb_solve(c[1], c[2], node_cap=sv.BB_NODE_CAP, piv_cap=1 << 16))
            for c in cases]


def test_bb_single_engine_from_planted_start_tableaux(engine, bb_cases_refs):
    """lpr_bb_run node by node against oracle.bb_solve from start tableaux with one planted
    +-inf, NaN or 1e308: cases whose trace holds a pivot with a non-finite normalised pivot row
    beside zero factors (the `nonfinite` vote of k_bb_select), cases with a non-finite factor."""
    from lpr_381_group_v22_amd import BranchBoundTree
    for (name, T, n, _, _), ref in bb_cases_refs:
        tree = BranchBoundTree.from_array(engine, T, n, max_depth=20)
        res, x = tree.run(enable_pruning=False, node_cap=sv.BB_NODE_CAP)
        records, pop, trace = tree.records(), tree.pop_order(), tree.trace()
        tree.destroy()
        _same_bb(ref, res.status, res.found, res.z, x, res.processed, res.best_node, records, pop,
                 trace, name)


@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=["auto", "W", "G", "H"])
def test_bb_batch_from_planted_start_tableaux(engine, bb_cases_refs, variant):
    from lpr_381_group_v22_amd import BranchAndBoundBatch
    bb = BranchAndBoundBatch.from_tableaux([c[1] for c, _ in bb_cases_refs],
                                           [c[2] for c, _ in bb_cases_refs],
                                           node_cap=sv.BB_NODE_CAP, trace_cap=1 << 16,
                                           engine=engine)
    bb.Run(variant=variant)
    a = bb.result_arrays()
    x = bb.solution_packed()
    at = 0
    for k, ((name, T, n, _, _), ref) in enumerate(bb_cases_refs):
        _same_bb(ref, a["status"][k], a["found"][k], a["z"][k], x[at:at + n], a["processed"][k],
                 a["best_node"][k], bb.Records(k), bb.PopOrder(k), bb.Trace(k), (name, variant))
        assert a["pivots"][k] == len(ref["trace"]), name
        at += n
    bb.destroy()


# ------------------------------------------------------------------------------ cut, dual, primal2
DUAL_STATUS = {0: 0, 1: 2, 3: 3, 5: 5}    # oracle rc -> lpr_status, as in test_cut_gpu.py
PRIM_STATUS = {0: 0, 1: 1, 3: 3, 5: 5}


@pytest.fixture(scope="module")
def cut_planted(oracle):
    return sv.cut_planted(oracle)


def test_dual_solve_on_planted_tableaux(engine, oracle, cut_planted):
    from lpr_381_group_v22_amd import Tableau
    for name, T0 in cut_planted["dual"]:
        T = T0.copy()
        rc, piv, log = oracle.dual_solve(T, print_steps=True, hard_cap=sv.CUT_HARD_CAP)
        tab = Tableau.from_array(engine, T0)
        res = tab.dual_solve(print_steps=True, hard_cap=sv.CUT_HARD_CAP)
        assert res.status == DUAL_STATUS[rc] and res.pivots == piv, (name, res.status, rc)
        assert tab.cut_log() == log, name
        sv.assert_same(tab.read(), T, name)
        tab.destroy()


def test_primal2_solve_on_planted_tableaux(engine, oracle, cut_planted):
    """A NaN factor updates its row in PrimalSimplexSolver2's pivot (`|f| <= EPS` skips, :160),
    unlike in DualSimplex's (`|f| > EPS` updates, :166): found by these cases."""
    from lpr_381_group_v22_amd import Tableau
    for name, T0 in cut_planted["primal2"]:
        T = T0.copy()
        rc, piv, log = oracle.primal2_solve(T, print_steps=False, hard_cap=sv.CUT_HARD_CAP)
        tab = Tableau.from_array(engine, T0)
        res = tab.primal2_solve(print_steps=False, hard_cap=sv.CUT_HARD_CAP)
        assert res.status == PRIM_STATUS[rc] and res.pivots == piv, (name, res.status, rc)
        assert tab.cut_log() == log, name
        sv.assert_same(tab.read(), T, name)
        sv.assert_same(res.z, T[0, -1], name)
        tab.destroy()


def test_cutting_plane_on_planted_tableaux(engine, oracle, cut_planted):
    from lpr_381_group_v22_amd import Tableau
    for name, T0 in cut_planted["cut"]:
        rc, cuts, T, log = oracle.cutting_plane(T0, max_cuts=4, hard_cap=sv.CUT_HARD_CAP)
        tab = Tableau.from_array(engine, T0)
        ex, ncuts = tab.cutting_plane(max_cuts=4, hard_cap=sv.CUT_HARD_CAP)
        assert (ex, ncuts) == (rc, cuts), (name, ex, ncuts, rc, cuts)
        assert tab.cut_log() == log, name
        sv.assert_same(tab.read(), T, name)
        tab.destroy()


# ------------------------------------------------------------------------------ sensitivity
def _same_sens_state(T, basic, sol, z, log, orc, skip, tag):
    st = orc.state()
    sv.assert_same(T, st["T"], tag)
    assert list(basic) == st["basic"], tag
    sv.assert_same(sol, st["sol"], tag)
    sv.assert_same(z, st["z"], tag)
    assert log == orc.log()[skip:], tag


@pytest.fixture(scope="module")
def sens_scripts(oracle):
    return sv.sens_scripts(oracle)


def test_sens_single_engine_special_edit_arguments(engine, oracle, sens_scripts):
    """Every edit kind with inf, NaN, +-1e308, -0.0 or 5e-324 as its argument, and one start
    tableau with a planted inf: outcome and the whole state after every edit."""
    from lpr_381_group_v22_amd.engine import SensState
    for name, (T, x, z, basis), ops in sens_scripts:
        o = oracle.sens(T, x, z, basis)
        d = SensState.create(engine, T, x, z)
        for k, (op, args) in enumerate(ops):
            rc = getattr(o, op)(*args)
            got = getattr(d, op)(*args)
            assert got == rc, (name, k, op, got, rc)
            dT, dbasic, dsol = d.read()
            _same_sens_state(dT, dbasic.tolist(), dsol, d.shape()[4], d.log(), o, 0, (name, k, op))
        d.destroy()


def test_sens_scenario_batch_special_edit_arguments(engine, oracle, sens_scripts):
    """The same scripts as scenarios of one batch per base (lpr_sens_batch_create_grow)."""
    import sens_batch_cases
    from lpr_381_group_v22_amd import SensitivityGrowBatch
    from lpr_381_group_v22_amd.engine import SensState
    groups = {}
    for name, base, ops in sens_scripts:
        groups.setdefault(id(base[0]), (base, []))[1].append((name, ops))
    assert len(groups) == 3
    for base, items in groups.values():
        T, x, z, _ = base
        d = SensState.create(engine, T, x, z)
        b = SensitivityGrowBatch(d, [ops for _, ops in items])
        d.destroy()
        res = b.Run()
        assert res.finished == len(items) and res.running == 0
        for k, (name, ops) in enumerate(items):
            o, outs, pivs, skip = sens_batch_cases.oracle_run(oracle, base, ops)
            assert b.Outcomes(k) == outs and b.Pivots(k) == pivs, (name, b.Outcomes(k), outs)
            assert b.LogCount(k) == len(o.log()) - skip, name
            got = b.State(k)
            _same_sens_state(got["T"], got["basic"], got["sol"], got["z"], b.Log(k), o, skip, name)
        b.destroy()
