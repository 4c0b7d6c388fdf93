"""GPU tests of the seam items (tests/seam_cases.py) on the three oldest batch bodies and their
twins: k_batch_simplex / k_batch_simplex_trace, the revised batch and its
traced twin (17, 21), k_bb_batch / k_bb_batch_narr (13, 23).  One batch per engine holds all of
that engine's items; it runs in auto form, forced to every variant the items fit, shuffled, and
through the twin.  Every item is compared with the oracle run on it alone by the comparators of
the engine's own GPU tests (check_batch, check_lp, check_ip), and the planted pivot itself is
asserted with a message that names the seam: the C# takes the first of the tied candidates, and a
reduction that is wrong on one lane, wave, stride or window seam changes exactly that entry."""
import numpy as np
import pytest

import seam_cases as sc
import test_batch_gpu as tb
import test_bb_batch_gpu as tbb
import test_revised_batch_gpu as trb

pytestmark = pytest.mark.gpu


def seam_of(it, what):
    return (f"{it.name} [{what}]: {it.kind} at {it.at}, {it.label}: the tie at {it.planted} "
            f"must go to {it.winner}")


# ============================================================================== primal batch
def primal_batch(engine, its, trace_cap=0):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    return PrimalSimplexBatch.from_tableaux([it.T for it in its], [it.basis for it in its],
                                            engine=engine, log_cap=sc.PRIMAL_PIVOTS,
                                            trace_cap=trace_cap)


def primal_pivot(pair, it):
    row, col = int(pair[0]), int(pair[1])
    return col if it.kind == "entering" else row


def check_primal(b, its, refs, what):
    """The planted pivot first (its message names the seam), then everything as bytes."""
    for k, (it, ref) in enumerate(zip(its, refs)):
        assert it.at < ref["pivots"] <= sc.PRIMAL_PIVOTS, it.name
        assert primal_pivot(b.PivotLog(k)[it.at], it) == it.winner, seam_of(it, what)
    tb.check_batch(b, refs)


def primal_snapshot(b):
    return ([b.GetFinalTableau(k).tobytes() for k in range(b.Count)],
            [b.PivotLog(k).tobytes() for k in range(b.Count)], b.basis_packed().tobytes(),
            [s.tobytes() for s in b.status_arrays()], b.solution_packed().tobytes())


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_primal_seams_in_every_form(engine, oracle, variant):
    """Auto form, then forced: a W item forced to G or H meets its tie on another lane map."""
    its = sc.items("primal")
    refs = [sc.primal_ref(oracle, it) for it in its]
    b = primal_batch(engine, its)
    res = b.Solve(max_pivots=sc.PRIMAL_PIVOTS, variant=variant)
    assert res.optimal + res.unbounded + res.limit == len(its)
    check_primal(b, its, refs, f"variant {variant}")
    b.destroy()


def test_primal_seams_shuffled(engine, oracle):
    its = sc.items("primal")
    order = np.random.RandomState(12).permutation(len(its)).tolist()
    assert order != sorted(order)  # other neighbours, another slot within a W workgroup
    its = [its[q] for q in order]
    b = primal_batch(engine, its)
    b.Solve(max_pivots=sc.PRIMAL_PIVOTS)
    check_primal(b, its, [sc.primal_ref(oracle, it) for it in its], "shuffled")
    b.destroy()


def test_primal_seams_through_the_traced_twin(engine, oracle):
    its = sc.items("primal")
    refs = [sc.primal_ref(oracle, it) for it in its]
    plain = primal_batch(engine, its)
    plain.Solve(max_pivots=sc.PRIMAL_PIVOTS)
    cap = max(r["pivots"] for r in refs) + 1  # record 0 and one per pivot: nothing truncated
    b = primal_batch(engine, its, trace_cap=cap)
    b.Solve(max_pivots=sc.PRIMAL_PIVOTS)
    check_primal(b, its, refs, "traced")
    assert primal_snapshot(b) == primal_snapshot(plain)
    recs = b.trace_info()[0]
    for k, (it, ref) in enumerate(zip(its, refs)):
        assert recs[k] == ref["pivots"] + 1 <= cap, it.name
        row, col, T = b.Snapshot(k, it.at + 1)  # the record pivot number `at` made
        assert primal_pivot((row, col), it) == it.winner, seam_of(it, "traced record header")
        assert (row, col) == tuple(ref["log"][it.at]), it.name
        if it.at + 1 == ref["pivots"]:
            assert T.tobytes() == ref["T"].tobytes(), it.name
    plain.destroy()
    b.destroy()


# ============================================================================== revised batch
def revised_batch(engine, its, trace_cap=0):
    from lpr_381_group_v22_amd import RevisedSimplexBatch
    return RevisedSimplexBatch([it.model for it in its], engine=engine, log_cap=sc.REV_CAP,
                               trace_cap=trace_cap)


def revised_pivot(triple, it):
    return int(triple[1]) if it.kind == "enter_fold" else int(triple[0])


def check_revised(b, its, refs, what):
    for k, it in enumerate(its):
        assert revised_pivot(b.PivotLog(k)[it.at], it) == it.winner, seam_of(it, what)
    for k, ref in enumerate(refs):
        trb.check_lp(b, k, ref, what)


def fits_revised(it, variant):
    from lpr_381_group_v22_amd import revised_batch as rb
    want = {1: rb.FORM_W, 2: rb.FORM_G, 3: rb.FORM_H}[variant]
    return rb.pick_form(it.m, it.n, variant) == want


def test_revised_seams_in_auto_form(engine, oracle):
    its = sc.items("revised")
    b = revised_batch(engine, its)
    res = b.Solve(max_pivots=sc.REV_CAP)
    assert res.launches >= 3  # every form holds an item
    check_revised(b, its, [sc.revised_ref(oracle, it) for it in its], "auto")
    b.destroy()


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_revised_seams_forced_to_every_form_they_fit(engine, oracle, variant):
    its = [it for it in sc.items("revised") if fits_revised(it, variant)]
    assert its and (variant != 3 or len(its) == len(sc.items("revised")))
    b = revised_batch(engine, its)
    b.Solve(max_pivots=sc.REV_CAP, variant=variant)
    check_revised(b, its, [sc.revised_ref(oracle, it) for it in its], f"variant {variant}")
    b.destroy()


def test_revised_seams_shuffled(engine, oracle):
    its = sc.items("revised")
    order = np.random.RandomState(17).permutation(len(its)).tolist()
    assert order != sorted(order)
    its = [its[q] for q in order]
    b = revised_batch(engine, its)
    b.Solve(max_pivots=sc.REV_CAP)
    check_revised(b, its, [sc.revised_ref(oracle, it) for it in its], "shuffled")
    b.destroy()


def test_revised_seams_through_the_traced_twin(engine, oracle):
    its = sc.items("revised")
    refs = [sc.revised_ref(oracle, it) for it in its]
    plain = revised_batch(engine, its)
    plain.Solve(max_pivots=sc.REV_CAP)
    cap = max(r["iterations"] for r in refs) + 1  # one per iteration and "Optimal"
    b = revised_batch(engine, its, trace_cap=cap)
    b.Solve(max_pivots=sc.REV_CAP)
    check_revised(b, its, refs, "traced")
    assert trb.snapshot(b) == trb.snapshot(plain)
    for k, (it, ref) in enumerate(zip(its, refs)):
        assert b.SnapshotCount(k) <= cap, it.name
        snap = b.Snapshot(k, it.at)
        got = snap["entering"] if it.kind == "enter_fold" else snap["leaving_row"]
        assert got == it.winner, seam_of(it, "traced record header")
        row, enter, leave = ref["log"][it.at]
        assert (snap["leaving_row"], snap["entering"], snap["leaving_var"]) == (row, enter, leave)
    plain.destroy()
    b.destroy()


# ============================================================================== B&B batch
def bb_roots(its):
    return [(it.name, it.T, it.nv) for it in its]


def bb_log(bb, k):
    return dict(records=bb.Records(k), trace=bb.Trace(k))


def check_bb(bb, its, refs, oracle, what):
    for k, it in enumerate(its):
        assert sc.bb_observed(bb_log(bb, k), it) == sc.bb_expected(it), seam_of(it, what)
    tbb.check_batch(bb, bb_roots(its), oracle, sc.BB_CAP, refs=refs)


def test_bb_seams_in_auto_form(engine, oracle):
    its = sc.items("bb")
    refs = [sc.bb_ref(oracle, it) for it in its]
    assert {tbb.form_of(it.T, sc.BB_CAP) for it in its} == {0, 1, 2}
    bb = tbb.make(engine, bb_roots(its), sc.BB_CAP, trace_cap=64)
    res = bb.Run()
    assert res.pivot_limit == 0 and res.launches >= 3
    check_bb(bb, its, refs, oracle, "auto")
    bb.destroy()


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_bb_seams_forced_to_every_form_they_fit(engine, oracle, variant):
    lim = {1: tbb.W_MAX, 2: tbb.G_MAX, 3: None}[variant]
    its = [it for it in sc.items("bb")
           if lim is None or tbb.footprint_bytes(it.T, sc.BB_CAP) <= lim]
    assert its
    bb = tbb.make(engine, bb_roots(its), sc.BB_CAP, trace_cap=64)
    bb.Run(variant=variant)
    check_bb(bb, its, [sc.bb_ref(oracle, it) for it in its], oracle, f"variant {variant}")
    bb.destroy()


def test_bb_seams_shuffled(engine, oracle):
    its = sc.items("bb")
    order = np.random.RandomState(23).permutation(len(its)).tolist()
    its = [its[q] for q in order]
    bb = tbb.make(engine, bb_roots(its), sc.BB_CAP, trace_cap=64)
    bb.Run()
    check_bb(bb, its, [sc.bb_ref(oracle, it) for it in its], oracle, "shuffled")
    bb.destroy()


def test_bb_seams_through_the_narrated_twin(engine, oracle):
    its = sc.items("bb")
    refs = [sc.bb_ref(oracle, it) for it in its]
    plain = tbb.make(engine, bb_roots(its), sc.BB_CAP, trace_cap=64)
    plain.Run()
    bb = tbb.make(engine, bb_roots(its), sc.BB_CAP, trace_cap=64)
    bb.Narrate()  # the second pass reserves what the first one counted: nothing truncated
    info = bb.narration_info()
    assert np.array_equal(info.doubles_kept, info.doubles_made)
    check_bb(bb, its, refs, oracle, "narrated")
    a, p = bb.result_arrays(), plain.result_arrays()
    for key in a:
        assert a[key].tobytes() == p[key].tobytes(), key
    assert bb.solution_packed().tobytes() == plain.solution_packed().tobytes()
    for k, it in enumerate(its):
        assert bb.Records(k) == plain.Records(k) and bb.Trace(k) == plain.Trace(k), it.name
        c = sc.bb_child(it)
        pop = bb.PopInfo(k)[0]
        assert pop["id"] == 0 and pop["vals"] == c.vals, it.name
        if it.kind == "bv":  # the pop's decision values hold the tie, the record the winner
            dist = [abs((pop["vals"][i] - np.floor(pop["vals"][i])) - 0.5) for i in it.planted]
            assert len(set(dist)) == 1 and dist[0] in (0.0, 0.25), seam_of(it, "narrated pop")
            assert all(pop["vals"][i] % 1.0 != 0 for i in it.planted), it.name
            assert bb.Records(k)[1]["var"] == it.winner, seam_of(it, "narrated pop")
        # the lower child as AddConstraint leaves it (-0.0 is +0.0 on the device by then)
        assert np.array_equal(bb.ChildTableaux(k, 1)[0], np.array(c.child)), \
            seam_of(it, "narrated child tableau")
    plain.destroy()
    bb.destroy()
