"""GPU tests of the narrated cutting-plane batch (lpr_cut_batch_narrate_*):
the events, every data block and the console text of every item against the text restatement
(tests/ref_py_cut_text.py, checked against the oracle in test_cut_batch_narr_cpu.py), while code,
cuts, log and tableau stay those of the un-narrated batch."""
import numpy as np
import pytest

import cut_batch_cases as cb
import cut_cases
import ref_py_cut_text as rt
import special_values as sv
from ref_py_text import CRLF

pytestmark = pytest.mark.gpu

TEXTBOOK_MAX_CUTS = 20


def lf(text):
    return text.replace(CRLF, "\n")


def ref_data(n):
    """The restatement's block 0 and blocks as the flat doubles a narrated item keeps."""
    return np.concatenate([np.asarray(n.record0, dtype=np.float64).reshape(-1)] +
                          [np.asarray(b, dtype=np.float64).reshape(-1) for b in n.blocks])


def two_pass(engine, tabs, max_cuts, from_batch=None, **run):
    """A counting handle with caps 0, then a keeping handle with exactly what was made."""
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    make = from_batch or (lambda: CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=max_cuts))
    count = make()
    count.narrate_reserve(0, 1)
    count.Run(**run)
    need = count.narration_info()
    assert not need.doubles_kept.any()
    count.destroy()
    keep = make()
    keep.narrate_reserve(need.doubles_made, int(need.events_made.max()))
    res = keep.Run(**run)
    return keep, need, res


def check_numbers(batch, k, n, what="", nan=False):
    """Item k's events and every block against the restatement `n`."""
    info = batch.narration_info()
    want = ref_data(n)
    assert int(info.events_made[k]) == len(n.events), what
    assert batch.Events(k) == n.events, what
    assert int(info.doubles_made[k]) == int(info.doubles_kept[k]) == want.size, what
    got = batch.NarrationData(k, 0, want.size)
    if nan:
        sv.assert_same(got, want, what)
    else:
        assert got.tobytes() == want.tobytes(), what
    rec0, blocks = batch.NarrationBlocks(k)
    assert rec0.shape == np.asarray(n.record0).shape and len(blocks) == len(n.blocks), what
    for b, r in zip(blocks, n.blocks):
        assert b.shape == np.asarray(r).shape, what


# ------------------------------------------------------------------ 1. text of every uncapped exit
@pytest.fixture(scope="module")
def textbook(oracle):
    return cb.textbook_items(oracle)


@pytest.fixture(scope="module")
def textbook_refs(oracle, textbook):
    """Per item: (the restatement, its code, its cuts, the oracle's reference).  Made once."""
    out = []
    for name, T in textbook:
        n, code, cuts = rt.narrate_cutting_plane(T, TEXTBOOK_MAX_CUTS)
        out.append((n, code, cuts, cb.reference(oracle, cb.MODE_CUT, T,
                                                max_cuts=TEXTBOOK_MAX_CUTS)))
    return out


@pytest.mark.parametrize("variant", [0, 2, 3])
def test_text_of_every_uncapped_exit(engine, textbook, textbook_refs, variant):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    names = [n for n, _ in textbook]
    tabs = [T for _, T in textbook]
    # the fixtures still reach what this test is about: checked on the reference itself
    assert len(tabs) == 12
    assert {code for _, code, _, _ in textbook_refs} == {0, 1, 2, 4, 5}
    assert sum(code == 4 for _, code, _, _ in textbook_refs) == 6
    by = dict(zip(names, textbook_refs))
    huge = by["huge_relaxation_value"]
    assert huge[1] == 5 and [sum(1 for e in huge[0].events if e[0] == rt.EV_PIVOT + q)
                             for q in (0, 1)] == [9, 2]
    assert by["binary_10v2c_s4"][1:3] == (0, 6)
    assert not any(n.stopped for n, _, _, _ in textbook_refs)

    batch, need, res = two_pass(engine, tabs, TEXTBOOK_MAX_CUTS, variant=variant)
    assert (res.items_g, res.items_h) == ((0, 12) if variant == 3 else (12, 0))
    plain = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=TEXTBOOK_MAX_CUTS)
    plain.Run(variant=variant)
    a, p = batch.result_arrays(), plain.result_arrays()
    for k, (n, code, cuts, ref) in enumerate(textbook_refs):
        what = (variant, names[k])
        check_numbers(batch, k, n, what)
        assert lf(batch.NarrationText(k, newline=CRLF)) == lf(n.text), what
        assert lf(batch.NarrationText(k)) == lf(n.text), what   # "\n" ends the WriteLines
        # code, cuts, log and tableau: the oracle's and the un-narrated batch's bytes
        assert (int(a["code"][k]), int(a["cuts"][k])) == (code, cuts) == (ref["code"], ref["cuts"])
        assert (int(p["code"][k]), int(p["cuts"][k])) == (code, cuts)
        assert batch.Log(k) == plain.Log(k) == [tuple(t) for t in ref["log"]], what
        assert batch.Tableau(k).tobytes() == plain.Tableau(k).tobytes() == ref["T"].tobytes(), what
    # read_all gives the same numbers in two copies
    ev, slab = batch.narration_packed()
    info = batch.narration_info()
    for k, (n, _, _, _) in enumerate(textbook_refs):
        assert [tuple(t) for t in ev[k, :len(n.events)].tolist()] == n.events
        at = int(info.data_off[k])
        assert slab[at:at + int(info.doubles_kept[k])].tobytes() == ref_data(n).tobytes()
    batch.destroy()
    plain.destroy()


# ------------------------------------------------------------------ 2. skipped rows
def zero_column_dual_item():
    """A dual tableau whose first pivot column (column 1: the ratios are 3, 2, 2) holds exact zeros
    in rows 2 and 3: the update leaves those rows, and the stored block must hold their old
    bits."""
    return np.array([[3.0, 2.0, 4.0, 0.0, 0.0, 0.0, 0.0],
                     [-1.0, -1.0, -2.0, 1.0, 0.0, 0.0, -4.5],
                     [0.5, 0.0, 0.25, 0.0, 1.0, 0.0, 7.125],
                     [0.1, 0.0, 1.0, 0.0, 0.0, 1.0, 3.0625]])


@pytest.mark.parametrize("variant", [0, 3])
def test_skipped_rows_keep_their_old_bits(engine, oracle, variant):
    T0 = zero_column_dual_item()
    n0, st0 = rt.narrate_solve(T0, cb.MODE_DUAL)
    ref0 = cb.reference(oracle, cb.MODE_DUAL, T0)
    assert st0 == ref0["code"] == 0 and n0.log == ref0["log"] and n0.log[0] == (0, 0, 1)
    first = np.asarray(n0.blocks[0])
    assert first[2].tobytes() == T0[2].tobytes() and first[3].tobytes() == T0[3].tobytes()
    assert first[0].tobytes() != T0[0].tobytes() and first[1].tobytes() != T0[1].tobytes()
    batch, _, _ = two_pass(engine, [T0], 2, mode=cb.MODE_DUAL, variant=variant)
    check_numbers(batch, 0, n0, "zero column")
    assert batch.Tableau(0).tobytes() == ref0["T"].tobytes()
    batch.destroy()
    for mode, T, victim, col in cb.nan_factor_cases(oracle):
        steps = mode == cb.MODE_DUAL
        n, st = rt.narrate_solve(T, mode, print_steps=steps, hard_cap=50)
        if mode == cb.MODE_DUAL:   # `|f| > EPS` is false for NaN: the row is left, old bits kept
            assert sv.same(np.asarray(n.blocks[0])[victim], T[victim])
        else:                      # `|f| <= EPS` is false for NaN: the row is updated to NaN
            assert np.isnan(np.asarray(n.blocks[0])[victim]).all()
        batch, _, _ = two_pass(engine, [T, T], 1, mode=mode, hard_cap=50, variant=variant)
        for k in (0, 1):
            check_numbers(batch, k, n, (mode, variant), nan=True)
            sv.assert_same(batch.Tableau(k), np.array(n.table()), (mode, variant))
        batch.destroy()


# ------------------------------------------------------------------ 3. resume
def test_chunk_of_one_pushes_nothing_twice(engine, textbook, textbook_refs):
    tabs = [T for _, T in textbook]
    for variant in (0, 3):
        batch, _, res = two_pass(engine, tabs, TEXTBOOK_MAX_CUTS, chunk=1, variant=variant)
        assert res.launches >= max(len(n.log) for n, _, _, _ in textbook_refs)
        for k, (n, _, _, _) in enumerate(textbook_refs):
            check_numbers(batch, k, n, ("chunk 1", variant, k))
        batch.destroy()


@pytest.mark.parametrize("mode", [cb.MODE_DUAL, cb.MODE_PRIMAL2])
def test_repeated_hard_cap_calls_equal_one_run(engine, oracle, mode):
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    tabs = [T for _, T in (cut_cases.dual_tableaux if mode == cb.MODE_DUAL
                           else cut_cases.primal2_tableaux)(oracle)]
    refs = [rt.narrate_solve(T, mode, print_steps=True)[0] for T in tabs]
    most = max(len(n.log) for n in refs)
    assert most >= 3
    batch = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=1)
    batch.narrate_reserve([ref_data(n).size for n in refs], 5 * (most + 2))
    calls = 0
    while True:
        batch.Run(mode=mode, hard_cap=1, print_steps=True)
        calls += 1
        if not (batch.result_arrays()["code"] == rt.LIMIT).any():
            break
        assert calls <= most
    # hard_cap stops a solve only in front of a pivot: the call that makes an item's last pivot
    # also sees its solve end
    assert calls == most
    for k, n in enumerate(refs):
        pivots = [e for e in batch.Events(k) if e[0] >= rt.EV_PIVOT]
        assert pivots == [e for e in n.events if e[0] >= rt.EV_PIVOT], k
        check_calls = [e for e in batch.Events(k) if e[0] == rt.EV_CALL]
        assert len(check_calls) == calls and all(e[1:3] == (mode, 1) for e in check_calls)
        want = ref_data(n)
        info = batch.narration_info()
        assert int(info.doubles_made[k]) == int(info.doubles_kept[k]) == want.size
        assert batch.NarrationData(k, 0, want.size).tobytes() == want.tobytes(), k
        # every call that met the cap says so; the one behind them says how the solve ended
        ends = [e for e in batch.Events(k) if e[0] == rt.EV_SOLVE_END]
        capped = max(len(n.log) - 1, 0)
        assert len(ends) == calls
        assert [e[1:3] for e in ends[:capped]] == [(rt.LIMIT, 1)] * capped
        assert ends[capped][1:3] == n.events[-2][1:3] and n.events[-2][0] == rt.EV_SOLVE_END
    batch.destroy()


# ------------------------------------------------------------------ 4. the prefix rule
SLACK = 37                       # doubles reserved behind each neighbour's need and never made
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)   # the data slab's fill at reserve time


def test_prefix_rule_and_nothing_past_the_slice(engine, oracle, textbook, textbook_refs):
    """A victim item at caps 0, need - 1 and need between neighbours that reserve SLACK doubles
    more than they make.  The slab is 0xFF bytes after reserve (checked here before the run), so
    after the run every double outside a kept block must still be that: the victim's dropped
    tail, every neighbour's slack, nothing else."""
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    T_g, _ = cb.g_item()
    pick = [3, 1, 5, 11]   # exit 4 (8 pivots), exit 1 (block 0 alone), exit 0 (6 cuts), exit 2
    tabs = [textbook[i][1] for i in pick] + [T_g]
    refs = [textbook_refs[i][0] for i in pick] + \
        [rt.narrate_cutting_plane(T_g, 8, text=False)[0]]   # no textbook item makes 8 cuts
    assert max(textbook_refs[i][2] for i in pick) < 8
    need = [ref_data(n).size for n in refs]
    n_ev = [len(n.events) for n in refs]
    for victim in (0, 2, 4):
        for cap in (0, need[victim] - 1, need[victim]):
            caps = [x + SLACK for x in need]
            caps[victim] = cap
            batch = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=TEXTBOOK_MAX_CUTS)
            batch.narrate_reserve(caps, max(n_ev) - (1 if cap == 0 else 0))
            info = batch.narration_info()
            _, before = batch.narration_packed()
            fresh = np.ones(before.size, dtype=bool)   # all but block 0 of every item is the fill
            for k, T in enumerate(tabs):
                if T.size <= caps[k]:
                    at = int(info.data_off[k])
                    fresh[at:at + T.size] = False
            assert (before.view(np.uint64)[fresh] == FILL).all()
            batch.Run(max_cuts=8)
            info = batch.narration_info()
            _, after = batch.narration_packed()
            assert info.events_made.tolist() == n_ev and info.doubles_made.tolist() == need
            outside = np.ones(after.size, dtype=bool)
            for k, n in enumerate(refs):
                want = ref_data(n)
                sizes = [np.asarray(n.record0).size] + [np.asarray(b).size for b in n.blocks]
                kept = 0
                for s in sizes:   # whole blocks, the longest prefix that fits
                    if kept + s > caps[k]:
                        break
                    kept += s
                assert int(info.doubles_kept[k]) == kept, (victim, cap, k)
                if k != victim or cap == need[k]:
                    assert kept == need[k]
                at = int(info.data_off[k])
                assert after[at:at + kept].tobytes() == want[:kept].tobytes(), (victim, cap, k)
                outside[at:at + kept] = False
                ev = batch.Events(k)
                assert ev == n.events[:len(ev)] and len(ev) == min(n_ev[k], batch._ev_cap)
            # every neighbour's slack and the victim's dropped tail: still the fill
            assert outside.sum() >= SLACK * (len(tabs) - 1)
            assert (after.view(np.uint64)[outside] == FILL).all(), (victim, cap)
            if cap < need[victim]:
                with pytest.raises(ValueError):
                    batch.NarrationText(victim)
                with pytest.raises(Exception):
                    batch.NarrationData(victim, 0, int(info.doubles_kept[victim]) + 1)
            batch.destroy()


# ------------------------------------------------------------------ 5. shapes the walk can get wrong
def test_g_and_h_items_in_one_batch(engine, oracle, textbook):
    """g_item() (41 x 101, form G) and h_item() (201 x 241, form H, 60 pivots, about 24 MB of
    blocks) with three textbook items in ONE batch: both forms in one call and one slab.  A batch
    has one row capacity, h_item()'s 12 cuts, so the G item makes 12 cuts here (52 pivots; its 23
    pivots at 8 cuts are pinned by the prefix-rule test above and on the CPU): its reference is
    the restatement at 12, checked against the oracle first.  Both end at exit 6: compared by
    numbers, NarrationText raises, and the partial text is compared with the restatement's --
    the H item's over the events through its first pivot, about 1 MB of its 36 MB."""
    from lpr_381_group_v22_amd.cut_batch import (EV_PIVOT, FORM_G, FORM_H, NarrationStopped,
                                                 form_of, format_cutting_plane)
    LIMIT = 1500000
    small = [T for _, T in textbook[:3]]
    (T_g, _), (T_h, mc) = cb.g_item(), cb.h_item()
    assert mc == 12 and form_of(*T_g.shape, mc) == FORM_G and form_of(*T_h.shape, mc) == FORM_H
    g, g_code, g_cuts = rt.narrate_cutting_plane(T_g, mc, text_limit=LIMIT)
    h, h_code, h_cuts = rt.narrate_cutting_plane(T_h, mc, text_limit=LIMIT)
    ref_g = cb.reference(oracle, cb.MODE_CUT, T_g, max_cuts=mc)
    assert (g_code, g_cuts, g.log) == (ref_g["code"], ref_g["cuts"], ref_g["log"])
    assert np.array(g.table()).tobytes() == ref_g["T"].tobytes()
    assert (g_code, g_cuts, len(g.log)) == (6, 12, 52) and g.stopped
    assert (h_code, h_cuts, len(h.log)) == cb.H_ITEM_OUTCOME and h.stopped
    smalls = [rt.narrate_cutting_plane(S, mc)[0] for S in small]
    batch, need, res = two_pass(engine, small + [T_g, T_h], mc)
    assert (res.items_g, res.items_h) == (4, 1)
    codes = batch.result_arrays()["code"]
    for k, n in ((3, g), (4, h)):
        assert int(codes[k]) == 6
        check_numbers(batch, k, n, ("large", k))
        with pytest.raises(NarrationStopped):
            batch.NarrationText(k)
    for q, s in enumerate(smalls):
        check_numbers(batch, q, s, ("beside the large items", q))
    # the G item's whole partial text begins with the restatement's first LIMIT characters
    part = batch.NarrationText(3, newline=CRLF, partial=True)
    assert len(g.text) >= LIMIT and lf(part).startswith(lf(g.text))
    # the H item: the formatter on the batch's own events and blocks through the first pivot
    ev = batch.Events(4)
    rec0, blocks = batch.NarrationBlocks(4)
    m = 1 + next(i for i, e in enumerate(ev) if e[0] >= EV_PIVOT)
    part = format_cutting_plane(ev[:m], rec0, blocks, newline=CRLF, partial=True)
    # three tableaux of at least 201 x 241 numbers, each a digit and a separator or more
    assert 3 * 2 * T_h.size < len(part) <= len(h.text) and lf(h.text).startswith(lf(part))
    assert "After pivot on cut: row 201, col " in part
    batch.destroy()


def test_form_g_above_64_kib_unnarrated_then_narrated(engine, oracle):
    """One 41 x 186 item at two cuts: 65 816 bytes of dynamic LDS in form G, the smallest width at
    this height above the 64 KiB a kernel gets without the dynamic-LDS attribute.  First on an
    un-narrated handle, then on narrated ones: k_cut_batch<true> and k_cut_batch_narr<true> each
    need the attribute set for themselves.  The oracle's bytes from both, the restatement's
    events and blocks from the narrated one."""
    from lpr_381_group_v22_amd import CuttingPlaneBatch
    from lpr_381_group_v22_amd import cut_batch as pycb
    mc = 2
    T = cut_cases.side_base(40, 145, 11)
    assert T.shape == (41, 186)
    assert pycb.footprint_g(41, 185, mc) <= 64 * 1024 < pycb.footprint_g(41, 186, mc)
    assert pycb.form_of(41, 186, mc) == pycb.FORM_G
    ref = cb.reference(oracle, cb.MODE_CUT, T, max_cuts=mc)
    n, code, cuts = rt.narrate_cutting_plane(T, mc, text=False)
    assert (code, cuts, n.log) == (ref["code"], ref["cuts"], ref["log"])
    assert (code, cuts, len(n.log)) == (6, 2, 4)
    assert np.array(n.table()).tobytes() == ref["T"].tobytes()
    plain = CuttingPlaneBatch.from_arrays(engine, [T], max_cuts=mc)
    res = plain.Run()
    assert (res.items_g, res.items_h) == (1, 0)
    batch, need, res = two_pass(engine, [T], mc)
    assert (res.items_g, res.items_h) == (1, 0)
    check_numbers(batch, 0, n, "G above 64 KiB")
    a, p = batch.result_arrays(), plain.result_arrays()
    assert (int(a["code"][0]), int(a["cuts"][0])) == (int(p["code"][0]), int(p["cuts"][0])) \
        == (code, cuts)
    assert batch.Log(0) == plain.Log(0) == [tuple(t) for t in ref["log"]]
    assert batch.Tableau(0).tobytes() == plain.Tableau(0).tobytes() == ref["T"].tobytes()
    batch.destroy()
    plain.destroy()


# ------------------------------------------------------------------ 6. modes 1 and 2
@pytest.mark.parametrize("steps", [True, False])
@pytest.mark.parametrize("mode", [cb.MODE_DUAL, cb.MODE_PRIMAL2])
def test_solver_modes_text_and_snapshots(engine, oracle, mode, steps):
    tabs = [T for _, T in (cut_cases.dual_tableaux if mode == cb.MODE_DUAL
                           else cut_cases.primal2_tableaux)(oracle)]
    assert len(tabs) == (16 if mode == cb.MODE_DUAL else 7)
    refs = [rt.narrate_solve(T, mode, print_steps=steps) for T in tabs]
    if mode == cb.MODE_PRIMAL2:
        assert rt.UNBOUNDED in {st for _, st in refs}
    batch, _, _ = two_pass(engine, tabs, 1, mode=mode, print_steps=steps)
    codes = batch.result_arrays()["code"]
    for k, (n, st) in enumerate(refs):
        assert int(codes[k]) == st
        check_numbers(batch, k, n, (mode, steps, k))
        assert lf(batch.NarrationText(k, newline=CRLF)) == lf(n.text), (mode, steps, k)
        assert (n.text == "") == (not steps)
        if mode == cb.MODE_PRIMAL2:
            assert batch.Snapshots(k) == n.snapshots, (steps, k)
            assert len(n.snapshots) == 2 * len(n.log) + len(n.log) + 1
    batch.destroy()


# ------------------------------------------------------------------ 7. from_primal_batch, texts
def _models():
    import bb_cases
    from lpr_381_group_v22_amd import Constraint
    return [(list(obj), [Constraint(list(c.Coefficients), c.Relation, c.RHS) for c in cons], True)
            for _, (obj, cons) in bb_cases.all_bb_cases()]


def test_from_primal_batch_then_reserve(engine, oracle):
    from lpr_381_group_v22_amd import CuttingPlaneBatch, PrimalSimplexBatch
    roots = cut_cases.cutting_plane_tableaux(oracle)
    refs = [rt.narrate_cutting_plane(T, 6)[0] for _, T in roots]

    def make():
        lp = PrimalSimplexBatch(_models(), engine=engine)
        lp.Solve()
        b = CuttingPlaneBatch.from_primal_batch(lp, max_cuts=6)
        lp.destroy()
        return b

    batch, _, _ = two_pass(engine, None, 6, from_batch=make)
    assert batch.Count == len(roots)
    for k, n in enumerate(refs):
        check_numbers(batch, k, n, ("from_primal_batch", k))
        if not n.stopped:
            assert lf(batch.NarrationText(k, newline=CRLF)) == lf(n.text)
    batch.destroy()


def test_cutting_plane_texts(engine, textbook, textbook_refs):
    from lpr_381_group_v22_amd import cutting_plane_texts
    texts = cutting_plane_texts([T for _, T in textbook], max_cuts=TEXTBOOK_MAX_CUTS,
                                engine=engine, newline=CRLF)
    assert len(texts) == 12
    for text, (n, _, _, _) in zip(texts, textbook_refs):
        assert lf(text) == lf(n.text)


# ------------------------------------------------------------------ 8. arguments
def test_arguments_and_refusals(engine, textbook):
    import ctypes as C
    from lpr_381_group_v22_amd import CuttingPlaneBatch, _native as N
    tabs = [T for _, T in textbook[:3]]
    I64 = C.POINTER(C.c_int64)

    def reserve(b, caps, ev_cap):
        arr = None if caps is None else np.asarray(caps, dtype=np.int64)
        return N.lib.lpr_cut_batch_narrate_reserve(
            b._h, None if arr is None else arr.ctypes.data_as(I64), ev_cap)

    b = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=4)
    # an un-narrated handle refuses the reads
    cnt = C.c_int64()
    one = np.zeros(4, dtype=np.float64)
    assert N.lib.lpr_cut_batch_narrate_info(b._h, None, None, None, None) == N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_cut_batch_narrate_events_read(b._h, 0, None, 0, C.byref(cnt)) == \
        N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_cut_batch_narrate_data_read(
        b._h, 0, 0, 1, one.ctypes.data_as(C.POINTER(C.c_double))) == N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_cut_batch_narrate_read_all(b._h, None, 0, None, 0) == N.LPR_BAD_ARGUMENT
    assert "not narrated" in N.lib.lpr_last_error().decode()
    # bad reserves leave it un-narrated
    assert reserve(b, None, 4) == N.LPR_BAD_ARGUMENT
    assert reserve(b, [10, -1, 10], 4) == N.LPR_BAD_ARGUMENT
    assert "cap_doubles[1]" in N.lib.lpr_last_error().decode()
    assert reserve(b, [10, 10, 10], 0) == N.LPR_BAD_ARGUMENT
    # a failed allocation names the buffer and its size; the handle stays usable and un-narrated
    assert reserve(b, [1 << 46, 0, 0], 4) == N.LPR_OUT_OF_MEMORY
    msg = N.lib.lpr_last_error().decode()
    assert "narration data slab" in msg and str(1 << 46) in msg
    assert N.lib.lpr_cut_batch_narrate_info(b._h, None, None, None, None) == N.LPR_BAD_ARGUMENT
    # a good one, once
    assert reserve(b, [1000, 1000, 1000], 64) == N.LPR_OK_OPTIMAL
    assert reserve(b, [1000, 1000, 1000], 64) == N.LPR_BAD_ARGUMENT
    assert "narrated already" in N.lib.lpr_last_error().decode()
    assert N.lib.lpr_cut_batch_narrate_info(b._h, None, None, None, None) == N.LPR_OK_OPTIMAL
    made = np.zeros(3, dtype=np.int64)
    kept = np.zeros(3, dtype=np.int64)
    assert N.lib.lpr_cut_batch_narrate_info(b._h, None, made.ctypes.data_as(I64),
                                            kept.ctypes.data_as(I64), None) == N.LPR_OK_OPTIMAL
    assert made.tolist() == kept.tolist() == [T.size for T in tabs]   # block 0 at reserve time
    # a range beyond what is kept, a bad item, too small a read_all buffer
    dp = one.ctypes.data_as(C.POINTER(C.c_double))
    assert N.lib.lpr_cut_batch_narrate_data_read(b._h, 0, int(kept[0]) - 3, 4, dp) == \
        N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_cut_batch_narrate_data_read(b._h, 0, int(kept[0]) - 4, 4, dp) == \
        N.LPR_OK_OPTIMAL
    assert one.tobytes() == tabs[0].reshape(-1)[-4:].tobytes()
    assert N.lib.lpr_cut_batch_narrate_data_read(b._h, 3, 0, 1, dp) == N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_cut_batch_narrate_events_read(b._h, -1, None, 0, C.byref(cnt)) == \
        N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_cut_batch_narrate_events_read(b._h, 0, None, 0, None) == N.LPR_BAD_ARGUMENT
    assert N.lib.lpr_cut_batch_narrate_read_all(b._h, None, 0, dp, 4) == N.LPR_BAD_ARGUMENT
    b.destroy()

    # after a run a reserve is refused, and the un-narrated handle of a failed reserve still runs
    b = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=4)
    assert reserve(b, [1 << 46, 0, 0], 4) == N.LPR_OUT_OF_MEMORY
    plain = CuttingPlaneBatch.from_arrays(engine, tabs, max_cuts=4)
    b.Run()
    plain.Run()
    assert b.result_arrays()["code"].tolist() == plain.result_arrays()["code"].tolist()
    for k in range(3):
        assert b.Tableau(k).tobytes() == plain.Tableau(k).tobytes() and b.Log(k) == plain.Log(k)
    assert reserve(b, [1000, 1000, 1000], 64) == N.LPR_BAD_ARGUMENT
    assert "has run" in N.lib.lpr_last_error().decode()
    b.destroy()
    plain.destroy()

    # an engine closed under a narrated handle orphans it; destroy still works
    import lpr_381_group_v22_amd as pkg
    eng2 = pkg.Engine(0)
    b = CuttingPlaneBatch.from_arrays(eng2, tabs, max_cuts=4)
    b.narrate_reserve(1000, 64)
    b.Run()
    eng2.close()
    assert N.lib.lpr_cut_batch_narrate_info(b._h, None, None, None, None) == N.LPR_BAD_ARGUMENT
    b.destroy()
