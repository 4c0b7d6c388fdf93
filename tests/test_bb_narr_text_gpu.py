"""GPU tests of the narrated B&B batch's device text (lpr_text_format_tableaux_rounded,
lpr_bb_batch_narrate_text): DisplayTableau -- Math.Round(v, 4) then Format --
written on the device, against host Format of the host-rounded tableau for values planted on the
rounding's seams, and NarrationTextDevice against NarrationText and the restatement's text across
forms, chunks, caps, pruning and node caps.  Every comparison is of bytes."""
import ctypes as C
import math

import numpy as np
import pytest

import special_values as sv
from test_bb_batch_gpu import PIV_CAP, bb_roots, form_of, make
from test_bb_batch_narr_gpu import (CAP, _h_root, batch, last_error, lf, narrated,  # noqa: F401
                                    ref_text, ref_walk, slices)
from test_bb_narr_text_cpu import host_body

pytestmark = pytest.mark.gpu


def ulp(v, up):
    return float(np.nextafter(v, math.inf if up else -math.inf))


def planted():
    """Values on the seams of Math.Round(v, 4) followed by F3.  Checked on the CPU
    (ref_py_bb.round4 / ref_py_text.py_fixed): 0.00049999 prints 0.000 raw and 0.001 rounded,
    1.23449999 prints 1.234 / 1.235."""
    vals = [0.00049999, 0.0004999999999, 1.23449999, -1.23449999, 7.00049999, -0.00049999,
            12345.67849999, 0.00045, 0.0005, 0.00049999999999999, -0.00004, 0.00004, -0.00005]
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 10000, 10001, 123456, 123457):  # ties of x * 1e4, both parities
        vals += [(k + 0.5) / 1e4, -(k + 0.5) / 1e4]
    vals += [0.5 ** 14, 3 * 0.5 ** 14, 0.5 ** 15]  # x * 1e4 = 0.6103.., exact binary fractions
    for edge in (1e11, 1e15, 1e16):  # the second rounding's threshold, the big-cell path, identity
        for v in (ulp(edge, False), edge, ulp(edge, True)):
            vals += [v, -v]
    vals += [999999999999999.875, 99999999999.99995, 9.9e15, 1e16 - 2, 123456789012.34565,
             1e15 + 0.375, 5e15 + 0.5, 1e17, 1e22]
    vals += [math.nan, math.inf, -math.inf, 5e-324, -5e-324, sv.MIN_NORMAL, sv.DBL_MAX,
             -sv.DBL_MAX, 0.0, -0.0, 1.0, -1.0, 2.0005, 0.0015, 99.9995]
    return vals


SHAPES = [(1, 1), (3, 5), (2, 65), (1, 130), (1, 1), (1, 1), (1, 1)]  # 65, 130: rows past 64 lanes


def planted_tableaux():
    pool, at, out = planted(), 0, []
    assert len(pool) <= sum(r * c for r, c in SHAPES)  # every planted value is in some tableau
    for n, (r, c) in enumerate(SHAPES):
        if n >= 4:  # the further 1 x 1 blocks: one seam value each
            t = np.array([[(ulp(1e15, False), math.nan, -0.00004)[n - 4]]])
        else:
            t = np.array([pool[(at + i) % len(pool)] for i in range(r * c)]).reshape(r, c)
            at += r * c
        out.append(t)
    return out


def nvars_of(tabs):
    return [min(2, t.shape[1] - 1) for t in tabs]


# ------------------------------------------------------------------ 1. planted values, rounded
def test_planted_values_show_the_rounding():
    """The inputs do what the GPU comparison relies on, on the host alone."""
    assert host_body(np.array([[0.00049999]]), 0, 0).endswith("Z\t0.000\t\r\n")
    assert host_body(np.array([[0.00049999]]), 0, 1).endswith("Z\t0.001\t\r\n")
    assert host_body(np.array([[0.0004999999999]]), 0, 1).endswith("Z\t0.001\t\r\n")
    assert host_body(np.array([[1.23449999]]), 0, 0).endswith("Z\t1.234\t\r\n")
    assert host_body(np.array([[1.23449999]]), 0, 2).endswith("Z\t1.235\t\r\n")
    assert host_body(np.array([[-0.00004]]), 0, 1).endswith("Z\t0.000\t\r\n")


@pytest.mark.parametrize("r", [0, 1, 2, "mixed"])
def test_format_bodies_rounded_equals_host_format_of_the_rounded_tableau(engine, r):
    from lpr_381_group_v22_amd import table_iteration_formater as fmt
    tabs = planted_tableaux()
    nv = nvars_of(tabs)
    r4 = [(0, 1, 2)[(i + 1) % 3] for i in range(len(tabs))] if r == "mixed" else [r] * len(tabs)
    got = fmt.format_bodies(tabs, nv, engine, round4=r4 if r == "mixed" else r)
    for i, t in enumerate(tabs):
        assert got[i].encode() == host_body(t, nv[i], r4[i]).encode(), (r, i, t.shape)
    if r == 1:  # the planted values tell rounded from unrounded
        raw = fmt.format_bodies(tabs, nv, engine)
        assert all(a != b for a, b in zip(got[:4], raw[:4]))


# ------------------------------------------------------------------------ 2. narrated batches
def check_batch(bb, roots, cap=CAP, pruning=False, restatement=True):
    text, first = bb.FormatNarration()
    info, res = bb.narration_info(), bb.result_arrays()
    assert first[0] == 0 and all(a <= b for a, b in zip(first[:-1], first[1:]))
    assert info.doubles_kept.tolist() == info.doubles_made.tolist()
    assert first[-1] == text.Count == int(info.tableaux.sum()) + int(res["found"].sum())
    for k, (name, T, nv) in enumerate(roots):
        assert first[k + 1] - first[k] == info.tableaux[k] + res["found"][k], name
        host = bb.NarrationText(k)
        assert bb.NarrationTextDevice(k).encode() == host.encode(), name
        if restatement:
            assert lf(host) == ref_text(ref_walk(name, T, nv, cap, pruning)[0]), name
    assert bb.all_narration_texts("\r\n") == [bb.NarrationText(k, "\r\n")
                                              for k in range(bb.Count)]


def test_device_text_equals_host_text_and_the_restatement(batch):
    bb, roots = batch
    check_batch(bb, roots)
    seen = "".join(bb.NarrationTextDevice(k) for k in range(bb.Count))
    for line in ("Infeasible tableau", "final tableau", "Optimal solution tableau at branch"):
        assert line in seen, line


def test_form_h_root_wider_than_a_wave(engine, oracle):
    roots = _h_root(oracle)
    assert len(roots) == 1 and form_of(roots[0][1], CAP) == 2 and roots[0][1].shape[1] > 64
    bb = narrated(engine, roots)
    check_batch(bb, roots, restatement=False)  # its restatement takes minutes; the host path is
    bb.destroy()                               # held against the single path in the parent's test


def _some_roots(oracle):
    return bb_roots(oracle)[:4] + [r for r in bb_roots(oracle) if r[0] == "frac_4v2c_s10"]


def test_chunk_one(batch, engine):
    base, roots = batch
    bb = narrated(engine, roots, chunk=1)
    check_batch(bb, roots)
    assert bb.all_narration_texts() == base.all_narration_texts()
    bb.destroy()


@pytest.mark.parametrize("cap,pruning", [(20, True), (1, False), (64, False)])
def test_pruning_and_node_caps(engine, oracle, cap, pruning):
    roots = _some_roots(oracle)
    bb = narrated(engine, roots, cap=cap, pruning=pruning)
    check_batch(bb, roots, cap, pruning)
    bb.destroy()


# -------------------------------------------------------------------------------------- 3. caps
def test_caps_one_double_short_raise_where_the_host_path_raises(batch, engine):
    base, roots = batch
    need = base.narration_info().doubles_made
    bb = make(engine, roots, CAP)
    bb.narrate_reserve([max(int(n) - 1, 0) for n in need])
    bb.Run()
    info = bb.narration_info()
    text, first = bb.FormatNarration()
    cut = 0
    for k in range(bb.Count):
        if info.doubles_kept[k] < need[k]:
            cut += 1
            for call in (bb.NarrationText, bb.NarrationTextDevice):
                with pytest.raises(ValueError, match="would miss tableaux"):
                    call(k)
        else:
            assert bb.NarrationTextDevice(k) == base.NarrationText(k), k
    assert cut > 0
    # the blocks are those of the kept prefix: everything but each cut IP's last tableau
    found = bb.result_arrays()["found"]
    assert first[-1] == int(info.tableaux.sum()) - cut + int(found.sum())
    bb.destroy()


def test_caps_of_zero_and_no_incumbent_are_refused(engine, oracle):
    from lpr_381_group_v22_amd import _native as N
    probe = make(engine, bb_roots(oracle), 1)
    probe.Run()
    roots = [r for k, r in enumerate(bb_roots(oracle)) if not probe.Result(k)["found"]]
    probe.destroy()
    assert roots  # a root that is not integer has no incumbent after one pop
    bb = make(engine, roots, 1)
    bb.narrate_reserve(0)
    bb.Run()
    assert bb.narration_info().tableaux.sum() > 0 and bb.narration_info().doubles_kept.sum() == 0
    with pytest.raises(N.EngineError):
        bb.FormatNarration()
    assert "lpr_bb_batch_narrate_text" in last_error() and "nothing to format" in last_error()
    bb.narrate_reserve(bb.narration_info().doubles_made)  # the batch stays usable
    bb.Run()
    check_batch(bb, roots, cap=1)
    bb.destroy()


# -------------------------------------------------------------------- 4. special values, slab
def test_special_values_through_the_slab(engine, oracle):
    """Start tableaux with one planted +-inf, NaN or 1e308 (tests/special_values.py), eight per
    planted value, evenly spaced over the positions."""
    cases = sv.bb_start_tableaux(oracle)
    per_value = len(cases) // len(sv.BB_VALUES)
    pick = [cases[min(v * per_value + (i * per_value) // 8, len(cases) - 1)]
            for v in range(len(sv.BB_VALUES)) for i in range(8)]
    assert len(pick) == 32 and len({c[0].split("@")[0] for c in pick}) == len(sv.BB_VALUES)
    from lpr_381_group_v22_amd import BranchAndBoundBatch
    bb = BranchAndBoundBatch.from_tableaux([c[1] for c in pick], [c[2] for c in pick],
                                           node_cap=sv.BB_NODE_CAP, trace_cap=PIV_CAP,
                                           engine=engine)
    bb.Narrate()
    seen, texts = "", 0
    for k, (name, _, _) in enumerate(pick):
        try:
            host = bb.NarrationText(k)
        except ValueError as e:
            with pytest.raises(ValueError) as got:
                bb.NarrationTextDevice(k)
            assert str(got.value) == str(e), name
            continue
        assert bb.NarrationTextDevice(k).encode() == host.encode(), name
        seen += host
        texts += 1
    assert texts > 16 and "NaN" in seen and "Infinity" in seen
    bb.destroy()


# ---------------------------------------------------------------------------------- 5. option 3
def test_option3_texts_with_device_text_are_the_same(engine):
    import os
    import lpr_381_group_v22_amd as pkg
    from test_bb_batch_gpu import _models, _parser
    sample = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "TextFile.txt")

    def parsers():
        p = pkg.InputFileParser()
        p.ReadInputFile(sample)
        return [p] + [_parser(obj, cons) for _, obj, cons in _models()[:6]]

    host = pkg.option3_texts(parsers(), engine=engine)
    dev = pkg.option3_texts(parsers(), engine=engine, device_text=True)
    assert len(host) == len(dev) == 7
    for k, (a, b) in enumerate(zip(host, dev)):
        assert a[0].encode() == b[0].encode(), k
        assert a[1] == b[1] and sv.same(a[2], b[2]), k


# ------------------------------------------------------------- 6. lifecycle and bad arguments
def raw_text(h):
    """Every byte and offset of an lpr_text, read now."""
    from lpr_381_group_v22_amd import _native as N
    blocks, nbytes = C.c_int64(), C.c_int64()
    N.check(N.lib.lpr_text_info(h, C.byref(blocks), C.byref(nbytes), None), "lpr_text_info")
    off = np.zeros(blocks.value + 1, dtype=np.int64)
    data = np.zeros(max(nbytes.value, 1), dtype=np.uint8)
    N.check(N.lib.lpr_text_offsets_read(h, N._ptr(off, C.c_int64)), "lpr_text_offsets_read")
    N.check(N.lib.lpr_text_read(h, 0, nbytes.value, N._ptr(data, C.c_uint8)), "lpr_text_read")
    return off.tobytes(), data[:nbytes.value].tobytes()


def test_lifecycle_and_bad_arguments(oracle):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd import table_iteration_formater as fmt
    eng = pkg.Engine(0)
    roots = bb_roots(oracle)[:3]
    bb = make(eng, roots, CAP)
    L = N.lib
    h = C.c_void_p()
    first = np.zeros(bb.Count + 1, dtype=np.int64)
    fp = first.ctypes.data_as(C.POINTER(C.c_int64))

    def refused(rc, what):
        assert rc == N.LPR_BAD_ARGUMENT and "lpr_bb_batch_narrate_text" in last_error() and \
            what in last_error(), (rc, last_error())

    bb.Run()
    refused(L.lpr_bb_batch_narrate_text(bb._h, fp, C.byref(h)), "not narrated")
    bb.narrate_reserve(1 << 20)
    refused(L.lpr_bb_batch_narrate_text(bb._h, fp, C.byref(h)), "has not run since")
    bb.Run()
    refused(L.lpr_bb_batch_narrate_text(bb._h, fp, None), "null out")
    refused(L.lpr_bb_batch_narrate_text(None, fp, C.byref(h)), "null or orphaned")
    assert L.lpr_bb_batch_narrate_text(bb._h, None, C.byref(h)) == 0  # first_block may be NULL
    assert L.lpr_text_destroy(h) == 0
    assert L.lpr_bb_batch_narrate_text(bb._h, fp, C.byref(h)) == 0
    want = raw_text(h)
    texts = [bb.NarrationTextDevice(k) for k in range(bb.Count)]
    assert texts == [bb.NarrationText(k) for k in range(bb.Count)]
    # the text owns its bytes: a second run (another search: pruning on), a new reserve and the
    # batch's destruction leave it as it is
    bb.Run(enable_pruning=True)
    assert raw_text(h) == want
    bb.narrate_reserve(0)
    assert raw_text(h) == want
    bb.destroy()
    assert raw_text(h) == want
    # a bad round4 entry names its index
    t = [np.ones((2, 3)), np.ones((1, 2)), np.ones((2, 2))]
    with pytest.raises(N.EngineError):
        fmt.format_bodies(t, 1, eng, round4=[0, 3, 1])
    assert "lpr_text_format_tableaux_rounded" in last_error() and "round4[1] = 3" in last_error()
    with pytest.raises(N.EngineError):
        fmt.format_bodies(t, 1, eng, round4=[2, 1, -1])
    assert "round4[2] = -1" in last_error()
    # closing the engine orphans the text and the batch
    bb2 = make(eng, roots, CAP)
    bb2.Narrate()
    eng.close()
    assert L.lpr_text_info(h, None, None, None) == N.LPR_BAD_ARGUMENT
    refused(L.lpr_bb_batch_narrate_text(bb2._h, fp, C.byref(h)), "orphaned")
    assert L.lpr_text_destroy(h) == 0
    bb2.destroy()


# ---------------------------------------------------------------------------- 7. unchanged paths
def test_round4_zero_is_the_unrounded_call(engine):
    from lpr_381_group_v22_amd import table_iteration_formater as fmt
    tabs = planted_tableaux()
    nv = nvars_of(tabs)
    plain = fmt.format_bodies(tabs, nv, engine)
    assert plain == fmt.format_bodies(tabs, nv, engine, round4=0)
    assert plain == fmt.format_bodies(tabs, nv, engine, round4=[0] * len(tabs))
    assert plain == [host_body(t, n, 0) for t, n in zip(tabs, nv)]
    titles = ["t%d" % i for i in range(len(tabs))]
    assert fmt.FormatMany(tabs, nv, titles, engine, round4=1) == \
        [fmt.title_line(s) + host_body(t, n, 1) for s, t, n in zip(titles, tabs, nv)]


def test_format_narration_leaves_the_slab_as_it_is(batch):
    bb, _ = batch
    before = slices(bb)
    tabs = [bb.IncumbentTableau(k) for k in range(bb.Count)]
    bb._drop_narration_text()
    text, _ = bb.FormatNarration()
    assert text.Count > 0 and text.KernelMs > 0
    assert slices(bb) == before
    for k, t in enumerate(tabs):
        u = bb.IncumbentTableau(k)
        assert (t is None) == (u is None) and (t is None or t.tobytes() == u.tobytes())
