"""CPU tests of the cutting-plane batch: the ABI, the ctypes binding and
the C# binding declare the lpr_cut_batch_* calls, the Python form helpers are the constants of
batch_common.hpp, and pack_tableaux refuses what lpr_cut_batch_create refuses.

The later tests do not test the batch: they run the oracle and ref_py_cut on the fixtures of
tests/cut_batch_cases.py, so that the GPU tests' cases cannot decay into easy ones."""
import ctypes
import os
import re

import numpy as np
import pytest

import cut_batch_cases as cb
import cut_cases
import ref_py_cut as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

CUT_BATCH_CALLS = ["lpr_cut_batch_create", "lpr_cut_batch_from_batch", "lpr_cut_batch_destroy",
                   "lpr_cut_batch_run", "lpr_cut_batch_result_read", "lpr_cut_batch_shape",
                   "lpr_cut_batch_tableau_read", "lpr_cut_batch_log_read", "lpr_cut_batch_z_read"]


def test_header_and_bindings_declare_the_cut_batch_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    for name in CUT_BATCH_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"static extern \w+ " + name + r"\(", cs)) == 1, name
    assert "typedef struct lpr_cut_batch lpr_cut_batch;" in text
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in CUT_BATCH_CALLS:
        assert hasattr(lib, name), name


def test_ctypes_structs_match_the_header():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for struct, cls in (("lpr_cut_batch_opts", N.CutBatchOpts),
                        ("lpr_cut_batch_result", N.CutBatchResult)):
        body = re.search(r"typedef struct %s\s*{(.*?)}\s*%s;" % (struct, struct), text,
                         re.S).group(1)
        fields = re.findall(r"int(?:32|64)_t\s+(\w+)(?:\[\d+\])?\s*;", body)
        assert fields == [f[0] for f in cls._fields_], struct
    assert ctypes.sizeof(N.CutBatchOpts) == 32 and N.CutBatchOpts.hard_cap.offset == 8
    assert ctypes.sizeof(N.CutBatchResult) == 64 and N.CutBatchResult.cuts.offset == 48


def test_package_exports_the_batch():
    import lpr_381_group_v22_amd as pkg
    assert pkg.CuttingPlaneBatch is pkg.cut_batch.CuttingPlaneBatch
    assert "CuttingPlaneBatch" in pkg.__all__ and "pack_tableaux" in pkg.__all__
    for m in ("from_arrays", "from_primal_batch", "Run", "result_arrays", "Tableau", "Log",
              "Shape", "destroy"):
        assert hasattr(pkg.CuttingPlaneBatch, m), m


def _constant(src, name):
    m = re.search(r"constexpr \w+ %s(?:\[\w+\])? = ([^;]+);" % name, src)
    assert m, name
    return m.group(1)


def test_form_helpers_match_the_headers():
    from lpr_381_group_v22_amd import cut_batch as pycb
    common = open(os.path.join(CSRC, "batch_common.hpp")).read()
    assert _constant(common, "kBatchWgScratch") == "(size_t)1 << 10"
    assert _constant(common, "kBatchMaxLdsG") == "((size_t)160 << 10) - kBatchWgScratch"
    assert pycb.MAX_LDS_G == (160 << 10) - (1 << 10) == cb.MAX_LDS_G
    assert int(_constant(common, "kBatchMaxRowsH")) == pycb.MAX_ROWS_H
    assert int(_constant(common, "kBatchMaxColsH")) == pycb.MAX_COLS_H
    assert int(_constant(common, "kBatchLogDefaultMax")) == pycb.LOG_DEFAULT_MAX
    own = open(os.path.join(CSRC, "cut_batch_common.hpp")).read()
    assert _constant(own, "kCutBatchChunk") == "{0, %d, %d}" % (pycb.CHUNK[pycb.FORM_G],
                                                                 pycb.CHUNK[pycb.FORM_H])
    assert int(_constant(own, "kCutBatchDefaultMaxCuts")) == pycb.DEFAULT_MAX_CUTS
    assert "(size_t)rcap * cols * sizeof(double) + cut_batch_aux_bytes(rcap, cols)" in own
    assert "(size_t)(rcap + cols) * sizeof(double)" in own
    eng = open(os.path.join(CSRC, "cut_batch_engine.hip")).read()
    assert "batch_pick_form(fp, o.variant, false)" in eng
    # the figure of the issue: (m, n) = (110, 20) at capacity + 1
    assert pycb.footprint_g(111, 131, 1) == 119320 == cb.footprint_g(111, 131, 1)
    assert pycb.footprint_g(8, 14, 0) == 8 * (72 * 14 + 72 + 14)   # max_cuts <= 0 is 64
    assert pycb.form_of(8, 14, 6) == pycb.FORM_G
    assert pycb.form_of(8, 14, 6, pycb.VARIANT_H) == pycb.FORM_H
    assert pycb.form_of(201, 241, 12) == pycb.FORM_H
    assert pycb.form_of(201, 241, 12, pycb.VARIANT_G) == pycb.FORM_H   # does not fit: stays H
    n_fit, n_over = cb.boundary_shapes()
    assert pycb.fits_g(41, n_fit + 41, 8) and not pycb.fits_g(41, n_over + 41, 8)
    assert pycb.launches_for(60, 16) == 4 and pycb.launches_for(60, 15) == 4
    assert pycb.launches_for(23, 8) == 3 and pycb.launches_for(0, 16) == 1


def test_pack_tableaux_packs_and_refuses():
    from lpr_381_group_v22_amd.cut_batch import pack_tableaux
    a = np.arange(10.0).reshape(2, 5)
    b = np.arange(12.0).reshape(4, 3)
    p = pack_tableaux([a, b.tolist()], max_cuts=3)
    assert p.rows.tolist() == [2, 4] and p.cols.tolist() == [5, 3] and p.rows.dtype == np.int32
    assert p.tableaux.tobytes() == a.tobytes() + b.tobytes()
    bad = [
        ([], 1),                                        # no tableaux
        ([[[1.0, 2.0, 3.0], [1.0, 2.0]]], 1),           # ragged rows
        ([np.zeros(5)], 1),                             # not 2-D
        ([np.zeros((1, 5))], 1),                        # no constraint row
        ([np.zeros((3, 1))], 1),                        # no column besides the RHS
        ([np.zeros((1000, 5))], 25),                    # 1025 rows at capacity
        ([np.zeros((961, 5))], 0),                      # ... with the default 64
        ([np.zeros((3, 2049))], 1),
        ([a, "tableau"], 1),
    ]
    for tabs, mc in bad:
        with pytest.raises(ValueError):
            pack_tableaux(tabs, max_cuts=mc)
    pack_tableaux([np.zeros((960, 2048))], 0)           # exactly the limit


# ---- guards on the fixtures -------------------------------------------------------------------
def split(T):
    return list(map(float, T[0])), [list(map(float, r)) for r in T[1:]]


def join(obj, rows):
    return np.array([obj] + rows, dtype=np.float64)


def ref_py(mode, T, max_cuts=0, hard_cap=0, max_iters=10000, print_steps=None):
    """cut_batch_cases.reference through ref_py_cut."""
    obj, rows = split(T)
    log = []
    if mode == cb.MODE_CUT:
        code, cuts = rp.cutting_plane(obj, rows, max_cuts=max_cuts, log=log, hard_cap=hard_cap)
        return dict(code=code, cuts=cuts, T=join(obj, rows), log=log)
    if print_steps is None:
        print_steps = mode == cb.MODE_DUAL
    fn = rp.dual_solve if mode == cb.MODE_DUAL else rp.primal2_solve
    st = fn(obj, rows, max_iters=max_iters, print_steps=print_steps, log=log, hard_cap=hard_cap)
    code = {"ok": 0, "infeasible": 2, "unbounded": 1, "limit": 5}[st]
    return dict(code=code, cuts=0, T=join(obj, rows), log=log)


def agree(a, b, what):
    assert a["code"] == b["code"] and a["cuts"] == b["cuts"], what
    assert [tuple(t) for t in a["log"]] == [tuple(t) for t in b["log"]], what
    assert a["T"].shape == b["T"].shape and a["T"].tobytes() == b["T"].tobytes(), what


def test_textbook_items_reach_every_exit(oracle):
    """Exits {0, 1, 2, 4, 5, 6} over max_cuts 1 / 6 and hard_cap 2000 / 2 / 1, and the two items
    that hard_cap 1 turns."""
    items = cb.textbook_items(oracle)
    exits, by = set(), {}
    for mc in (1, 6):
        for hc in (2000, 2, 1):
            for name, T in items:
                ref = cb.reference(oracle, cb.MODE_CUT, T, max_cuts=mc, hard_cap=hc)
                agree(ref, ref_py(cb.MODE_CUT, T, max_cuts=mc, hard_cap=hc), (name, mc, hc))
                exits.add(ref["code"])
                by[(name, mc, hc)] = (ref["code"], ref["cuts"])
    assert exits == {0, 1, 2, 4, 5, 6}
    assert by[("exit2_integer_rows", 1, 2000)] == (2, 1)
    assert by[("huge_relaxation_value", 6, 2000)][0] == 5
    assert by[("huge_relaxation_value", 6, 1)][0] == 4
    assert by[("binary_10v2c_s4", 6, 2000)] == (0, 6)
    assert by[("binary_10v2c_s4", 6, 1)] == (4, 1)


def test_larger_items_give_their_outcomes(oracle):
    for (T, mc), want in ((cb.g_item(), cb.G_ITEM_OUTCOME), (cb.h_item(), cb.H_ITEM_OUTCOME)):
        ref = cb.reference(oracle, cb.MODE_CUT, T, max_cuts=mc, hard_cap=2000)
        assert (ref["code"], ref["cuts"], ref["pivots"]) == want
        agree(ref, ref_py(cb.MODE_CUT, T, max_cuts=mc, hard_cap=2000), want)
    from lpr_381_group_v22_amd import cut_batch as pycb
    (Tg, mg), (Th, mh) = cb.g_item(), cb.h_item()
    assert pycb.form_of(*Tg.shape, mg) == pycb.FORM_G
    assert pycb.form_of(*Th.shape, mh) == pycb.FORM_H


def test_modes_1_and_2_fixtures_agree(oracle):
    for mode, tabs in ((cb.MODE_DUAL, cut_cases.dual_tableaux(oracle)),
                       (cb.MODE_PRIMAL2, cut_cases.primal2_tableaux(oracle))):
        for name, T in tabs:
            for kw in (dict(hard_cap=3000), dict(max_iters=1, print_steps=True, hard_cap=3000),
                       dict(max_iters=1, print_steps=False, hard_cap=3000)):
                agree(cb.reference(oracle, mode, T, **kw), ref_py(mode, T, **kw), (name, kw))


@pytest.mark.parametrize("gen_name", list(cb.STRIDE_GENS))
def test_stride_cases_name_their_planted_index(oracle, gen_name):
    """The oracle's first log triple names the planted index at every shape, tie mode and gap;
    at the G shapes ref_py_cut agrees with the oracle on the whole result."""
    from lpr_381_group_v22_amd import cut_batch as pycb
    for form, want in (("G", pycb.FORM_G), ("H", pycb.FORM_H)):
        mode, field, items = cb.stride_group(gen_name, form)
        assert len(items) == len(cb.STRIDE_GENS[gen_name][4]) * len(cb.G_GAPS if form == "G"
                                                                      else cb.H_GAPS)
        for name, T, planted in items:
            assert pycb.form_of(T.shape[0], T.shape[1], 1) == want, name
            ref = cb.stride_reference(oracle, mode, T)
            assert ref["log"] and ref["log"][0][field] == planted, name
            if form == "G":
                kw = dict(max_cuts=1) if mode == cb.MODE_CUT else {}
                agree(ref, ref_py(mode, T, hard_cap=cb.STRIDE_HARD_CAP, **kw), name)


def test_nan_factor_cases_split_the_two_skip_rules(oracle):
    """primal2 rewrites the row of a NaN factor, the dual pivot leaves it."""
    (m2, T2, v2, c2), (m1, T1, v1, c1) = cb.nan_factor_cases(oracle)
    assert (m2, m1) == (cb.MODE_PRIMAL2, cb.MODE_DUAL)
    r2 = cb.reference(oracle, m2, T2, hard_cap=1)
    assert r2["pivots"] == 1 and np.isnan(r2["T"][v2]).all()
    r1 = cb.reference(oracle, m1, T1, hard_cap=1)
    assert r1["pivots"] == 1 and np.isnan(r1["T"][v1]).sum() == 1 and np.isnan(r1["T"][v1, c1])
