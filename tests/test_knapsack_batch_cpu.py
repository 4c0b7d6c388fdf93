"""CPU tests of the knapsack batch, no device: the header and both bindings
declare the lpr_knap_batch_* calls, the Python form helpers are the constants and the formula of
the C++ headers, pack_knapsacks refuses what lpr_knap_batch_create refuses, and the instances of
tests/knapsack_batch_cases.py have, on the restatement, the properties the GPU tests rely on."""
import ctypes
import os
import re

import pytest

import knapsack_batch_cases as kb
import knapsack_cases as KC
import ref_py_knapsack as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

CALLS = ["lpr_knap_batch_create", "lpr_knap_batch_destroy", "lpr_knap_batch_solve",
         "lpr_knap_batch_result_read", "lpr_knap_batch_rank_read", "lpr_knap_batch_selected_read",
         "lpr_knap_batch_nodes_read", "lpr_knap_batch_dp"]


def test_header_and_bindings_declare_the_calls():
    from lpr_381_group_v22_amd import _native as N
    text = open(os.path.join(ROOT, "include", "lpr_engine.h")).read()
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    gs = open(os.path.join(ROOT, "integration", "csharp", "GpuSolvers.cs")).read()
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
        assert re.search(r"static extern int %s\(" % name, cs), name
        assert "NativeMethods.%s(" % name in gs, name
    assert "typedef struct lpr_knap_batch lpr_knap_batch;" in text
    assert "AT THE SAME node_cap" in text          # the parity statement of the issue
    assert ctypes.sizeof(N.KnapBatchOpts) == 8 and ctypes.sizeof(N.KnapBatchResult) == 32
    for struct, cls in (("lpr_knap_batch_opts", N.KnapBatchOpts),
                        ("lpr_knap_batch_result", N.KnapBatchResult)):
        body = re.search(r"typedef struct %s\s*{(.*?)}" % struct, text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in cls._fields_], struct


def test_package_exports():
    import lpr_381_group_v22_amd as pkg
    assert pkg.KnapsackBatch is pkg.knapsack_batch.KnapsackBatch
    assert pkg.solve_knapsacks is pkg.knapsack_batch.solve_knapsacks
    for name in ("Solve", "Status", "Z", "SelectedIds", "Rank", "Stats", "Nodes", "IterationLines",
                 "DP", "destroy"):
        assert callable(getattr(pkg.KnapsackBatch, name)), name


def test_python_helpers_are_the_headers_constants():
    from lpr_381_group_v22_amd import knapsack_batch as pykb
    own = open(os.path.join(CSRC, "knapsack_batch_common.hpp")).read()
    common = open(os.path.join(CSRC, "batch_common.hpp")).read()
    assert "kBatchMaxLdsW = (kBatchWgLdsW - kBatchWgScratch) / 4" in common
    assert "kBatchMaxLdsG = ((size_t)160 << 10) - kBatchWgScratch" in common
    assert pykb.MAX_LDS_W == kb.MAX_LDS_W == 16128 and pykb.MAX_LDS_G == kb.MAX_LDS_G == 162816
    assert "kKnapBatchDefaultCap = 1024" in own and pykb.DEFAULT_NODE_CAP == kb.DEFAULT_CAP == 1024
    assert "kKnapBatchMaxCap = (int64_t)1 << 22" in own and pykb.MAX_NODE_CAP == 1 << 22
    assert "kKnapBatchDpMaxCells = (int64_t)1 << 22" in own
    assert pykb.DP_MAX_CELLS == kb.DP_MAX_CELLS >= 1 << 22
    assert "kKnapBatchDpCells = 4" in own and kb.DP_CHUNK_W == 256 and kb.DP_CHUNK_G == 1024
    # the formula is defined once, next to the forms, and the engine picks the form through it
    assert own.count("inline size_t knap_batch_footprint(") == 1
    eng = open(os.path.join(CSRC, "knapsack_batch_engine.hip")).read()
    assert "batch_pick_form(fp, o.variant)" in eng and "knap_batch_footprint(d.n, d.cap)" in eng
    # the product's Python helper against the restatement of DESIGN.md in the cases file
    for n in (1, 6, 64, 65, 128, 129, 200, 8129, 8192):
        for cap in (1, 5, 251, 252, 1024, 2543, 2544, 40000, 1 << 22):
            assert pykb.footprint(n, cap) == kb.footprint(n, cap)
            for variant in (0, 1, 2, 3):
                assert pykb.form_of(n, cap, variant) == kb.form_of(n, cap, variant)
    assert kb.footprint(6, 1) == 64 + 48 and kb.footprint(65, 10) == 10 * 96 + 520


def test_pack_knapsacks():
    from lpr_381_group_v22_amd.knapsack_batch import pack_knapsacks
    p = pack_knapsacks([40, 7], [[11, 8, 6], [3.0]], [[2, 3, 3], [9]], node_cap=[0, 77])
    assert p.capacity.tolist() == [40, 7] and p.n.tolist() == [3, 1]
    assert p.weights.tolist() == [11, 8, 6, 3] and p.values.tolist() == [2, 3, 3, 9]
    assert p.node_cap.tolist() == [0, 77] and p.offsets.tolist() == [0, 3, 4]
    assert pack_knapsacks([1], [[1]], [[1]], node_cap=9).node_cap.tolist() == [9]
    assert pack_knapsacks([1], [[1]], [[1]]).node_cap.tolist() == [0]
    for bad, msg in (
            (dict(capacities=[1, 1], weights=[[1], []], values=[[1], []]), "instance 1: n = 0"),
            (dict(capacities=[1], weights=[[1] * 8193], values=[[1] * 8193]), "n = 8193"),
            (dict(capacities=[1, -1], weights=[[1], [1]], values=[[1], [1]]), "instance 1: capacity"),
            (dict(capacities=[1], weights=[[1, 2]], values=[[1]]), "differ in length"),
            (dict(capacities=[1], weights=[[1]], values=[[1]], node_cap=[(1 << 22) + 1]), "2^22"),
            (dict(capacities=[1], weights=[[1]], values=[[1]], node_cap=[1, 2]), "one entry"),
            (dict(capacities=[], weights=[], values=[]), ">= 1")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            pack_knapsacks(**bad)


def test_main_batch_holds_all_of_knapsack_cases_and_every_form():
    batch = kb.main_batch()
    names = [c["name"] for c in batch]
    assert set(KC.case_names()) <= set(names)
    for c in KC.all_cases():   # at their own caps, unchanged
        assert next(x for x in batch if x["name"] == c["name"]) is c
        assert 600 <= c["node_cap"] <= 40000
    forms = [kb.form_of(len(c["w"]), c["node_cap"]) for c in batch]
    # under the footprint formula every instance of knapsack_cases is form H at its own cap; the
    # instances of lds_cases() put W and G into the same batch
    assert all(kb.form_of(len(c["w"]), c["node_cap"]) == kb.FORM_H for c in KC.all_cases())
    lds = {c["name"]: kb.form_of(len(c["w"]), c["node_cap"]) for c in kb.lds_cases()}
    assert sorted(lds.values()) == [0, 0, 0, 0, 0, 1, 1, 1]
    assert {kb.FORM_W, kb.FORM_G, kb.FORM_H} == set(forms)
    # W packs four per workgroup: the W instances are not a multiple of four
    assert forms.count(kb.FORM_W) % 4 != 0
    ns = [len(c["w"]) for c in batch]
    assert min(ns) == 1 and max(ns) == 8192 and 64 in ns and 65 in ns


def test_lds_cases_finish_or_stop_as_meant():
    want = {"sample_cap5_exact": K.OK, "sample_cap64": K.OK, "sc_s11_n30_cap200": K.NODE_CAP,
            "sc_s12_n40_cap2000": K.NODE_CAP, "sc_s13_n64_cap150": K.NODE_CAP,
            "sc_s13_n65_cap150": K.NODE_CAP, "sc_s14_n130_cap1200": K.NODE_CAP,
            "small_s15_n10_cap1024": K.OK}
    for c in kb.lds_cases():
        r = kb.reference(c)
        assert r["status"] == want[c["name"]], c["name"]
        assert r["evaluated"] <= c["node_cap"]
        if r["status"] == K.NODE_CAP:   # more than the root, and multi-level
            assert r["levels"] >= 3 and r["widest"] >= 8, c["name"]
    # wide levels in form G: more than one 256-lane step of the compaction, nodes of both kinds
    r = kb.reference(next(c for c in kb.lds_cases() if c["name"] == "sc_s12_n40_cap2000"))
    assert r["widest"] > 256
    assert any(W > 256 and 0 < b < W for _, W, b in KC.level_split(r["records"]))
    # three bitmap words in LDS: a critical item past the first word (knapsack_cases' n = 65
    # instances put k there for two words)
    r = kb.reference(next(c for c in kb.lds_cases() if c["name"] == "sc_s14_n130_cap1200"))
    assert max(rec[4] for rec in r["records"]) >= 64


def test_the_sample_meets_its_cap_exactly():
    full = K.branch_and_bound(*kb.SAMPLE)
    assert full["evaluated"] == kb.SAMPLE_EVALUATED == 5 and full["levels"] == 3
    split = KC.level_split(full["records"])
    base, width, _ = split[-1]
    assert base + width == kb.SAMPLE_EVALUATED   # evaluated + width == cap at the last level
    at = kb.reference(kb.sample(5, "_exact"))
    assert at["status"] == K.OK and at["records"] == full["records"]
    below = kb.reference(kb.sample(4))
    assert below["status"] == K.NODE_CAP and below["evaluated"] == 3 and below["levels"] == 2
    assert kb.reference(kb.sample(6))["records"] == full["records"]
    root_only = kb.reference(kb.sample(2))
    assert root_only["status"] == K.NODE_CAP and root_only["evaluated"] == 1


def test_cap_cases_of_the_gpu_test():
    """test 4's instances: E, E - 1 and E + 1, and a cap that stops the search after the root."""
    forms = set()
    for c in kb.cap_cases():
        full = kb.reference(c)
        E = full["evaluated"]
        assert full["status"] == K.OK and full["levels"] >= 4 and 10 < E < c["node_cap"], c["name"]
        at = kb.reference(c, E)
        assert at["status"] == K.OK and at["evaluated"] == E
        assert kb.reference(c, E + 1)["records"] == full["records"]
        less = kb.reference(c, E - 1)
        assert less["status"] == K.NODE_CAP and less["evaluated"] < E
        assert less["records"] == full["records"][:less["evaluated"]]
        root = kb.reference(c, 2)
        assert root["status"] == K.NODE_CAP and root["evaluated"] == 1 and root["levels"] == 1
        forms.add(kb.form_of(len(c["w"]), E))
    assert forms == {kb.FORM_H, kb.FORM_W} or forms == {kb.FORM_H, kb.FORM_G}


def test_limit_and_form_order_cases():
    for c, form in kb.limit_cases():
        n, cap = len(c["w"]), c["node_cap"]
        assert kb.form_of(n, cap) == form, c["name"]
    fp = [kb.footprint(8, cap) for cap in (250, 251, 252, 2542, 2543, 2544)]
    assert fp[1] == kb.MAX_LDS_W and fp[0] == fp[1] - 64 and fp[2] == fp[1] + 64
    assert fp[4] == kb.MAX_LDS_G and fp[3] == fp[4] - 64 and fp[5] == fp[4] + 64
    assert [kb.form_of(len(c["w"]), c["node_cap"]) for c in kb.form_order_cases()] == \
        [kb.FORM_H, kb.FORM_W, kb.FORM_G]
    # forced forms: only where the instance fits
    assert kb.form_of(8, 252, 1) == kb.FORM_G and kb.form_of(8, 251, 3) == kb.FORM_H
    assert kb.form_of(8, 251, 2) == kb.FORM_G and kb.form_of(8, 2544, 2) == kb.FORM_H


def test_dp_edge_cases():
    cases = kb.dp_edge_cases()
    cells = sorted(c["C"] + 1 for c in cases if c["name"].startswith("dp_cells"))
    assert cells == [255, 256, 257, 1023, 1024, 1025, 2015, 2016, 2017, 20351, 20352, 20353]
    assert kb.DP_CELLS_W * 8 == kb.MAX_LDS_W and kb.DP_CELLS_G * 8 == kb.MAX_LDS_G
    by = {c["name"]: c for c in cases}
    assert by["dp_c0"]["C"] == 0 and K.dp(0, by["dp_c0"]["w"], by["dp_c0"]["v"]) == 0
    c = by["dp_w_is_c"]
    assert c["w"][0] == c["C"] and K.dp(c["C"], c["w"], c["v"]) == 1000   # the item alone wins
    c = by["dp_w_is_c_plus_1"]
    assert c["w"][0] == c["C"] + 1 and K.dp(c["C"], c["w"], c["v"]) == 15   # it never fits
    c = by["dp_values_zero"]
    assert K.dp(c["C"], c["w"], c["v"]) == 0
    for c in cases:
        assert c["C"] + 1 <= kb.DP_MAX_CELLS and all(1 <= x < 2 ** 31 for x in c["w"])
