"""CPU tests of the batched Branch & Bound: the ABI, the ctypes binding and the
C# binding declare the lpr_bb_batch_* calls, the kernels build for gfx950 without scratch and within
their LDS, pack_roots packs and refuses as lpr_bb_batch_create does, and option3_models builds the
models program._append_unit_bound_rows does, without touching the caller's parsers."""
import os
import re
import subprocess

import numpy as np
import pytest

import bb_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

BB_BATCH_CALLS = ["lpr_bb_batch_create", "lpr_bb_batch_from_batch", "lpr_bb_batch_destroy",
                  "lpr_bb_batch_run", "lpr_bb_batch_result_read", "lpr_bb_batch_solution_read",
                  "lpr_bb_batch_records_read", "lpr_bb_batch_pop_order_read",
                  "lpr_bb_batch_trace_read"]


def test_header_and_bindings_declare_the_bb_batch_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    gs = open(os.path.join(ROOT, "integration", "csharp", "GpuSolvers.cs")).read()
    for name in BB_BATCH_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"static extern \w+ " + name + r"\(", cs)) == 1, name
        assert "NativeMethods." + name + "(" in gs, name
    assert "typedef struct lpr_bb_batch lpr_bb_batch;" in text
    assert "class BranchAndBoundBatch" in gs
    # every status-returning call of the wrapper is checked
    body = gs[gs.index("class BranchAndBoundBatch"):gs.index("class RevisedPrimalSimplexSolver")]
    for call in re.findall(r"(.{0,40})NativeMethods\.(lpr_bb_batch_\w+)\(", body):
        assert "ThrowIfError(" in call[0], call


def test_ctypes_structs_match_the_header():
    from lpr_381_group_v22_amd import _native as N
    assert [f for f, _ in N.BBBatchOpts._fields_] == ["enable_pruning", "chunk", "variant",
                                                      "max_child_pivots"]
    assert [f for f, _ in N.BBBatchResult._fields_] == ["done", "node_cap", "pivot_limit",
                                                        "launches", "pops", "pivots"]
    assert C_sizeof(N.BBBatchOpts) == 16 and C_sizeof(N.BBBatchResult) == 32


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_bb_batch_kernels_build_without_scratch(tmp_path):
    """bb_batch_kernels.hip alone, for gfx950, with the Makefile's flags: every kernel has a private
    segment of 0 bytes (no spills) and its static LDS leaves its form's dynamic share within
    160 KiB."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "bb_batch_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-fno-fast-math", "-DLPR_BUILD", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "bb_batch_kernels.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    s = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", s, flags=re.S)
    names = [k for k, _ in kernels]
    assert sum("k_bb_batchIL" in k for k in names) == 3, names
    assert any("k_bb_batch_load" in k for k in names)
    assert any("k_bb_batch_reset" in k for k in names)
    for name, body in kernels:
        priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert priv == 0, (name, priv)
        assert lds <= 1024, (name, lds)  # the reserved workgroup scratch (kBatchWgScratch)
        assert lds + 159 * 1024 <= 160 * 1024


def test_sample_model_takes_form_w():
    """The sample model's root is 8 x 14; at node cap 20 its pair and factor column are
    2 * 28 * 34 + 28 doubles, within a quarter of 63 KiB."""
    fp = 8 * (2 * 28 * 34 + 28)
    assert fp <= (64 * 1024 - 1024) // 4
    assert '#include "batch_common.hpp"' in open(os.path.join(CSRC, "bb_batch_common.hpp")).read()
    src = open(os.path.join(CSRC, "batch_common.hpp")).read()  # the one owner of the form limits
    assert "constexpr size_t kBatchMaxLdsW = (kBatchWgLdsW - kBatchWgScratch) / 4;" in src


def test_pack_roots_packs_and_refuses():
    from lpr_381_group_v22_amd.bb_batch import pack_roots
    a = np.arange(8 * 14, dtype=np.float64).reshape(8, 14)
    b = np.arange(6 * 10, dtype=np.float64).reshape(6, 10) * 0.5
    p = pack_roots([a, b], [6, 4])
    assert p.rows.tolist() == [8, 6] and p.cols.tolist() == [14, 10]
    assert p.nvars.tolist() == [6, 4] and p.nvars.dtype == np.int32
    assert p.tableaux.tobytes() == np.concatenate([a.reshape(-1), b.reshape(-1)]).tobytes()
    assert pack_roots([np.zeros((1004, 3))], [1], node_cap=20).rows.tolist() == [1004]
    bad = [
        ([], []),                          # no IPs
        ([a], [6, 4]),                     # counts differ
        ([a], [14]),                       # nvars > cols - 1
        ([a], [-1]),
        ([np.zeros(5)], [1]),              # not 2-D
        ([np.zeros((3, 1))], [0]),         # cols < 2
        ([np.zeros((1005, 3))], [1]),      # rows + 20 > 1024
        ([np.zeros((2, 2029))], [1]),      # cols + 20 > 2048
    ]
    for tabs, nv in bad:
        with pytest.raises(ValueError):
            pack_roots(tabs, nv)
    with pytest.raises(ValueError):
        pack_roots([a], [6], node_cap=65)
    assert pack_roots([a], [6], node_cap=64).rows.tolist() == [8]


def test_option3_models_match_append_unit_bound_rows():
    from lpr_381_group_v22_amd import Constraint, InputFileParser
    from lpr_381_group_v22_amd.bb_batch import option3_models
    from lpr_381_group_v22_amd.program import _append_unit_bound_rows
    parsers = []
    for _, (obj, cons) in bb_cases.all_bb_cases():
        raw = cons[:len(cons) - len(obj)]
        parsers.append(InputFileParser(ProblemType="max", ObjectiveCoefficients=list(obj),
                                       Constraints=[Constraint(list(c.Coefficients), c.Relation,
                                                               c.RHS) for c in raw]))
    before = [[(list(c.Coefficients), c.Relation, c.RHS) for c in p.Constraints] for p in parsers]
    models = option3_models(parsers)
    after = [[(list(c.Coefficients), c.Relation, c.RHS) for c in p.Constraints] for p in parsers]
    assert after == before  # the caller's parsers are untouched
    for p, (obj, cons, is_max) in zip(parsers, models):
        _append_unit_bound_rows(p)
        assert is_max is True and obj == list(p.ObjectiveCoefficients)
        assert [(list(c.Coefficients), c.Relation, c.RHS) for c in cons] == \
               [(list(c.Coefficients), c.Relation, c.RHS) for c in p.Constraints]
