"""CPU tests of the traced primal batch: the ABI declares the four
lpr_batch_trace_* calls and the bindings have and use them, the record layout is stated once and
used by the kernels and the engine, the traced kernels build for gfx950 without scratch and within
the untraced kernels' LDS, a host-only sanitizer program walks every index of the layout, the
constructed inputs of the GPU tests do what those tests rely on, and the shared formatter gives
the restatement's text from the oracle's numbers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import batch_trace_cases as tc
import lp_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

CALLS = ["lpr_batch_trace_reserve", "lpr_batch_trace_info", "lpr_batch_trace_read",
         "lpr_batch_trace_read_all"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_and_bindings_declare_and_use_the_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", _read(HEADER), flags=re.S)
    cs = _read(ROOT, "integration", "csharp", "NativeMethods.cs")
    gs = _read(ROOT, "integration", "csharp", "GpuSolvers.cs")
    py = _read(ROOT, "lpr_381_group_v22_amd", "primal_batch.py")
    eng = _read(CSRC, "batch_engine.hip")
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"\b" + name + r"\s*\(", cs)) == 1, name
        assert "NativeMethods." + name + "(" in gs, name
        assert "N.lib." + name + "(" in py, name
        assert re.search(r"^int " + name + r"\(", eng, flags=re.M), name
    snaps = "public List<string> IterationSnapshots(int k)"
    assert snaps in gs and "TableIterationFormater.Format(" in gs.split(snaps)[1]
    # opts and result keep their fields: the trace is a property of the handle
    assert [f for f, _ in N.BatchOpts._fields_] == ["max_pivots", "chunk", "variant"]
    assert [f for f, _ in N.BatchResult._fields_] == ["optimal", "unbounded", "limit", "launches",
                                                       "pivots"]
    # the descriptor other engines read through batch_view keeps its size
    assert "static_assert(sizeof(BatchDesc) == 72" in _read(CSRC, "batch_common.hpp")
    assert "keeps no iteration snapshots" not in py


def test_layout_is_stated_once_and_used():
    from lpr_381_group_v22_amd import primal_batch as pb
    own = _read(CSRC, "batch_common.hpp")
    body = _read(CSRC, "batch_body.hpp")
    eng = _read(CSRC, "batch_engine.hip")
    for f in ("stride", "tab", "row", "col"):
        assert len(re.findall(r"constexpr int64_t batch_trace_%s\(" % f, own)) == 1, f
    assert "batch_trace_stride(R, C)" in body and "batch_trace_tab()" in body
    assert "batch_trace_row()" in body and "batch_trace_col()" in body
    assert "batch_trace_stride(d.rows, d.cols)" in eng
    # no literal restatement of the stride outside the header
    for text in (body, eng):
        code = re.sub(r"//.*", "", text)
        assert not re.search(r"2\s*\+\s*\(?\s*(\(\w+\))?\s*(rows|R|d\.rows)\s*\*", code)
    assert "batch_simplex_run<NT, kLds, false>" in _read(CSRC, "batch_kernels.hip")
    assert "batch_simplex_run<NT, kLds, true>" in _read(CSRC, "batch_trace_kernels.hip")
    assert "k_batch_trace_first" in _read(CSRC, "batch_trace_kernels.hip")
    # the trace adds nothing to the LDS footprint: one form rule, one footprint, both kernels
    assert eng.count("batch_footprint(") == 1
    # the restatement in the mirror
    for rows, cols in ((1, 2), (3, 4), (64, 318), (1024, 2048)):
        assert pb.trace_stride(rows, cols) == 2 + rows * cols
    assert (pb.TRACE_ROW, pb.TRACE_COL, pb.TRACE_TAB) == (0, 1, 2)
    r, e, T = pb.trace_record(np.arange(8.0), 2, 3)
    assert (r, e) == (0, 1) and T.tolist() == [[2.0, 3.0, 4.0], [5.0, 6.0, 7.0]]


def _kernels(hipcc, src, out):
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-fno-fast-math", "-DLPR_BUILD", "--cuda-device-only", "-S",
                    os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True)
    found = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", out.read_text(),
                       flags=re.S)
    res = {}
    for name, body in found:
        res[name] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                     int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)))
    return res


def test_trace_kernels_build_without_scratch(tmp_path):
    """batch_trace_kernels.hip alone, for gfx950, with the Makefile's flags: the three solve
    kernels have a private segment of 0 bytes and no more static LDS than k_batch_simplex has in
    the same build of batch_kernels.hip."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    traced = _kernels(hipcc, "batch_trace_kernels.hip", tmp_path / "batch_trace_kernels.s")
    plain = _kernels(hipcc, "batch_kernels.hip", tmp_path / "batch_kernels.s")
    solve = {k: v for k, v in traced.items() if "k_batch_simplex_traceI" in k}
    base = {k: v for k, v in plain.items() if "k_batch_simplexI" in k}
    assert len(solve) == 3 and len(base) == 3, (sorted(traced), sorted(plain))
    assert any("k_batch_trace_first" in k for k in traced)
    form = lambda k: re.search(r"ILi(\d+)ELb(\d)E", k).groups()
    for name, (priv, lds) in solve.items():
        twin = [v for k, v in base.items() if form(k) == form(name)]
        assert len(twin) == 1, name
        assert priv == 0, (name, priv)
        assert lds <= twin[0][1], (name, lds, twin[0][1])


def test_layout_walk_under_sanitizers(tmp_path):
    """tools/batch_trace_check.cpp, a stand-alone host program built with the address and
    undefined-behaviour sanitizers: every index of the layout and the lane walk over an exactly
    sized buffer, every cell of every kept record written exactly once."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "batch_trace_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "batch_trace_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert re.search(r"batch_trace_check: \d+ batches, 0 failures", p.stdout), tail
    assert "runtime error" not in tail, tail


def test_constructed_inputs_do_what_the_gpu_tests_rely_on(oracle):
    """Conditions on the case list, computed with the oracle alone.  The one thing taken from the
    package is the mirror's restated stride: the slab sizes the GPU tests assume (SHAPE_PIVOTS
    keeps the G and H slabs in the low megabytes) are formed with it."""
    from lpr_381_group_v22_amd import primal_batch as pb
    names = [n for n, _ in tc.all_cases()]
    tableaux = [tc.built(oracle, c) for _, c in tc.all_cases()]
    refs = tc.refs_of(oracle, "cases", tableaux)
    by = dict(zip(names, refs))
    # the slab of the batch of every case, and of the largest threshold shape, in bytes
    strides = [pb.trace_stride(*T.shape) for T in tableaux]
    assert strides == [2 + T.size for T in tableaux]
    assert 8 * tc.TRACE_CAP * sum(strides) < 32 << 20
    m, n = tc.THRESHOLDS[-1]
    assert 8 * (tc.SHAPE_PIVOTS + 2) * pb.trace_stride(m + 1, n + m + 1) < 2 << 20
    statuses = {r["status"] for r in refs}
    assert {tc.OPTIMAL, tc.UNBOUNDED} <= statuses and tc.LIMIT not in statuses
    assert (by["zero_pivot"]["status"], by["zero_pivot"]["pivots"]) == (tc.OPTIMAL, 0)
    assert by["unbounded_later"]["status"] == tc.UNBOUNDED and by["unbounded_later"]["pivots"] >= 1
    assert by["unbounded"]["status"] == tc.UNBOUNDED
    # the three form models land in W, G, H
    forms = [tc.form_of(*tc.built(oracle, c).shape) for _, c in tc.form_models()]
    assert forms == [0, 1, 2]
    assert [tc.form_of(m + 1, n + m + 1) for m, n in tc.THRESHOLDS] == [0, 1, 1, 2]
    # and make at least SHAPE_PIVOTS pivots, so that the limit of the shape tests is met
    for name, _ in tc.form_models()[1:]:
        assert by[name]["pivots"] >= tc.SHAPE_PIVOTS, name
    # the cap-test LP makes more pivots than that test's trace_cap holds
    cap = tc.step_records(oracle, tc.built(oracle, tc.cap_lp()), keep=tc.SMALL_TRACE_CAP)
    assert cap["pivots"] + 1 > tc.SMALL_TRACE_CAP and len(cap["records"]) == tc.SMALL_TRACE_CAP
    # with trace_cap = TRACE_CAP at least three quarters of the cases keep all their records
    whole = [1 + r["pivots"] <= tc.TRACE_CAP for r in refs]
    assert 4 * sum(whole) >= 3 * len(whole), whole
    assert not all(whole)  # and one does not
    # the -0.0 tableau: one pivot, and the -0.0 under the pivot row's -2 becomes +0.0
    T, _ = tc.negative_zero_tableau()
    nz = tc.step_records(oracle, T)
    assert nz["pivots"] == 1 and np.signbit(nz["records"][0][2][2, 1])
    assert not np.signbit(nz["records"][1][2][2, 1])


@pytest.mark.parametrize("name", ["sample", "unbounded_later"])
def test_formatter_on_oracle_tableaux_is_the_restatement(oracle, name):
    """format_snapshots and format_console fed the oracle's stepped tableaux (numpy arrays, no
    device) against the independent restatement tests/ref_py_text.py."""
    from lpr_381_group_v22_amd.primal_simplex_solver import format_console, format_snapshots
    from ref_py_text import PyPrimalText
    obj, cons, mx = lp_cases.sample_option1() if name == "sample" else tc.unbounded_later_lp()
    ref = PyPrimalText(obj, cons, mx)
    snaps, console = ref.solve_text()
    st = tc.step_records(oracle, tc.built(oracle, (obj, cons, mx)))
    n = len(obj)
    x, z = oracle.extract_solution(st["T"], n)
    sol = [float(v) for v in x] if st["status"] == tc.OPTIMAL else None
    z = z if st["status"] == tc.OPTIMAL else 0.0
    got = format_snapshots([T for _, _, T in st["records"]], n, st["status"], st["T"], z, sol)
    assert len(got) == len(snaps) == 1 + st["pivots"] + 1
    assert got == snaps
    assert format_console(st["records"], n, st["status"], z, sol) == console
    assert ref.status == ("optimal" if name == "sample" else "unbounded")
