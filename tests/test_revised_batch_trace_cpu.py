"""CPU tests of the traced revised-simplex batch: the ABI declares the four
lpr_rev_batch_trace_* calls and the bindings have and use them, the record layout restated in
revised_batch.py is the oracle's and the header's, the traced kernels build for gfx950 without
scratch and within the workgroup's LDS, and the constructed inputs of the GPU tests do what those
tests rely on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import revised_batch_cases as rc
from test_oracle_revised import flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

CALLS = ["lpr_rev_batch_trace_reserve", "lpr_rev_batch_trace_info", "lpr_rev_batch_trace_read",
         "lpr_rev_batch_trace_read_all"]


def test_header_and_bindings_declare_and_use_the_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    gs = open(os.path.join(ROOT, "integration", "csharp", "GpuSolvers.cs")).read()
    py = open(os.path.join(ROOT, "lpr_381_group_v22_amd", "revised_batch.py")).read()
    eng = open(os.path.join(CSRC, "rev_batch_engine.hip")).read()
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"\b" + name + r"\s*\(", cs)) == 1, name
        assert "NativeMethods." + name + "(" in gs, name
        assert "N.lib." + name + "(" in py, name
        assert re.search(r"^int " + name + r"\(", eng, flags=re.M), name
    assert "public List<string> IterationSnapshots(int k)" in gs
    # opts and result keep their fields: the trace is a property of the handle
    assert [f for f, _ in N.RevBatchOpts._fields_] == ["max_pivots", "chunk", "variant"]


def test_record_layout_is_the_oracles(oracle):
    from lpr_381_group_v22_amd import revised_batch as rb
    oracle.lib.orc_revised_trace_stride.restype = C.c_int64
    grid = [(1, 1), (12, 1), (1, 8), (64, 48), (3, 4), (8, 8), (20, 33), (1024, 1023)]
    for n, m in grid:
        assert rb.trace_stride(m, n) == oracle.lib.orc_revised_trace_stride(n, m), (n, m)
        assert rb.trace_stride(m, n) == 6 + 7 * m + n + m * n + m * m
        at = len(rb.TRACE_SCALARS)
        for name, ln in (("y", m), ("rcX", n), ("rcS", m), ("u_pre", m), ("ratios_pre", m),
                         ("basis_pre", m), ("basis_post", m), ("xB", m), ("BInvA", m * n),
                         ("BInv", m * m)):  # the order of oracle_lib.revised_trace
            assert rb.trace_offsets(m, n)[name] == (at, ln), (n, m, name)
            at += ln
    assert rb.TRACE_SCALARS == ("entering", "leaving_row", "leaving_var", "rc_pre", "z_working",
                                "z_original")
    # a raw oracle record read through the restated layout is the oracle's own dict
    obj, cons, is_min = dict(rc.models())["sample_option2"]
    A, b = flat(cons)
    tr = oracle.revised_trace(obj, A, b, is_min, cap=8)
    m, n = A.shape
    S = rb.trace_stride(m, n)
    buf = np.zeros(8 * S)
    ns, it = C.c_int64(), C.c_int64()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    oracle.lib.orc_revised_solve_trace(
        n, m, dp(np.asarray(obj, dtype=np.float64)), dp(A), dp(b), 1 if is_min else 0,
        C.c_int64(0), None, None, None, dp(buf), C.c_int64(8), C.byref(ns), C.byref(it))
    assert ns.value == tr["count"] == 7
    for i, want in enumerate(tr["snapshots"]):
        got = rb.trace_record(buf[i * S:(i + 1) * S], m, n)
        assert sorted(got) == sorted(want)
        for key in want:
            assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), (i, key)


def test_header_states_the_layout_once_and_the_kernels_use_it():
    own = open(os.path.join(CSRC, "rev_batch_common.hpp")).read()
    body = open(os.path.join(CSRC, "rev_batch_body.hpp")).read()
    eng = open(os.path.join(CSRC, "rev_batch_engine.hip")).read()
    assert own.count("constexpr int64_t rev_trace_stride(") == 1
    for f in ("y", "rcx", "rcs", "u", "ratios", "basis_pre", "basis_post", "xb", "binva", "binv"):
        assert own.count("constexpr int64_t rev_trace_%s(" % f) == 1, f
        assert "rev_trace_%s(m, n)" % f in body, f
    assert "rev_trace_stride(m, n)" in body and "rev_trace_stride(d.m, d.n)" in eng
    # no literal restatement of the stride outside the header
    assert "7 * m" not in body and "7 * m" not in eng
    # the trace adds nothing to the LDS footprint: one form rule, one footprint, for both kernels
    assert eng.count("rev_batch_footprint(d.m, d.n)") == 1
    assert "rev_batch_run<NT, kLds, false>" in open(
        os.path.join(CSRC, "rev_batch_kernels.hip")).read()
    assert "rev_batch_run<NT, kLds, true>" in open(
        os.path.join(CSRC, "rev_batch_trace_kernels.hip")).read()


def test_trace_kernels_build_without_scratch(tmp_path):
    """rev_batch_trace_kernels.hip alone, for gfx950, with the Makefile's flags: three kernels,
    each with a private segment of 0 bytes (no spills to scratch) and static LDS within the
    workgroup scratch the forms leave free (kBatchWgScratch)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "rev_batch_trace_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-fno-fast-math", "-DLPR_BUILD", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "rev_batch_trace_kernels.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    s = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", s, flags=re.S)
    names = [k for k, _ in kernels]
    assert len(names) == 3 and all("k_rev_batch_traceI" in k for k in names), names
    for name, body in kernels:
        priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert priv == 0, (name, priv)
        assert lds <= 1024, (name, lds)


def _trace(oracle, model, max_iter=rc.CAP, cap=8):
    obj, cons, is_min = model
    A, b = flat(cons)
    return oracle.revised_trace(obj, A, b, is_min, max_iter=max_iter, cap=cap)


def test_constructed_inputs_do_what_the_gpu_tests_rely_on(oracle):
    from lpr_381_group_v22_amd import revised_batch as rb
    for args, form, count in (((12, 5, 6, 21), 0, 1), ((20, 6, 10, 16), 0, 2),
                              ((70, 12, 10, 2), 1, 1)):
        mdl = rc.duplicated_rows(*args)
        tr = _trace(oracle, mdl)
        assert (tr["status"], tr["count"], tr["iterations"]) == (2, count, count), args
        assert rb.pick_form(len(mdl[1]), len(mdl[0])) == form, args
    for seed, count in ((10, 3), (15, 2), (24, 2)):
        rng = np.random.RandomState(seed)
        A = np.round(rng.uniform(-2, 3, (3, 4)), 1)
        b = np.round(rng.uniform(1, 9, 3), 1)
        c = np.round(rng.uniform(0.5, 5, 4), 1)
        tr = oracle.revised_trace(c, A, b, False, max_iter=rc.CAP, cap=8)
        assert (tr["status"], tr["count"]) == (1, count), seed
    by = dict(rc.models() + rc.degenerate_models())
    for name, count in (("sample_option2", 7), ("klee_minty_8", 256), ("unbounded", 0),
                        ("infeasible_basis", 0), ("zero_objective", 1), ("zero_A", 0),
                        ("m1_n12", 3)):
        assert _trace(oracle, by[name], cap=1)["count"] == count, name
    tr = _trace(oracle, by["klee_minty_8"], max_iter=7, cap=16)
    assert (tr["status"], tr["count"]) == (5, 7)
    # -0.0 in A with B^-1 = I: MultiplyMatrices starts every sum at +0.0
    tr = _trace(oracle, rc.to_model([0.0, 0.0], [[-0.0, 1.0], [2.0, -0.0]], [1.0, 1.0]))
    assert (tr["status"], tr["count"]) == (0, 1)
    opt = tr["snapshots"][0]
    assert opt["entering"] == -1 and not np.signbit(opt["BInvA"]).any()
    assert not opt["u_pre"].any() and not np.signbit(opt["u_pre"]).any()
    assert np.isposinf(opt["ratios_pre"]).all()
    assert opt["basis_pre"].tolist() == opt["basis_post"].tolist() == [2, 3]
    tr = _trace(oracle, rc.ieee_div_model())
    assert float(tr["snapshots"][0]["BInv"][1][0]).hex() == "-0x1.6666666666667p-2"
