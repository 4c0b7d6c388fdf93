"""CPU tests of the narrated cutting-plane batch: the ABI declares the
lpr_cut_batch_narrate_* calls and the bindings have and use them; the text restatement
(tests/ref_py_cut_text.py) gives the oracle's exit code, cuts, log and final tableau for every
fixture of the GPU tests, and only then is the reference for events, blocks and text; the shared
formatter gives the restatement's text from the restatement's numbers; "0.####" and "0.###" on
constructed values; TableIterationFormater.Format with numVars <= 0; the layout rules against a
list model; the host-only walker under sanitizers; the narrated kernels build for gfx950 without
scratch and within their twins' LDS while cut_batch_kernels.hip keeps exactly the kernels it had."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cut_batch_cases as cbc
import cut_cases
import ref_py_cut_text as rt
from ref_py_text import CRLF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")
TEXTBOOK_MAX_CUTS = 20

CALLS = ["lpr_cut_batch_narrate_reserve", "lpr_cut_batch_narrate_info",
         "lpr_cut_batch_narrate_events_read", "lpr_cut_batch_narrate_data_read",
         "lpr_cut_batch_narrate_read_all"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def lf(text):
    return text.replace(CRLF, "\n")


def test_header_and_bindings_declare_and_use_the_calls():
    from lpr_381_group_v22_amd import _native as N
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", _read(HEADER), flags=re.S)
    cs = _read(ROOT, "integration", "csharp", "NativeMethods.cs")
    gs = _read(ROOT, "integration", "csharp", "GpuSolvers.cs")
    py = _read(ROOT, "lpr_381_group_v22_amd", "cut_batch.py")
    eng = _read(CSRC, "cut_batch_engine.hip")
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"\b" + name + r"\s*\(", cs)) == 1, name
        assert "NativeMethods." + name + "(" in gs, name
        assert "N.lib." + name + "(" in py, name
        assert re.search(r"^int " + name + r"\(", eng, flags=re.M), name
    assert "public string Narration(int k)" in gs and "public void Narrate(" in gs
    # opts, result and the descriptor stay: narration is a property of the handle
    assert ctypes.sizeof(N.CutBatchOpts) == 32 and ctypes.sizeof(N.CutBatchResult) == 64
    # one text of the state machine, expanded inside both kernels; one computation of the update
    plain, narr = _read(CSRC, "cut_batch_kernels.hip"), _read(CSRC, "cut_batch_narr_kernels.hip")
    body = _read(CSRC, "cut_batch_body.hpp")
    for src, flag in ((plain, "constexpr bool kNarr = false;"), (narr, "constexpr bool kNarr = true;")):
        assert flag in src and src.count('#include "cut_batch_body.hpp"') == 2
        assert src.count("#define LPR_CUT_BATCH_BODY_TEXT") == 1
    assert body.count("f * prow[jj[u]]") == 1 and body.count("staged_eps_fold(") == 5
    assert "staged_eps_fold(" not in _read(CSRC, "cut_batch_kernels.hip")
    layout, rule = _read(CSRC, "cut_narr_layout.hpp"), _read(CSRC, "kept_prefix.hpp")
    assert "hip/" not in layout and "hip/" not in rule
    assert "kept_push(" in rule and "_push(" not in layout
    assert "constexpr int64_t cut_narr_event_doubles(" in layout


# ---- the restatement is the oracle's equal, fixture by fixture -------------------------------------
def _same_as_oracle(n, code, ref, cuts=None):
    assert code == ref["code"]
    if cuts is not None:
        assert cuts == ref["cuts"]
    assert n.log == ref["log"]
    assert np.array(n.table()).tobytes() == ref["T"].tobytes()
    assert sum(1 for e in n.events if e[0] >= rt.EV_PIVOT) == len(ref["log"])


def test_restatement_equals_the_oracle_on_the_textbook_items(oracle):
    codes = set()
    for name, T in cbc.textbook_items(oracle):
        ref = cbc.reference(oracle, cbc.MODE_CUT, T, max_cuts=TEXTBOOK_MAX_CUTS)
        n, code, cuts = rt.narrate_cutting_plane(T, TEXTBOOK_MAX_CUTS)
        _same_as_oracle(n, code, ref, cuts)
        assert not n.stopped, name   # every one ends where the C# can
        codes.add(code)
    assert len(cbc.textbook_items(oracle)) == 12 and codes == {0, 1, 2, 4, 5}


def test_restatement_equals_the_oracle_on_the_solver_items(oracle):
    for mode, tabs in ((cbc.MODE_DUAL, cut_cases.dual_tableaux(oracle)),
                       (cbc.MODE_PRIMAL2, cut_cases.primal2_tableaux(oracle))):
        assert len(tabs) == (16 if mode == cbc.MODE_DUAL else 7)
        for name, T in tabs:
            for steps in (True, False):
                ref = cbc.reference(oracle, mode, T, print_steps=steps)
                n, st = rt.narrate_solve(T, mode, print_steps=steps)
                _same_as_oracle(n, st, ref)
    assert any(rt.narrate_solve(T, 2)[1] == rt.UNBOUNDED
               for _, T in cut_cases.primal2_tableaux(oracle))


def test_restatement_equals_the_oracle_on_the_large_and_nan_items(oracle):
    for (T, mc), outcome in ((cbc.g_item(), cbc.G_ITEM_OUTCOME), (cbc.h_item(), cbc.H_ITEM_OUTCOME)):
        ref = cbc.reference(oracle, cbc.MODE_CUT, T, max_cuts=mc)
        n, code, cuts = rt.narrate_cutting_plane(T, mc, text=False)
        _same_as_oracle(n, code, ref, cuts)
        assert (code, cuts, len(n.log)) == outcome and n.stopped
    for mode, T, victim, col in cbc.nan_factor_cases(oracle):
        ref = cbc.reference(oracle, mode, T, hard_cap=50)
        n, st = rt.narrate_solve(T, mode, print_steps=mode == cbc.MODE_DUAL, hard_cap=50)
        _same_as_oracle(n, st, ref)
    for hard_cap in (1, 2):
        for name, T in cbc.textbook_items(oracle)[:6]:
            ref = cbc.reference(oracle, cbc.MODE_CUT, T, max_cuts=TEXTBOOK_MAX_CUTS,
                                hard_cap=hard_cap)
            n, code, cuts = rt.narrate_cutting_plane(T, TEXTBOOK_MAX_CUTS, hard_cap=hard_cap)
            _same_as_oracle(n, code, ref, cuts)


# ---- the formatter on the restatement's numbers ----------------------------------------------------
def test_formatter_on_restatement_numbers_is_the_restatement_text(oracle):
    from lpr_381_group_v22_amd.cut_batch import (NarrationStopped, format_cutting_plane,
                                                 format_primal2_snapshots)
    for name, T in cbc.textbook_items(oracle):
        n, code, _ = rt.narrate_cutting_plane(T, TEXTBOOK_MAX_CUTS)
        text = format_cutting_plane(n.events, n.record0, n.blocks, newline=CRLF)
        assert lf(text) == lf(n.text) and len(text) > 100, name
        assert text.startswith("Initial tableau:" + CRLF + "z:  ")
    for mode, tabs in ((1, cut_cases.dual_tableaux(oracle)), (2, cut_cases.primal2_tableaux(oracle))):
        for name, T in tabs:
            for steps in (True, False):
                n, _ = rt.narrate_solve(T, mode, print_steps=steps)
                text = format_cutting_plane(n.events, n.record0, n.blocks, newline=CRLF)
                assert lf(text) == lf(n.text), (name, steps)
                assert (text == "") == (not steps)
                if mode == 2:
                    assert format_primal2_snapshots(n.events, n.record0, n.blocks) == n.snapshots
                    assert n.snapshots[0].startswith("Start of iter 0" + CRLF + "Current Tableau:")
    # no C# text: the cut limit and a hard_cap stop raise, partial gives the restatement's prefix
    T = cbc.textbook_items(oracle)[3][1]
    for kw in (dict(max_cuts=2), dict(max_cuts=TEXTBOOK_MAX_CUTS, hard_cap=1)):
        n, code, _ = rt.narrate_cutting_plane(T, **kw)
        assert n.stopped
        with pytest.raises(NarrationStopped):
            format_cutting_plane(n.events, n.record0, n.blocks)
        part = format_cutting_plane(n.events, n.record0, n.blocks, newline=CRLF, partial=True)
        assert len(part) > 1000 and lf(n.text).startswith(lf(part))
    # a missing block stops the text there
    n, _, _ = rt.narrate_cutting_plane(T, TEXTBOOK_MAX_CUTS)
    with pytest.raises(NarrationStopped):
        format_cutting_plane(n.events, n.record0, n.blocks[:3])
    part = format_cutting_plane(n.events, n.record0, n.blocks[:3], newline=CRLF, partial=True)
    assert lf(n.text).startswith(lf(part)) and 0 < len(part) < len(n.text)


def test_max_iterations_line_of_both_solvers(oracle):
    from lpr_381_group_v22_amd.cut_batch import format_cutting_plane, format_primal2_snapshots
    for mode, tabs in ((1, cut_cases.dual_tableaux(oracle)), (2, cut_cases.primal2_tableaux(oracle))):
        T = next(T for _, T in tabs if len(cbc.reference(oracle, mode, T)["log"]) >= 2)
        ref = cbc.reference(oracle, mode, T, max_iters=1, print_steps=True)
        n, st = rt.narrate_solve(T, mode, max_iters=1, print_steps=True)
        _same_as_oracle(n, st, ref)
        assert st == rt.LIMIT and n.text.endswith("Max iterations reached." + CRLF)
        assert lf(format_cutting_plane(n.events, n.record0, n.blocks)) == lf(n.text)
        if mode == 2:  # :90 returns behind the pivot: no "Start of iter 1"
            assert format_primal2_snapshots(n.events, n.record0, n.blocks) == n.snapshots
            assert len(n.snapshots) == 3


# ---- number formats --------------------------------------------------------------------------------
def test_custom_formats_on_constructed_values():
    from lpr_381_group_v22_amd import table_iteration_formater as f
    cases4 = [(0.12345, "0.1235"), (-0.12345, "-0.1235"), (2.00005, "2.0001"), (1.00015, "1.0002"),
              (0.00005, "0.0001"), (-0.00004, "0"), (-0.0, "0"), (0.0, "0"), (1e15, "1" + "0" * 15),
              (1.5, "1.5"), (-2.0, "-2"), (0.1 + 0.2, "0.3"), (float("nan"), "NaN"),
              (float("inf"), "Infinity"), (float("-inf"), "-Infinity"),
              # 15 significant digits first: the 16th digit of 0.30000000000000004 is gone, and a
              # value one ulp below a midpoint rounds up once its 15-digit image is the midpoint
              (0.30000000000000004, "0.3"), (np.nextafter(0.12345, 0.0), "0.1235"),
              (123456789012.34565, "123456789012.346"), (99999.99995, "100000"),
              (12345678901234.56, "12345678901234.6")]
    for v, want in cases4:
        assert f.H4(float(v)) == want, (v, f.H4(float(v)), want)
        assert rt.py_hashes(float(v), 4) == want, (v, rt.py_hashes(float(v), 4), want)
    cases3 = [(2.0005, "2.001"), (-2.0005, "-2.001"), (-0.0004, "0"), (0.0005, "0.001"),
              (1e15, "1" + "0" * 15), (15.4, "15.4"), (float("nan"), "NaN"),
              (float("-inf"), "-Infinity"), (np.nextafter(2.0005, 0.0), "2.001"),
              (1234567890123.4565, "1234567890123.46")]
    for v, want in cases3:
        assert f.H3(float(v)) == want == f._custom_0_hashes(float(v)), (v, f.H3(float(v)))
        assert rt.py_hashes(float(v), 3) == want, v
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.normal(size=4000) * 10.0 ** rng.integers(-6, 14, 4000),
                           np.round(rng.normal(size=2000) * 100, 4) + 0.00005])
    for v in vals:
        assert f.H4(float(v)) == rt.py_hashes(float(v), 4), v
        assert f.H3(float(v)) == rt.py_hashes(float(v), 3), v


def test_format_with_zero_and_negative_num_vars():
    """DualSimplex.cs:228-234 gives cols - 1 - constraints, which shrinks with every cut: the two
    label loops of TableIterationFormater.Format (:32-33) are restated as they are."""
    from lpr_381_group_v22_amd import table_iteration_formater as f
    from ref_py_text import py_format_table
    t = np.array([[1.0, -2.0, 0.5, 3.0], [0.0, 1.0, 2.0005, -4.0]])
    zero = f.Format(t, 0, "Dual Simplex Tableau")
    assert "Table\tt1\tt2\tt3\tRHS" + CRLF in zero and "x1" not in zero
    neg = f.Format(t, -2, "Dual Simplex Tableau")
    assert "Table\tt1\tt2\tt3\tt4\tt5\tRHS" + CRLF in neg   # j runs from -2: five labels, four columns
    for nv in (0, -2):
        assert f.Format(t, nv, "Dual Simplex Tableau") == py_format_table(t.tolist(), nv,
                                                                         "Dual Simplex Tableau")


# ---- layout ----------------------------------------------------------------------------------------
def test_layout_functions_against_a_list_model(oracle):
    from lpr_381_group_v22_amd import cut_batch as cb
    assert (cb.EV_CALL, cb.EV_LEVEL, cb.EV_CUT, cb.EV_SOLVE_BEGIN, cb.EV_SOLVE_END, cb.EV_EXIT,
            cb.EV_PIVOT) == (rt.EV_CALL, rt.EV_LEVEL, rt.EV_CUT, rt.EV_SOLVE_BEGIN,
                             rt.EV_SOLVE_END, rt.EV_EXIT, rt.EV_PIVOT)
    layout = _read(CSRC, "cut_narr_layout.hpp")
    for name, val in (("kCutEvCall", 0), ("kCutEvLevel", 1), ("kCutEvCut", 2),
                      ("kCutEvSolveBegin", 3), ("kCutEvSolveEnd", 4), ("kCutEvExit", 5),
                      ("kCutEvPivot", 8)):
        assert re.search(r"\b%s = %d," % (name, val), layout), name
    T = cbc.textbook_items(oracle)[5][1]
    n, _, _ = rt.narrate_cutting_plane(T, TEXTBOOK_MAX_CUTS)
    rows0, cols = T.shape
    model = [np.asarray(n.record0).size] + [np.asarray(b).size for b in n.blocks]
    offs = cb.block_offsets(n.events, rows0, cols)
    assert [d for _, d in offs] == model
    assert [o for o, _ in offs] == [int(x) for x in np.cumsum([0] + model[:-1])]
    need = sum(model)
    for cap in (0, model[0] - 1, model[0], model[0] + model[1], need - 1, need, need + 7):
        c = dict(cap=cap, cur=0, made_d=0, made_b=0, kept_b=0)
        at = [cb.narr_push(c, d) for d in model]
        kept = 0
        while kept < len(model) and sum(model[:kept + 1]) <= cap:
            kept += 1
        assert c["made_d"] == need and c["made_b"] == len(model)
        assert c["kept_b"] == kept and c["cur"] == sum(model[:kept])
        assert at == [o for o, _ in offs[:kept]] + [-1] * (len(model) - kept)


def test_layout_walk_under_sanitizers(tmp_path):
    """tools/cut_narr_check.cpp, a stand-alone host program built with the address and
    undefined-behaviour sanitizers: the push rule and the lane walk replayed over exactly sized
    buffers."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "cut_narr_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "cut_narr_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert "cut_narr_check: ok" in p.stdout, tail
    assert "runtime error" not in tail, tail


# ---- kernel build ----------------------------------------------------------------------------------
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


def test_narrated_kernels_build_without_scratch(tmp_path):
    """cut_batch_narr_kernels.hip alone, for gfx950, with the Makefile's flags: every kernel has a
    private segment of 0 bytes, the two state-machine kernels no more static LDS than their
    un-narrated twins in the same build; cut_batch_kernels.hip still yields exactly the kernels it
    had."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    narr = _kernels(hipcc, "cut_batch_narr_kernels.hip", tmp_path / "cut_batch_narr_kernels.s")
    plain = _kernels(hipcc, "cut_batch_kernels.hip", tmp_path / "cut_batch_kernels.s")
    search = {k: v for k, v in narr.items() if "k_cut_batch_narrIL" in k}
    base = {k: v for k, v in plain.items() if "k_cut_batchIL" in k}
    assert len(search) == 2 and len(base) == 2, (sorted(narr), sorted(plain))
    assert len(plain) == 3 and any("k_cut_batch_load" in k for k in plain)
    assert not any("narr" in k for k in plain)
    assert len(narr) == 4 and any("k_cut_batch_narr_first" in k for k in narr)
    assert any("k_cut_batch_narr_call" in k for k in narr)
    form = lambda k: re.search(r"ILb(\d)E", k).group(1)
    for name, (priv, lds) in search.items():
        twin = [v for k, v in base.items() if form(k) == form(name)]
        assert len(twin) == 1, name
        assert lds <= twin[0][1], (name, lds, twin[0][1])
    for name, (priv, _) in list(narr.items()) + list(plain.items()):
        assert priv == 0, (name, priv)
