"""CPU tests of the narrated Branch & Bound batch: the ABI declares the
lpr_bb_batch_narrate_* calls and the bindings have and use them, the narrated kernels build for
gfx950 without scratch and within their un-narrated twins' LDS while bb_batch_kernels.hip keeps
exactly the kernels it had, a host-only sanitizer program replays the cursor rules over an exactly
sized buffer, the inputs of the GPU tests do what those tests rely on, and the shared formatter
gives the restatement's text from the restatement's numbers."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bb_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

CALLS = ["lpr_bb_batch_narrate_reserve", "lpr_bb_batch_narrate_info",
         "lpr_bb_batch_narrate_pops_read", "lpr_bb_batch_narrate_children_read",
         "lpr_bb_batch_narrate_tableaux_read", "lpr_bb_batch_narrate_read_all",
         "lpr_bb_batch_narrate_best_read"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_and_bindings_declare_and_use_the_calls():
    from lpr_381_group_v22_amd import _native as N
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", _read(HEADER), flags=re.S)
    cs = _read(ROOT, "integration", "csharp", "NativeMethods.cs")
    gs = _read(ROOT, "integration", "csharp", "GpuSolvers.cs")
    py = _read(ROOT, "lpr_381_group_v22_amd", "bb_batch.py")
    eng = _read(CSRC, "bb_batch_engine.hip")
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"\b" + name + r"\s*\(", cs)) == 1, name
        assert "NativeMethods." + name + "(" in gs, name
        assert "N.lib." + name + "(" in py, name
        assert re.search(r"^int " + name + r"\(", eng, flags=re.M), name
    assert "public string Narration(int k)" in gs
    # opts, result and the ABI version stay: narration is a property of the handle
    assert ctypes.sizeof(N.BBBatchOpts) == 16 and ctypes.sizeof(N.BBBatchResult) == 32
    # one text of the search, two instantiations
    assert "bb_batch_body<NT, kLds, false>" in _read(CSRC, "bb_batch_kernels.hip")
    assert "bb_batch_body<NT, kLds, true>" in _read(CSRC, "bb_batch_narr_kernels.hip")
    for fn in ("ip_pivot", "child_lp", "add_constraint"):
        assert len(re.findall(r"__device__ [\w ]*\b%s\(" % fn,
                              _read(CSRC, "bb_batch_body.hpp"))) == 1, fn
        assert fn + "(" not in _read(CSRC, "bb_batch_kernels.hip"), fn
    # the layout headers need no HIP, and the cursor rules are stated in kept_prefix.hpp alone
    layout, rule = _read(CSRC, "bb_narr_layout.hpp"), _read(CSRC, "kept_prefix.hpp")
    assert "hip/" not in layout and "hip/" not in rule
    assert "kept_push(" in rule and "kept_drop(" in rule
    assert "_push(" not in layout and "_drop(" not in layout


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
    """bb_batch_narr_kernels.hip alone, for gfx950, with the Makefile's flags: the three search
    kernels have a private segment of 0 bytes and no more static LDS than their un-narrated twins
    in the same build; bb_batch_kernels.hip still yields exactly the kernels it had."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    narr = _kernels(hipcc, "bb_batch_narr_kernels.hip", tmp_path / "bb_batch_narr_kernels.s")
    plain = _kernels(hipcc, "bb_batch_kernels.hip", tmp_path / "bb_batch_kernels.s")
    search = {k: v for k, v in narr.items() if "k_bb_batch_narrIL" in k}
    base = {k: v for k, v in plain.items() if "k_bb_batchIL" in k}
    assert len(search) == 3 and len(base) == 3, (sorted(narr), sorted(plain))
    assert len(plain) == 5 and any("k_bb_batch_load" in k for k in plain)
    assert any("k_bb_batch_reset" in k for k in plain)
    assert not any("narr" in k for k in plain)
    assert len(narr) == 4 and any("k_bb_batch_narr_reset" in k for k in narr)
    form = lambda k: re.search(r"ILi(\d+)ELb(\d)E", k).groups()
    for name, (priv, lds) in search.items():
        twin = [v for k, v in base.items() if form(k) == form(name)]
        assert len(twin) == 1, name
        assert priv == 0, (name, priv)
        assert lds <= twin[0][1], (name, lds, twin[0][1])
    for name, (priv, _) in narr.items():
        assert priv == 0, (name, priv)


def test_layout_walk_under_sanitizers(tmp_path):
    """tools/bb_narr_check.cpp, a stand-alone host program built with the address and
    undefined-behaviour sanitizers: the cursor rules of bb_narr_layout.hpp replayed over an
    exactly sized buffer."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "bb_narr_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "bb_narr_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert "bb_narr_check: ok" in p.stdout, tail
    assert "runtime error" not in tail, tail


_SOLVED = {}


def solved(oracle, name, pruning=False, cap=20):
    key = (name, pruning, cap)
    if key not in _SOLVED:
        obj, cons = dict(bb_cases.all_bb_cases())[name]
        st, T, n = bb_cases.primal_final_tableau(oracle, obj, cons)
        nv = n if st == 0 else max(1, T.shape[1] - 1)
        _SOLVED[key] = (T, nv, oracle.bb_solve(T, nv, enable_pruning=pruning, node_cap=cap))
    return _SOLVED[key]


def test_inputs_do_what_the_gpu_tests_rely_on(oracle):
    for name in ("binary_8v3c_s3", "huge_relaxation_value"):
        tr = solved(oracle, name)[2]["trace"]
        assert any(t[1] == 1 for t in tr) and any(t[1] == 2 for t in tr), name
    for name in ("knapsack_sample", "binary_6v2c_s2", "frac_4v2c_s10"):
        assert any(r["status"] == 1 for r in solved(oracle, name)[2]["records"]), name
    r = solved(oracle, "binary_4v1c_s0")[2]
    assert len(r["records"]) == 1 and r["found"] and r["processed"] == 1
    r = solved(oracle, "binary_5v2c_s1")[2]
    assert max(x["depth"] for x in r["records"]) == 20 and r["processed"] == 20
    assert solved(oracle, "knapsack_sample")[2]["processed"] == 20
    assert solved(oracle, "knapsack_sample", pruning=True)[2]["processed"] == 5
    # no case has a failed child: that line is covered with synthetic numbers below
    for name, _ in bb_cases.all_bb_cases():
        assert not any(x["status"] == 2 for x in solved(oracle, name)[2]["records"]), name


def restatement_numbers(T, nv, cap=20, pruning=False):
    """The restatement's search (tests/ref_py_bb.py) walked for its numbers: what
    format_branch_and_bound takes.  Nothing of the product computes them."""
    from lpr_381_group_v22_amd.branch_and_bound import (BB_FAILED, BB_INFEASIBLE, BB_SOLVED,
                                                         ChildNumbers, PopNumbers)
    from ref_py_bb import INF, BranchAndBound, ceil_total, floor_total, round4, to_int32
    b = BranchAndBound(nv, cap)
    pops, best, have, best_tab, capped = [], -INF, False, None, False
    stack = [b.RoundTableau([[float(v) for v in row] for row in T])]
    it = 0
    while stack:
        it += 1
        if it > cap:
            capped = True
            break
        tab = b.RoundTableau(stack.pop())
        z = round4(tab[0][-1])
        if pruning and have and z <= best:
            pops.append(PopNumbers(z, None, None))
            continue
        vals = b._decision(tab)
        if all(b.IsInteger(v) for v in vals) and z > best:
            best, have, best_tab = z, True, np.array(tab)
        cand = [(abs((v - floor_total(v)) - 0.5), i) for i, v in enumerate(vals)
                if not b.IsInteger(v)]
        if not cand:
            pops.append(PopNumbers(z, vals, None))
            continue
        var = min(cand, key=lambda t: t[0])[1]
        kids, children = [], []
        for bound, typ in ((to_int32(floor_total(vals[var])), 0),
                           (to_int32(ceil_total(vals[var])), 1)):
            con = [1.0 if i == var else 0.0 for i in range(nv)] + [float(bound), float(typ)]
            try:
                tabs, opt = b.solver.DoDualSimplex(b.AddConstraint(con, tab))
            except IndexError:
                children.append(ChildNumbers(BB_FAILED, list(b.solver.trace), []))
                continue
            arr = [np.array(t) for t in tabs]
            children.append(ChildNumbers(BB_INFEASIBLE if opt is None else BB_SOLVED,
                                         list(b.solver.trace), arr))
            if opt is not None:
                kids.append(b.RoundTableau(tabs[-1]))
        pops.append(PopNumbers(z, vals, children))
        stack.extend(reversed(kids))
    return pops, best_tab, capped


@pytest.mark.parametrize("name,pruning", [("knapsack_sample", False), ("knapsack_sample", True),
                                          ("binary_8v3c_s3", False), ("binary_4v1c_s0", False),
                                          ("binary_5v2c_s1", False), ("frac_4v2c_s10", True)])
def test_formatter_on_restatement_numbers_is_execute_narrated(oracle, name, pruning):
    from lpr_381_group_v22_amd.branch_and_bound import format_branch_and_bound
    from ref_py_bb_text import NarratedBranchAndBound
    from ref_py_text import CRLF
    T, nv, _ = solved(oracle, name)
    res = NarratedBranchAndBound(nv).ExecuteNarrated([[float(v) for v in r] for r in T], pruning)
    pops, tab, capped = restatement_numbers(T, nv, pruning=pruning)
    text, x, z, processed = format_branch_and_bound(nv, pops, tab, capped, pruning)
    assert text.replace(CRLF, "\n") == res["text"].replace(CRLF, "\n")
    assert x == res["x"] and z == res["z"] and processed == res["processed"]
    assert capped == ("Potential infinite loop detected" in text)


def test_failed_line_from_synthetic_numbers():
    """`failed: {e}` (:1147 / :1207): no case reaches it, so the formatter gets a made-up pop whose
    lower child failed and whose upper child was solved."""
    from lpr_381_group_v22_amd.branch_and_bound import (BB_FAILED, BB_SOLVED, ChildNumbers,
                                                         PopNumbers, format_branch_and_bound)
    t = np.array([[0.0, 0.0, 1.0, 3.0], [1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 2.0]])
    pops = [PopNumbers(3.5, [0.5, 1.0], [ChildNumbers(BB_FAILED, [], []),
                                         ChildNumbers(BB_SOLVED, [(0, 2, 1)], [t, t])]),
            PopNumbers(3.0, [1.0, 2.0], None)]
    text, x, z, processed = format_branch_and_bound(2, pops, t, False)
    assert ("Lower branch (branch 1) failed: System.ArgumentOutOfRangeException: Index was out "
            "of range.") in text
    assert "branch 2 Upper branch Tableau 1" in text and "branch 2 Upper branch final tableau" in text
    assert "pivot @ constraint 2, column 2\n" in text
    assert "--- Processing branch 2 (Depth 1) ---\nParent branch: 0\n" in text
    assert (x, z, processed) == ([1.0, 2.0], 3.0, 2) and "Optimal branch: 2\n" in text


_PROBE = """
import sys
sys.path.insert(0, %r)
from oracle_lib import Oracle
import special_values as sv
o = Oracle()
for name, T, n in sv.bb_start_tableaux(o):
    r = o.bb_solve(T, n, node_cap=sv.BB_NODE_CAP)
    if any(rec["status"] == 2 for rec in r["records"]):
        print(name)
print("done")
"""


def test_no_special_value_start_tableau_has_a_failed_child():
    """The B&B start tableaux of tests/special_values.py (minus BB_NON_TERMINATING) on the oracle,
    in a child process with a timeout (some oracle searches have no iteration cap): none gives a
    status-2 record, so the GPU tests have no natural failed child either."""
    p = subprocess.run([sys.executable, "-c", _PROBE % os.path.dirname(os.path.abspath(__file__))],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split() == ["done"], p.stdout
