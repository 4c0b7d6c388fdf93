"""CPU tests of the narrated B&B batch's device text: the shared formatter
gives the same text from pre-formatted bodies as from arrays, the block index function places a
record's tableaux among its IP's blocks, the ABI declares and exports the two calls, the rounded
text kernels build for gfx950 without scratch beside unrounded ones that carry no floating-point
code, and a host-only sanitizer program replays the block layout rule."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_bb_batch_narr_cpu import restatement_numbers, solved

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")
CALLS = ["lpr_text_format_tableaux_rounded", "lpr_bb_batch_narrate_text"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


# --------------------------------------------------------------------- 1. formatter with bodies
def host_body(tab, nv, times):
    """Format(round4^times(tab), nv, "") minus its title line: what the device writes."""
    from lpr_381_group_v22_amd import table_iteration_formater as fmt
    from lpr_381_group_v22_amd.branch_and_bound import _round4_np
    t = np.asarray(tab, dtype=np.float64)
    for _ in range(times):
        t = _round4_np(t)
    text = fmt.Format(t, nv, "")
    assert text.startswith(fmt.title_line(""))
    return text[len(fmt.title_line("")):]


def with_bodies(pops, incumbent, nv):
    """The same pops with every tableau replaced by its body, rounded as the text rounds it."""
    from lpr_381_group_v22_amd.branch_and_bound import BB_SOLVED, ChildNumbers, PopNumbers
    out = []
    for p in pops:
        kids = None
        if p.children is not None:
            kids = [ChildNumbers(c.status, c.pivots,
                                 [host_body(t, nv, 2 if c.status == BB_SOLVED else 1)
                                  for t in c.tableaux]) for c in p.children]
        out.append(PopNumbers(p.z, p.vals, kids))
    return out, None if incumbent is None else host_body(incumbent, nv, 1)


@pytest.mark.parametrize("name,pruning", [("knapsack_sample", False), ("knapsack_sample", True),
                                          ("binary_8v3c_s3", False), ("binary_4v1c_s0", False),
                                          ("binary_5v2c_s1", False), ("frac_4v2c_s10", True),
                                          ("huge_relaxation_value", False)])
def test_bodies_give_the_text_arrays_give(oracle, name, pruning):
    from lpr_381_group_v22_amd.branch_and_bound import format_branch_and_bound
    from ref_py_bb_text import NarratedBranchAndBound
    from ref_py_text import CRLF
    T, nv, _ = solved(oracle, name)
    res = NarratedBranchAndBound(nv).ExecuteNarrated([[float(v) for v in r] for r in T], pruning)
    pops, tab, capped = restatement_numbers(T, nv, pruning=pruning)
    a = format_branch_and_bound(nv, pops, tab, capped, pruning)
    bp, bt = with_bodies(pops, tab, nv)
    b = format_branch_and_bound(nv, bp, bt, capped, pruning)
    assert a == b
    assert a[0].replace(CRLF, "\n") == res["text"].replace(CRLF, "\n")
    for nl in ("\n", CRLF):
        assert format_branch_and_bound(nv, bp, bt, capped, pruning, nl) == \
            format_branch_and_bound(nv, pops, tab, capped, pruning, nl)


def test_bodies_of_synthetic_infeasible_and_failed_children():
    """An infeasible child with three tableaux (only the first is shown, rounded once), a failed
    child (none is shown) and solved children, with cells whose text depends on the rounding."""
    from lpr_381_group_v22_amd.branch_and_bound import (BB_FAILED, BB_INFEASIBLE, BB_SOLVED,
                                                         ChildNumbers, PopNumbers,
                                                         format_branch_and_bound)
    t = np.array([[0.00049999, 0.0, 1.23449999, 3.0], [1.0, -0.00004, 0.0, 1.0],
                  [0.0, 1.0, 0.0, 2.00005]])
    u, v = t * 3.0, t - 0.25
    pops = [PopNumbers(3.5, [0.5, 1.0], [ChildNumbers(BB_INFEASIBLE, [(0, 2, 1), (0, 1, 2)],
                                                      [t, u, v]),
                                         ChildNumbers(BB_SOLVED, [(0, 2, 1)], [u, t])]),
            PopNumbers(3.25, [0.5, 2.0], [ChildNumbers(BB_FAILED, [], []),
                                          ChildNumbers(BB_SOLVED, [(1, 1, 0)], [v])]),
            PopNumbers(3.0, [1.0, 2.0], None)]
    a = format_branch_and_bound(2, pops, t, False)
    bp, bt = with_bodies(pops, t, 2)
    assert isinstance(bp[0].children[0].tableaux[2], str) and isinstance(bt, str)
    b = format_branch_and_bound(2, bp, bt, False)
    assert a == b
    text = a[0]
    assert "branch 1: Infeasible tableau" in text and text.count("Infeasible tableau") == 1
    assert "failed: System.ArgumentOutOfRangeException" in text
    assert "Optimal solution tableau at branch 2.2" in text
    # the rounding shows: 0.00049999 prints 0.001 after it, 0.000 before
    assert "Z\t0.001\t0.000\t1.235\t3.000\t" in text and "\t0.000\t0.000\t1.234\t" not in text
    # an infeasible child without a tableau is "(empty)" either way
    none = [PopNumbers(3.5, [0.5, 1.0], [ChildNumbers(BB_INFEASIBLE, [], []),
                                         ChildNumbers(BB_INFEASIBLE, [], [])])]
    assert "branch 1: Infeasible tableau (empty)" in format_branch_and_bound(2, none, None, False)[0]


# ------------------------------------------------------------------------ 2. block index function
def test_block_index_on_constructed_records():
    from lpr_381_group_v22_amd.bb_batch import kept_tableaux, narration_block_index
    R, C = 3, 5
    recs = [dict(depth=0), dict(depth=1), dict(depth=1), dict(depth=2), dict(depth=2)]
    e1, e2 = (R + 1) * (C + 1), (R + 2) * (C + 2)
    # record 2 made three and stepped back to two (the drop of :392-400): ntab counts what remains
    ntab = [0, 2, 2, 3, 1]
    off = [0, 0, 2 * e1, 4 * e1, 4 * e1 + 3 * e2]
    need = 4 * e1 + 4 * e2
    assert narration_block_index((R, C), recs, off, ntab, need) == [0, 0, 2, 4, 7, 8]
    assert narration_block_index((R, C), recs, off, ntab, need + 5) == [0, 0, 2, 4, 7, 8]
    # one double short of the need: everything but the last tableau
    assert narration_block_index((R, C), recs, off, ntab, need - 1) == [0, 0, 2, 4, 7, 7]
    # a cap cut inside record 3: one of its three tableaux, and nothing of record 4, whose
    # tab_off is where the cursor stood -- the kept size
    kept = 4 * e1 + e2
    off_cut = [0, 0, 2 * e1, 4 * e1, kept]
    assert narration_block_index((R, C), recs, off_cut, ntab, kept) == [0, 0, 2, 4, 5, 5]
    # one double short of a tableau, and nothing at all
    assert narration_block_index((R, C), recs, [0, 0, 0, 0, 0], ntab, e1 - 1) == [0] * 6
    assert narration_block_index((R, C), recs, [0, 0, 0, 0, 0], ntab, 0) == [0] * 6
    assert narration_block_index((R, C), recs[:1], [0], [0], 0) == [0, 0]  # the root alone
    # the rule itself, as _child_tableaux applies it
    assert kept_tableaux(4, 6, 0, 2, 47) == 1 and kept_tableaux(4, 6, 0, 2, 48) == 2
    assert kept_tableaux(4, 6, 48, 2, 47) == 0 and kept_tableaux(4, 6, 100, 2, 0) == 0
    assert kept_tableaux(4, 6, 0, 2, 10 ** 9) == 2


# -------------------------------------------------------------------------- 3. header and library
def test_header_bindings_and_library_have_the_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", _read(HEADER), flags=re.S)
    cs = _read(ROOT, "integration", "csharp", "NativeMethods.cs")
    gs = _read(ROOT, "integration", "csharp", "GpuSolvers.cs")
    assert re.search(r"#define LPR_ABI_VERSION 1\b", text)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"\b" + name + r"\s*\(", cs)) == 1, name
        assert "NativeMethods." + name + "(" in gs, name
        assert getattr(lib, name) is not None, name
    assert re.search(r"lpr_text_format_tableaux_rounded\(lpr_engine\* e, int32_t count,\s*"
                     r"const int32_t\* rows,\s*const int32_t\* cols, const int32_t\* nvars,\s*"
                     r"const int32_t\* round4, const double\* tableaux,\s*lpr_text\*\* out\);", text)
    assert re.search(r"lpr_bb_batch_narrate_text\(lpr_bb_batch\* b, int64_t\* first_block, "
                     r"lpr_text\*\* out\);", text)
    assert "public string NarrationText(int k, DeviceText text, long[] firstBlock)" in gs
    assert "N.lib.lpr_bb_batch_narrate_text(" in _read(ROOT, "lpr_381_group_v22_amd",
                                                       "bb_batch.py")
    # the layout rule is stated in a header that needs no HIP, and the engine uses that text
    layout = _read(CSRC, "bb_narr_text_layout.hpp")
    assert "hip/" not in layout and "narr_text_runs(" in layout
    assert "narr_text_runs(" in _read(CSRC, "bb_batch_engine.hip")


# ------------------------------------------------------------------------------ 4. compiler report
def test_rounded_text_kernels_build_without_scratch(tmp_path):
    """text_kernels.hip alone, for gfx950, with the Makefile's flags: the rounded measure and
    write kernels have a private segment of 0 bytes; the unrounded ones are still emitted, also
    without scratch, and hold no double-precision instruction (the rounding's code is not in
    them: the number core of text_common.hpp has no floating-point operation)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "text_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-fno-fast-math", "-DLPR_BUILD", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "text_kernels.hip"), "-o", str(out)], check=True,
                   capture_output=True)
    asm = out.read_text()
    meta = dict(re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S))
    code = dict(re.findall(r"^(_ZN\S+):[^\n]*\n(.*?)\n\s*s_endpgm", asm, flags=re.S | re.M))
    for stem in ("k_text_measure", "k_text_write"):
        for flag, rounded in (("ILb1E", True), ("ILb0E", False)):
            names = [k for k in meta if stem + flag in k]
            assert len(names) == 1, (stem, flag, sorted(meta))
            priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)",
                                 meta[names[0]]).group(1))
            assert priv == 0, (names[0], priv)
            f64 = re.findall(r"\bv_\w+_f64\b", code[names[0]])
            assert bool(f64) == rounded, (names[0], f64[:4])
    assert len([k for k in meta if "k_text_" in k]) == 9, sorted(meta)


# -------------------------------------------------------------------------------- 5. sanitizer tool
def test_block_layout_walk_under_sanitizers(tmp_path):
    """tools/bb_narr_text_check.cpp, a stand-alone host program built with the address and
    undefined-behaviour sanitizers: the rule of bb_narr_text_layout.hpp replayed on constructed
    record lists at every cap, each block read from an exactly sized kept prefix."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "bb_narr_text_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "bb_narr_text_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert "bb_narr_text_check: ok" in p.stdout, tail
    assert "runtime error" not in tail, tail
