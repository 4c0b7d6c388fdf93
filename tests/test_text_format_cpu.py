"""CPU tests of the device text formatter: the number core of
csrc/text_common.hpp against a restatement of the {v:F3} rule in a stand-alone host program under
the address and undefined-behaviour sanitizers, the header's constants against what
``format_fixed`` and ``fractions`` give, the two host statements of the rule against each other on
the values the GPU tests use, and the host assembly of the device paths (bodies supplied by the
host ``Format``) against ``format_snapshots`` / ``format_console``."""
import math
import os
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import batch_trace_cases as btc
import text_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")


@pytest.fixture(scope="module")
def check_tool(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("text") / "text_format_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "text_format_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    return str(exe)


def test_number_core_under_sanitizers(check_tool):
    p = subprocess.run([check_tool], capture_output=True, text=True, timeout=600)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert "text_format_check: ok" in p.stdout, tail
    assert "runtime error" not in tail, tail


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _ceil_double_bits(x):
    """Bits of the smallest double >= the positive rational x; +Inf's past DBL_MAX."""
    if x > Fraction(2) ** 1024 - Fraction(2) ** 970:
        return 0x7FF0000000000000
    f = float(x)
    if Fraction(f) < x:
        f = math.nextafter(f, math.inf)
    assert Fraction(f) >= x > Fraction(math.nextafter(f, 0.0))
    return _bits(f)


def test_constants_of_the_header(check_tool):
    from lpr_381_group_v22_amd.table_iteration_formater import format_fixed
    p = subprocess.run([check_tool, "--constants"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    got = {"pow10": {}, "carry": {}}
    for line in p.stdout.split("\n"):
        w = line.split()
        if len(w) == 2:
            got[w[0]] = int(w[1], 16)
        elif len(w) == 3:
            got[w[0]][int(w[1])] = int(w[2], 16)
    # the threshold: bisection on the bit pattern between 0.0004 ("0.000") and 0.0006 ("0.001")
    lo, hi = _bits(0.0004), _bits(0.0006)
    as_double = lambda b: struct.unpack("<d", struct.pack("<Q", b))[0]
    assert format_fixed(as_double(lo), 3) == "0.000" and format_fixed(as_double(hi), 3) == "0.001"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if format_fixed(as_double(mid), 3) == "0.000":
            lo = mid
        else:
            hi = mid
    assert got["threshold"] == hi == 0x3F40624DD2F1A9F8
    assert got["big"] == _bits(1e15) and Fraction(1e15) == Fraction(10) ** 15
    assert sorted(got["pow10"]) == list(range(-4, 309))
    for k, b in got["pow10"].items():
        assert b == _ceil_double_bits(Fraction(10) ** k), k
    assert sorted(got["carry"]) == list(range(15, 309))
    for k, b in got["carry"].items():
        assert b == _ceil_double_bits((Fraction(10) ** 16 - 5) * Fraction(10) ** (k - 15)), k


def test_the_two_host_rules_agree_on_the_gpu_values():
    from lpr_381_group_v22_amd.table_iteration_formater import format_fixed
    from ref_py_text import py_fixed
    vals = text_cases.cell_values()
    assert len(vals) > 300
    for v in vals:
        assert format_fixed(v, 3) == py_fixed(v, 3), v.hex()
    # what the GPU tests rely on: the list reaches every class and the length-changing carries
    texts = {format_fixed(v, 3) for v in vals}
    for t in ("NaN", "Infinity", "-Infinity", "0.000", "0.001", "1000.000", "-1000.000",
              "1000000000000000.000", "100000000000000.000", "100000000000002.000",
              "1" + "0" * 300 + ".000"):
        assert t in texts, t
    assert "-0.000" not in texts
    assert max(len(t) for t in texts) == 314


def test_host_assembly_from_bodies(oracle):
    """snapshots_from_bodies / console_from_bodies with bodies cut from the host Format are
    format_snapshots / format_console, on every case of batch_trace_cases."""
    from lpr_381_group_v22_amd.primal_batch import console_from_bodies, snapshots_from_bodies
    from lpr_381_group_v22_amd.primal_simplex_solver import format_console, format_snapshots
    from lpr_381_group_v22_amd.table_iteration_formater import Format, title_line
    body = lambda T, n: Format(T, n, "q")[len(title_line("q")):]
    seen = set()
    for name, case in btc.all_cases():
        n = len(case[0])
        pivots = btc.SHAPE_PIVOTS if name.startswith("form_") else btc.CAP
        ref = btc.step_records(oracle, btc.built(oracle, case), pivots)
        recs, st = ref["records"], ref["status"]
        seen.add(st)
        x = [float(i) + 0.5 for i in range(n)] if st == btc.OPTIMAL else None
        z = 12.5 if st == btc.OPTIMAL else 0.0
        bodies = [body(T, n) for _, _, T in recs]
        final = body(ref["T"], n) if st in (btc.OPTIMAL, btc.UNBOUNDED) else None
        assert snapshots_from_bodies(bodies, n, st, final, z, x) == \
            format_snapshots([T for _, _, T in recs], n, st, ref["T"], z, x), name
        if ref["pivots"] < btc.TRACE_CAP:
            assert console_from_bodies([(r, e) for r, e, _ in recs[1:]], bodies, n, st, z, x) == \
                format_console(recs, n, st, z, x), name
    assert seen >= {btc.OPTIMAL, btc.UNBOUNDED, btc.LIMIT}


def test_block_cases_cover_the_seams():
    """The shapes the GPU seam test formats: every lane count of a row, label widths, nvars on
    both sides of cols - 1."""
    blocks = text_cases.seam_blocks()
    cols = {T.shape[1] for T, _ in blocks}
    rows = {T.shape[0] for T, _ in blocks}
    assert cols >= {1, 2, 63, 64, 65, 255, 256, 257, 1025}
    assert rows >= {1, 2, 10, 11, 100, 101}
    assert {nv for _, nv in blocks} >= {0, 1, 9, 10, 99, 100}
    assert any(nv == T.shape[1] - 1 for T, nv in blocks)
    assert any(nv == T.shape[1] for T, nv in blocks)
    assert any(nv == T.shape[1] + 3 for T, nv in blocks)
    assert any(np.any(np.abs(T) == np.finfo(np.float64).max) for T, _ in blocks)
