"""CPU tests of the scenario batch's sensitivity report (lpr_sens_batch_ranging, DESIGN.md section
19): the library exports the two calls, header, bindings and the C# declarations name them, a null
handle is refused with nothing written, the lane constants the GPU tests restate are those of the
header, and the trim of one scenario's row out of the padded arrays (sens_batch.trim_ranging) is
checked on hand-made arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_py_ranging as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
NAMES = ("lpr_sens_batch_ranging", "lpr_sens_batch_ranging_time")


def test_library_header_and_bindings_declare_the_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert getattr(N.lib, name) is not None, name            # exported by the library
        assert len(re.findall(r"static extern \w+ " + name + r"\(", cs)) == 1, name
    assert len(N.SIGNATURES["lpr_sens_batch_ranging"][1]) == 10  # the handle and nine outputs
    # the header cites the C# lines of lpr_sens_ranging
    raw = open(HEADER).read()
    at = raw.index("int lpr_sens_batch_ranging(")
    comment = raw[raw.rindex("/*", 0, at):at]
    for lines in (":276-297", ":324-359", ":396-424", ":212-222", ":69-84"):
        assert lines in comment, lines


def test_null_handle_is_refused_and_nothing_is_written():
    from lpr_381_group_v22_amd import _native as N
    ints = [np.full(4, 77, dtype=np.int32) for _ in range(2)]
    dbls = [np.full(4, 7.5, dtype=np.float64) for _ in range(7)]
    args = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in ints] + \
           [a.ctypes.data_as(C.POINTER(C.c_double)) for a in dbls]
    assert N.lib.lpr_sens_batch_ranging(None, *args) == N.LPR_BAD_ARGUMENT
    assert "null or orphaned" in N.lib.lpr_last_error().decode()
    assert all((a == 77).all() for a in ints) and all((a == 7.5).all() for a in dbls)
    assert N.lib.lpr_sens_batch_ranging(None, *([None] * 9)) == N.LPR_BAD_ARGUMENT
    ms = C.c_double(-1.0)
    assert N.lib.lpr_sens_batch_ranging_time(None, C.byref(ms)) == N.LPR_BAD_ARGUMENT
    assert ms.value == -1.0


def test_lane_constants_match_the_kernel():
    """test_sens_batch_ranging_gpu.py restates the lane mapping; here against the header."""
    import test_sens_batch_ranging_gpu as g
    text = open(os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc",
                             "sens_batch_ranging_common.hpp")).read()
    val = lambda k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1))
    assert val("kSbrLanes") == g.LANES and val("kSbrWaveLanes") == g.WAVE_LANES
    assert re.search(r"constexpr int kSbrWaves = kSbrLanes / kSbrWaveLanes;", text)
    assert g.WAVES == g.LANES // g.WAVE_LANES
    text = open(os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc",
                             "sens_batch_ranging_kernels.hip")).read()
    assert val("kSbrLoad") == g.LOAD


def _padded(count, mc, mr, shapes):
    """Hand-made padded arrays: scenario k's own cells hold 1000 k + position, the rest the fill."""
    from lpr_381_group_v22_amd.engine import RangingReport
    from lpr_381_group_v22_amd.sens_batch import NO_BASIC_ENTRY
    out = {}
    for f in ref.FIELDS:
        is_col = f in ("kind", "var_row", "reduced_cost", "cost_lo", "cost_hi")
        width = mc if is_col else mr
        if f in ref.INT_FIELDS:
            a = np.full((count, width), NO_BASIC_ENTRY, dtype=np.int32)
        else:
            a = np.full((count, width), np.nan)
        for k, (r, c) in enumerate(shapes):
            own = (c - 1) if is_col else (r - 1)
            a[k, :own] = 1000 * k + np.arange(own)
        out[f] = a
    return RangingReport(**out)


def test_trim_of_one_scenario():
    from lpr_381_group_v22_amd.sens_batch import NO_BASIC_ENTRY, trim_ranging
    shapes = [(3, 5), (5, 8), (4, 6), (5, 8)]
    pad = _padded(4, 7, 4, shapes)
    assert NO_BASIC_ENTRY == -2 ** 31
    for k, (r, c) in enumerate(shapes):
        rep = trim_ranging(pad, k, r, c)
        for f in ref.FIELDS:
            a = getattr(rep, f)
            own = (c - 1) if f in ("kind", "var_row", "reduced_cost", "cost_lo", "cost_hi") \
                else (r - 1)
            assert a.shape == (own,), (k, f)
            assert a.dtype == (np.int32 if f in ref.INT_FIELDS else np.float64), (k, f)
            assert a.tolist() == (1000 * k + np.arange(own)).tolist(), (k, f)
            a[:] = 0                                  # a copy: the padded arrays stay
            assert getattr(pad, f)[k, :own].tolist() == (1000 * k + np.arange(own)).tolist()
    # a NaN of the scenario's own (a NaN reduced cost, say) is data, not padding
    pad.reduced_cost[0, 1] = np.nan
    assert np.isnan(trim_ranging(pad, 0, 3, 5).reduced_cost[1])
    # cutting data off, or a shape past the padded row, is refused
    with pytest.raises(ValueError):
        trim_ranging(pad, 1, 4, 8)                    # one constraint of scenario 1 would be lost
    with pytest.raises(ValueError):
        trim_ranging(pad, 1, 5, 7)                    # one column would be lost
    with pytest.raises(ValueError):
        trim_ranging(pad, 1, 6, 8)                    # rows - 1 = 5 > 4
    with pytest.raises(ValueError):
        trim_ranging(pad, 0, 3, 9)                    # cols - 1 = 8 > 7
