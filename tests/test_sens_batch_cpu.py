"""CPU tests of the sensitivity scenario batch: the ABI, the ctypes binding
and the C# binding declare the lpr_sens_batch_* calls and lpr_sens_edit, pack_scripts packs and
refuses as lpr_sens_batch_create does, and the Python form rule is the header's.

The last test does not test the batch: it runs the oracle alone on the constructions of
tests/sens_batch_cases.py, so that the GPU tests' cases cannot decay into easy ones."""
import ctypes
import os
import re

import numpy as np
import pytest

import sens_batch_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

SENS_BATCH_CALLS = ["lpr_sens_batch_create", "lpr_sens_batch_destroy", "lpr_sens_batch_run",
                    "lpr_sens_batch_info", "lpr_sens_batch_outcomes_read",
                    "lpr_sens_batch_state_read", "lpr_sens_batch_solution_read",
                    "lpr_sens_batch_tableau_read", "lpr_sens_batch_log_read"]


def test_header_and_bindings_declare_the_sens_batch_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    for name in SENS_BATCH_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"static extern \w+ " + name + r"\(", cs)) == 1, name
    assert "typedef struct lpr_sens_batch lpr_sens_batch;" in text
    assert re.search(r"typedef struct lpr_sens_edit\s*{[^}]*int32_t op, a, b, reserved;[^}]*"
                     r"double v;[^}]*}\s*lpr_sens_edit;", text)
    for op, code in [("RESOLVE_ALL", 0), ("NONBASIC_CBAR", 1), ("BASIC", 2), ("RHS", 3),
                     ("NONBASIC_COLUMN", 4)]:
        assert re.search(r"LPR_SENS_EDIT_%s = %d\b" % (op, code), text), op
        assert getattr(N, "LPR_SENS_EDIT_" + op) == code


def test_ctypes_structs_match_the_header():
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.sens_batch import EDIT_DTYPE
    assert [f for f, _ in N.SensEdit._fields_] == ["op", "a", "b", "reserved", "v"]
    assert ctypes.sizeof(N.SensEdit) == 24 and EDIT_DTYPE.itemsize == 24
    assert N.SensEdit.v.offset == 16 and EDIT_DTYPE.fields["v"][1] == 16
    assert [f for f, _ in N.SensBatchOpts._fields_] == ["max_pivots", "chunk", "variant"]
    assert [f for f, _ in N.SensBatchResult._fields_] == ["finished", "running", "launches",
                                                          "form", "pivots"]
    assert ctypes.sizeof(N.SensBatchOpts) == 16 and ctypes.sizeof(N.SensBatchResult) == 24


def test_package_exports_the_batch():
    import lpr_381_group_v22_amd as pkg
    assert pkg.SensitivityBatch is pkg.sens_batch.SensitivityBatch
    assert "SensitivityBatch" in pkg.__all__


def test_pack_scripts_packs_and_refuses():
    from lpr_381_group_v22_amd.sens_batch import pack_scripts
    p = pack_scripts([[("change_rhs", 3, -50.0), ("resolve_all",)],
                      [],
                      [("change_nonbasic_column", (2, 8, 0.5)), ("change_basic", (1, 0.25)),
                       ("change_nonbasic_cbar", -1, 1.0)]])
    assert p.nedits.tolist() == [2, 0, 3] and p.nedits.dtype == np.int32
    assert p.edits["op"].tolist() == [3, 0, 4, 2, 1]
    assert p.edits["a"].tolist() == [3, 0, 2, 1, -1]
    assert p.edits["b"].tolist() == [0, 0, 8, 0, 0]
    assert p.edits["reserved"].tolist() == [0] * 5
    assert p.edits["v"].tolist() == [-50.0, 0.0, 0.5, 0.25, 1.0]
    assert p.edits.tobytes() == b"".join(
        np.array([op, a, b, 0], dtype=np.int32).tobytes() + np.float64(v).tobytes()
        for op, a, b, v in [(3, 3, 0, -50.0), (0, 0, 0, 0.0), (4, 2, 8, 0.5), (2, 1, 0, 0.25),
                            (1, -1, 0, 1.0)])
    # an index int32 cannot hold stays out of range instead of wrapping into range
    assert pack_scripts([[("change_nonbasic_cbar", 10 ** 12, 1.0)]]).edits["a"][0] == 2 ** 31 - 1
    bad = [
        [],                                              # no scenarios
        [[("add_activity", 5.0, [1.0, 2.0])]],           # changes the shape
        [[("resolve_all",)], [("add_constraint", [1.0], 1.0)]],
        [[("change_everything", 1)]],                    # unknown op
        [[("change_rhs", 1)]],                           # an argument short
        [[("change_rhs", 1.5, 2.0)]],                    # a fractional index
    ]
    for scripts in bad:
        with pytest.raises(ValueError):
            pack_scripts(scripts)
    with pytest.raises(ValueError, match="single handle"):
        pack_scripts([[("add_activity", 5.0, [1.0])]])


def test_form_rule_matches_the_header():
    """footprint_g is sens_batch_footprint_g, and G's budget is kBatchMaxLdsG."""
    from lpr_381_group_v22_amd import sens_batch as sb
    src = open(os.path.join(CSRC, "sens_batch_engine.hip")).read()
    assert "batch_pick_form(sens_batch_footprint_g(v.R, v.C), o.variant, false)" in src
    src = open(os.path.join(CSRC, "batch_common.hpp")).read()
    assert "fitG = bytes <= kBatchMaxLdsG" in src
    assert sb.MAX_LDS_G == 160 * 1024 - 1024
    assert sb.fits_g(8, 14) and sb.fits_g(33, 97) and not sb.fits_g(257, 769)
    ne = sens_batch_cases.largest_g_extra(60)
    assert sb.fits_g(61, 121 + ne) and not sb.fits_g(61, 122 + ne)


def test_constructed_cases_give_their_outcomes(oracle):
    """A guard on the fixtures, not a test of the batch: the constructions of the GPU tests on the
    oracle give outcomes 1, 2, 8 and -1 from the three constructed bases, 23 OK / 9 rolled back /
    59 pivots over the RHS sweep, and a stale base whose stored basicVars differ from a rebuild
    in a way the first edit of a script can see."""
    run = sens_batch_cases.oracle_run
    base, scripts = sens_batch_cases.unbounded_base(31)
    assert run(oracle, base, scripts[0])[1] == [1]
    base, scripts = sens_batch_cases.infeasible_base(32)
    assert run(oracle, base, scripts[0])[1] == [2]
    base, scripts = sens_batch_cases.rollback_base(33)
    assert run(oracle, base, scripts[0])[1] == [8, 0, 0, -1, 0]
    base, scripts = sens_batch_cases.rhs_sweep(oracle)
    refs = [run(oracle, base, s) for s in scripts]
    assert len(refs) == 32
    assert sum(r[1] == [0] for r in refs) == 23 and sum(r[1] == [8] for r in refs) == 9
    assert sum(r[2][0] for r in refs) == 59
    base, prefix, scripts = sens_batch_cases.stale_base()
    stored, rebuilt, differ = sens_batch_cases.stale_differs(oracle, base, prefix, scripts)
    assert stored == [0, 1, 9, 3, -1, 5] and rebuilt == [0, 1, 7, 3, -1, 5]
    assert {scripts[q][0] for q in differ} == {
        ("change_nonbasic_cbar", (7, 0.75)), ("change_nonbasic_cbar", (9, 0.75)),
        ("change_basic", (7, 0.25)), ("change_basic", (9, 0.25)),
        ("change_nonbasic_column", (1, 7, 0.5)), ("change_nonbasic_column", (1, 9, 0.5))}
