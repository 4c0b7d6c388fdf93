"""CPU tests of the batched revised simplex: the ABI declares the
lpr_rev_batch_* calls and the bindings have them, pack_revised_models flattens models as the
single-model path does and refuses what the constructor refuses, the Python form rule is the
header's, the kernels build for gfx950 without scratch and within the workgroup's LDS, the
tie-clause inputs are not vacuous, and the oracle agrees with the Python restatement on every
input the GPU tests use."""
import os
import re
import subprocess

import numpy as np
import pytest

import revised_batch_cases as rc
import special_values as sv
from ref_py import PyConstraint, PyRevised
from test_oracle_revised import STATUS, flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

CALLS = ["lpr_rev_batch_create", "lpr_rev_batch_destroy", "lpr_rev_batch_solve",
         "lpr_rev_batch_status_read", "lpr_rev_batch_solution_read", "lpr_rev_batch_basis_read",
         "lpr_rev_batch_log_read", "lpr_rev_batch_binv_read", "lpr_rev_batch_xb_read",
         "lpr_rev_batch_shape"]


def test_header_and_bindings_declare_the_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    gs = open(os.path.join(ROOT, "integration", "csharp", "GpuSolvers.cs")).read()
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"\b" + name + r"\s*\(", cs)) == 1, name
        assert "NativeMethods." + name + "(" in gs, name
    for struct in ("typedef struct lpr_rev_batch lpr_rev_batch;", "} lpr_rev_batch_opts;",
                   "} lpr_rev_batch_result;"):
        assert struct in text, struct
    assert [f for f, _ in N.RevBatchOpts._fields_] == ["max_pivots", "chunk", "variant"]
    assert [f for f, _ in N.RevBatchResult._fields_] == [
        "optimal", "unbounded", "infeasible", "other", "limit", "launches", "iterations"]
    assert "LprRevBatchOpts" in cs and "LprRevBatchResult" in cs


def test_pack_revised_models_matches_flat():
    from lpr_381_group_v22_amd import pack_revised_models
    cases = [c for _, c in rc.models()]
    p = pack_revised_models(cases)
    fl = [flat(cons) for _, cons, _ in cases]
    assert p.n.tolist() == [len(obj) for obj, _, _ in cases]
    assert p.m.tolist() == [len(cons) for _, cons, _ in cases]
    assert p.is_min.tolist() == [1 if mn else 0 for _, _, mn in cases]
    assert p.objective.tobytes() == np.concatenate(
        [np.asarray(obj, dtype=np.float64) for obj, _, _ in cases]).tobytes()
    assert p.A.tobytes() == np.concatenate([f[0].reshape(-1) for f in fl]).tobytes()
    assert p.b.tobytes() == np.concatenate([f[1] for f in fl]).tobytes()
    assert p.n.dtype == np.int32 and p.m.dtype == np.int32 and p.is_min.dtype == np.int8
    assert p.objective.dtype == p.A.dtype == p.b.dtype == np.float64


def test_constructor_errors_name_the_model():
    from lpr_381_group_v22_amd import pack_revised_models
    good = ([1.0], [PyConstraint([1.0], "<=", 1.0)], False)
    with pytest.raises(ValueError, match=r"model 1: Objective cannot be null or empty\."):
        pack_revised_models([good, ([], [PyConstraint([], "<=", 1.0)], False)])
    with pytest.raises(ValueError, match=r"model 2: Constraints cannot be null or empty\."):
        pack_revised_models([good, good, ([1.0], [], True)])
    with pytest.raises(ValueError,
                       match=r"model 0: Constraint 2 has incorrect number of coefficients\."):
        pack_revised_models([([1.0, 2.0], [PyConstraint([1.0, 1.0], "<=", 1.0),
                                           PyConstraint([1.0], "<=", 1.0)], False)])
    with pytest.raises(ValueError):
        pack_revised_models([])


def _const(text, name):
    return re.search(r"constexpr \w+ " + name + r"(?:\[\w+\])? = ([^;]+);", text).group(1)


def test_form_rule_matches_the_headers():
    from lpr_381_group_v22_amd import revised_batch as rb
    own = open(os.path.join(CSRC, "rev_batch_common.hpp")).read()
    common = open(os.path.join(CSRC, "batch_common.hpp")).read()
    eng = open(os.path.join(CSRC, "rev_batch_engine.hip")).read()
    # the formula is written once and the engine picks the form through it
    assert own.count("constexpr size_t rev_batch_footprint(") == 1
    assert "rev_batch_footprint(d.m, d.n)" in eng
    assert "batch_pick_form(fp * sizeof(double), o.variant)" in eng
    assert "(size_t)m * rev_batch_ld(m) + (size_t)m * rev_batch_ld(n) + rev_batch_vectors(m, n)" \
        in own
    assert "(size_t)kRevBatchVecM * m + n + (size_t)(n + m) + (size_t)(m + 1) / 2 +" in own
    assert "(size_t)(n + m + 7) / 8" in own and "return k | 1;" in own
    assert int(_const(own, "kRevBatchVecM")) == rb.VEC_M
    assert _const(own, "kRevBatchChunk") == "{%d, %d, %d}" % rb.CHUNK
    assert _const(common, "kBatchWgScratch") == "(size_t)1 << 10"
    assert _const(common, "kBatchWgLdsW") == "(size_t)64 << 10"
    assert _const(common, "kBatchMaxLdsW") == "(kBatchWgLdsW - kBatchWgScratch) / 4"
    assert _const(common, "kBatchMaxLdsG") == "((size_t)160 << 10) - kBatchWgScratch"
    assert rb.MAX_LDS_W == (65536 - 1024) // 4 and rb.MAX_LDS_G == 160 * 1024 - 1024
    assert (int(_const(common, "kBatchMaxRowsH")) - 1, int(_const(common, "kBatchMaxColsH")) - 1) \
        == (rb.MAX_M, rb.MAX_NM)

    def restated(m, n):  # B^-1 and A with odd leading dimensions, then the vectors
        return (m * (m + 1 - m % 2) + m * (n + 1 - n % 2) + 6 * m + n + (n + m) + -(-m // 2) +
                -(-(n + m) // 8))

    def form(m, n, variant):
        w, g = 8 * restated(m, n) <= rb.MAX_LDS_W, 8 * restated(m, n) <= rb.MAX_LDS_G
        if variant == 1 and w:
            return 0
        if variant == 2 and g:
            return 1
        if variant == 3:
            return 2
        return 0 if w else (1 if g else 2)

    shapes = rc.threshold_shapes()
    assert [f for _, _, _, f in shapes] == [0, 1, 1, 1, 2, 2]
    for _, m, n, f in shapes:
        assert rb.footprint(m, n) == restated(m, n)
        for variant in (0, 1, 2, 3):
            assert rb.pick_form(m, n, variant) == form(m, n, variant)
    (_, mw, nw, _), _, _, (_, mg, ng, _) = shapes[:4]
    assert 8 * rb.footprint(mw, nw) <= rb.MAX_LDS_W < 8 * rb.footprint(mw, nw + 1)
    assert 8 * rb.footprint(mg, ng) <= rb.MAX_LDS_G < 8 * rb.footprint(mg, ng + 1)
    assert rb.footprint(3, 4) == 3 * 3 + 3 * 5 + 18 + 4 + 7 + 2 + 1


def test_kernels_build_without_scratch(tmp_path):
    """rev_batch_kernels.hip alone, for gfx950, with the Makefile's flags: every kernel has a
    private segment of 0 bytes (no spills to scratch) and its static LDS stays within the
    workgroup scratch the forms leave free (kBatchWgScratch)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "rev_batch_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-fno-fast-math", "-DLPR_BUILD", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "rev_batch_kernels.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    s = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", s, flags=re.S)
    names = [k for k, _ in kernels]
    assert sum("k_rev_batchI" in k for k in names) == 3, names
    assert any("k_rev_batch_build" in k for k in names)
    for name, body in kernels:
        priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert priv == 0, (name, priv)
        assert lds <= 1024, (name, lds)


def test_tie_clause_inputs_are_not_vacuous():
    stats = [rc.tie_stats(mdl) for mdl in rc.tie_models()]
    assert len(stats) == 256
    optimal = sum(s[0] == "optimal" for s in stats)
    fired = sum(s[2] > 0 for s in stats)
    changed = sum(s[3] > 0 for s in stats)
    print("optimal", optimal, "tie clause fired in", fired, "LPs, changed the row in", changed)
    assert changed >= 10


def _gpu_inputs():
    """(name, model, max_pivots) of every LP tests/test_revised_batch_gpu.py solves, but for the
    one of m = 1023 (its own test below: it needs the oracle's generator)."""
    out = [(name, mdl, rc.CAP) for name, mdl in rc.models()]
    out += [(name, mdl, rc.CAP) for name, mdl in rc.threshold_models()]
    out += [(name, mdl, rc.CAP) for name, mdl in rc.degenerate_models()]
    out += [(f"mixed_{k}", mdl, rc.CAP) for k, mdl in enumerate(rc.mixed_models())]
    out += [("dup_70x12", rc.duplicated_rows(70, 12, 10, 2), rc.CAP),
            ("dup_130x9", rc.duplicated_rows(130, 9, 13, 4), rc.CAP),
            ("ieee_div", rc.ieee_div_model(), rc.CAP)]
    out += [(f"zero_skip_{k}", mdl, 500) for k, mdl in enumerate(rc.zero_skip_models())]
    out += [("special_" + name, rc.to_model(c, A, b), sv.REVISED_CAP)
            for name, c, A, b in sv.revised_cases()]
    return out


def _agrees(oracle, model, cap):
    obj, cons, is_min = model
    r = rc.oracle_ref(oracle, model, cap)
    p = PyRevised(obj, cons, is_min)
    ps = p.solve(max_iter=cap)
    assert ps == STATUS[r["status"]]
    assert [tuple(v) for v in r["log"].tolist()] == p.log
    assert r["basis"].tolist() == p.basic
    sv.assert_same(np.array(p.Binv), r["Binv"], "Binv")  # bytes, NaN bits excluded
    sv.assert_same(np.array(p.xB), r["xB"], "xB")
    if ps == "optimal":
        sv.assert_same(p.FinalZ, r["z"], "z")
        sv.assert_same(np.array(p.SolutionVector), r["x"], "x")


@pytest.mark.parametrize("name,model,cap", _gpu_inputs(), ids=[c[0] for c in _gpu_inputs()])
def test_oracle_equals_python_restatement_on_the_gpu_inputs(oracle, name, model, cap):
    _agrees(oracle, model, cap)


def test_oracle_equals_python_restatement_on_the_tie_set(oracle):
    for mdl in rc.tie_models():
        _agrees(oracle, mdl, rc.CAP)


def test_oracle_equals_python_restatement_on_the_h_limit_shape(oracle):
    c, A, b = oracle.gen_dense_lp(1023, 1024, 0)
    r = oracle.revised_solve(c, A, b, False, max_iter=4)
    assert (r["status"], r["iterations"]) == (5, 4)
    _agrees(oracle, rc.to_model(c, A, b), 4)


def test_constructed_inputs_do_what_the_gpu_tests_rely_on(oracle):
    r = rc.oracle_ref(oracle, rc.duplicated_rows(70, 12, 10, 2))
    assert (r["status"], r["iterations"]) == (2, 1)
    mdl = rc.duplicated_rows(130, 9, 13, 4)
    r = rc.oracle_ref(oracle, mdl)
    assert (r["status"], r["iterations"]) == (0, 11)
    assert rc.tie_stats(mdl)[1:] == (11, rc.tie_stats(mdl)[2], 1)
    r = rc.oracle_ref(oracle, rc.ieee_div_model())
    assert r["status"] == 0 and r["log"].tolist() == [[0, 0, 1]]
    assert float(r["Binv"][1][0]).hex() == "-0x1.6666666666667p-2"
    assert float(r["Binv"][0][0]).hex() == "0x1.0000000000003p-2"
    by_name = dict(rc.degenerate_models())
    assert rc.oracle_ref(oracle, by_name["zero_objective"])["status"] == 0
    assert rc.oracle_ref(oracle, by_name["zero_objective"])["iterations"] == 0
    r = rc.oracle_ref(oracle, by_name["zero_A"])
    assert (r["status"], r["iterations"]) == (1, 0)
