"""CPU tests of the batched primal simplex: the ABI declares the lpr_batch_*
calls and the binding has them, pack_models flattens models exactly as the single-model path
does, malformed models are refused, and the batch kernels build for gfx950 without scratch and
within the workgroup's LDS."""
import os
import re
import subprocess

import numpy as np
import pytest

import lp_cases
from ref_py import PyConstraint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
CSRC = os.path.join(ROOT, "lpr_381_group_v22_amd", "csrc")

BATCH_CALLS = ["lpr_batch_from_lps", "lpr_batch_create", "lpr_batch_destroy", "lpr_batch_solve",
               "lpr_batch_status_read", "lpr_batch_solution_read", "lpr_batch_basis_read",
               "lpr_batch_log_read", "lpr_batch_tableau_read", "lpr_batch_shape"]


def test_header_and_binding_declare_the_batch_calls():
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in BATCH_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
    assert "typedef struct lpr_batch lpr_batch;" in text


def test_pack_models_matches_flatten():
    from lpr_381_group_v22_amd import pack_models
    cases = [c for _, c in lp_cases.all_cases()]
    p = pack_models(cases)
    flat = [lp_cases.flatten(obj, cons) for obj, cons, _ in cases]
    assert p.n.tolist() == [len(obj) for obj, _, _ in cases]
    assert p.m.tolist() == [len(cons) for _, cons, _ in cases]
    assert p.is_max.tolist() == [1 if mx else 0 for _, _, mx in cases]
    assert p.objective.tobytes() == np.concatenate([f[0] for f in flat]).tobytes()
    assert p.A.tobytes() == np.concatenate([f[1].reshape(-1) for f in flat]).tobytes()
    assert p.ncoef.tobytes() == np.concatenate([f[2] for f in flat]).tobytes()
    assert p.relation.tobytes() == np.concatenate([f[3] for f in flat]).tobytes()
    assert p.rhs.tobytes() == np.concatenate([f[4] for f in flat]).tobytes()
    assert p.n.dtype == np.int32 and p.relation.dtype == np.int8 and p.is_max.dtype == np.int8


def test_pack_models_ragged_and_relations():
    from lpr_381_group_v22_amd import pack_models
    p = pack_models([([1.0, 2.0], [PyConstraint([5.0, 6.0, 7.0], ">=", 3.0),
                                   PyConstraint([], "=", 1.0),
                                   PyConstraint([4.0], "<", 2.0)], False)])
    assert p.ncoef.tolist() == [2, 0, 1]
    assert p.relation.tolist() == [1, 2, 0]  # anything but ">=" / "=" is "<=" (:36-50)
    assert p.A.tolist() == [5.0, 6.0, 0.0, 0.0, 4.0, 0.0]
    assert p.is_max.tolist() == [0]


@pytest.mark.parametrize("models", [
    [],
    [([1.0], [PyConstraint([1.0], "<=", 1.0)])],                   # not a triple
    [("12", [], True)],                                           # objective is a string
    [([1.0, "x"], [], True)],                                     # non-number in the objective
    [([1.0], [PyConstraint(["a"], "<=", 1.0)], True)],            # non-number coefficient
    [([1.0], [PyConstraint([1.0], "<=", "b")], True)],            # non-number RHS
    [([1.0], [PyConstraint([1.0], 2, 1.0)], True)],               # relation is not a string
    [([1.0], [(1.0, "<=", 1.0)], True)],                          # not a Constraint
    [([], [], True)],                                             # no variables, no rows
    [([1.0], [], "yes")],                                         # isMaximization not a bool
    [([True, False], [], True)],                                  # bools are not coefficients
])
def test_pack_models_refuses_malformed(models):
    from lpr_381_group_v22_amd import pack_models
    with pytest.raises(ValueError):
        pack_models(models)


def test_batch_kernels_build_without_scratch(tmp_path):
    """batch_kernels.hip alone, for gfx950, with the Makefile's flags: every batch kernel has a
    private segment of 0 bytes (no spills) and its static LDS leaves the dynamic share its form
    needs within 160 KiB."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "batch_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                    "-fno-fast-math", "-DLPR_BUILD", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "batch_kernels.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    s = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", s, flags=re.S)
    names = [k for k, _ in kernels]
    assert sum("k_batch_simplex" in k for k in names) == 3, names
    assert any("k_batch_build" in k for k in names) and any("k_batch_extract" in k for k in names)
    for name, body in kernels:
        priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert priv == 0, (name, priv)
        assert lds <= 1024, (name, lds)  # the reserved workgroup scratch (kBatchWgScratch)
        assert lds <= 160 * 1024
