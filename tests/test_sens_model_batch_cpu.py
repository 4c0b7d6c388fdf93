"""CPU tests of the fixtures of test_sens_model_batch_gpu.py (tests/sens_model_batch_cases.py) and
of the host side of the scenario batch built from an LP batch (lpr_sens_batch_from_batch, DESIGN.md
section 20): every base is optimal on the oracle, the scripts reach the outcomes {0, 1, 2, 8, -1},
the C oracle and the Python restatement agree bit for bit on every case, pack_grow_scripts packs
every script, and the constructed tableaux hold what their names say -- so the GPU test cannot pass
vacuously."""
import os
import re

import numpy as np

import ref_py_sens as rp
import sens_model_batch_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")
EPS = 1e-9


def _both(oracle, name, base, ops):
    """The oracle and the Python restatement on one script over one base: the same constructor
    state, the same outcome and the same bits after every edit.  Returns mc.grow.follow's result."""
    T, x, z, basis = base
    script, ref, shapes = mc.grow.follow(oracle, base, ops)
    o = oracle.sens(T, x, z, basis)
    p = rp.PySens(T.tolist(), list(map(float, x)), float(z), [int(b) for b in basis])

    def same(tag):
        st = o.state()
        assert np.array(p.t).shape == st["T"].shape, (name, tag)
        assert np.array(p.t).tobytes() == st["T"].tobytes(), (name, tag)
        assert p.basic == st["basic"], (name, tag)
        assert np.array(p.sol).tobytes() == st["sol"].tobytes(), (name, tag)
        assert p.z == st["z"] or (p.z != p.z and st["z"] != st["z"]), (name, tag)
        assert p.log == o.log(), (name, tag)

    same("ctor")
    for k, (op, args) in enumerate(script):
        rc = getattr(o, op)(*args)
        prc = rp.run(getattr(p, op), *args)
        assert (0 if prc is None else prc) == rc, (name, k, op, rc, prc)
        same((k, op))
    return script, ref, shapes


def _well_formed(scripts, shapes0):
    """pack_grow_scripts output against the scripts: counts, ops in 0..6, payload ranges disjoint
    and in order, and lengths that fit the shape the script has reached."""
    from lpr_381_group_v22_amd.sens_batch import EDIT_DTYPE, pack_grow_scripts
    p = pack_grow_scripts(scripts)
    assert p.nedits.dtype == np.int32 and p.nedits.tolist() == [len(s) for s in scripts]
    assert p.edits.dtype == EDIT_DTYPE and p.edits.size == sum(len(s) for s in scripts)
    assert p.payload.dtype == np.float64
    at, q = 0, 0
    for k, script in enumerate(scripts):
        rows, cols = shapes0[k]
        for op, args in script:
            e = p.edits[q]
            q += 1
            assert 0 <= e["op"] <= 6 and e["reserved"] == 0, (k, op)
            if op == "add_activity":
                assert (e["op"], e["a"], e["b"]) == (5, at, rows - 1) and e["v"] == args[0], (k, op)
                assert p.payload[at:at + e["b"]].tobytes() == np.asarray(args[1], float).tobytes()
                at += e["b"]
                cols += 1
            elif op == "add_constraint":
                assert (e["op"], e["a"], e["b"]) == (6, at, cols - 1) and e["v"] == args[1], (k, op)
                assert p.payload[at:at + e["b"]].tobytes() == np.asarray(args[0], float).tobytes()
                at += e["b"]
                rows += 1
                cols += 1
    assert at == p.payload.size
    return p


def test_header_and_bindings_declare_the_call():
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    gs = open(os.path.join(ROOT, "integration", "csharp", "GpuSolvers.cs")).read()
    for name in ("lpr_sens_batch_from_batch", "lpr_sens_batch_from_batch_time"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"static extern \w+ " + name + r"\(", cs)) == 1, name
    assert "NativeMethods.lpr_sens_batch_from_batch(" in gs
    assert re.search(r"#define LPR_ABI_VERSION 1\b", open(HEADER).read())
    assert issubclass(pkg.SensitivityModelBatch, pkg.SensitivityGrowBatch)
    assert {"SensitivityModelBatch", "optimal_items"} <= set(pkg.__all__)


def test_every_fixture_model_is_optimal_except_the_refusals(oracle):
    models = mc.shape_models() + [mc.large_model()]
    shapes = set()
    for q, model in enumerate(models):
        st, base = mc.solve(oracle, model)
        assert st == mc.OPTIMAL, q
        shapes.add(base[0].shape)
        assert base[0].shape[1] >= base[0].shape[0]
    assert {(2, 3), (3, 6), (4, 6), (9, 21), (34, 98), (200, 300)} <= shapes, shapes
    assert {63, 64, 65} <= {s[1] for s in shapes}
    assert mc.solve(oracle, mc.unbounded_model())[0] == mc.UNBOUNDED
    obj, cons, is_max = mc.many_pivot_model()
    o, A, ncoef, rel, rhs = mc.lp_cases.flatten(obj, cons)
    T, basis = oracle.primal_build(o, A, rel, rhs, is_max, ncoef)
    assert oracle.primal_solve(T, basis)[1] > 1
    assert mc.tall_tableau().shape[1] < mc.tall_tableau().shape[0]
    W = mc.wide_optimal_tableau()
    assert W.shape == (3, 2048) and (W[0, :-1] >= 0).all()


def test_scripts_reach_every_outcome_and_both_restatements_agree(oracle):
    from lpr_381_group_v22_amd import sens_batch as sb
    seen, ops_seen, finals = set(), set(), set()
    for name, case in (("mixed", mc.mixed_case(oracle)), ("every_op", mc.every_op_case(oracle))):
        models, bases, items, ops_list = case
        assert max(items) == len(bases) - 1 and min(items) == 0
        scripts, shapes0 = [], []
        for k, (it, ops) in enumerate(zip(items, ops_list)):
            script, ref, shapes = _both(oracle, (name, k), bases[it], ops)
            scripts.append(script)
            shapes0.append(bases[it][0].shape)
            seen |= set(ref[1])
            ops_seen |= {op for op, _ in script}
            finals.add(shapes[-1] if shapes else bases[it][0].shape)
        p = _well_formed(scripts, shapes0)
        assert set(p.edits["op"].tolist()) == set(range(7)), name
    assert {0, 1, 2, 8, -1} <= seen, seen
    assert ops_seen == set(sb.EDIT_OPS) | set(sb.SHAPE_CHANGING_OPS), ops_seen
    assert len(finals) >= 12, finals
    # the mixed batch: permuted, one LP under three different scripts
    _, _, items, ops_list = mc.mixed_case(oracle)
    assert items != sorted(items) and items.count(2) == 3
    assert len({repr([op for op, _ in ops_list[k]]) for k, it in enumerate(items) if it == 2}) == 3
    # the forms case: the large LP alone forces form H
    models, bases, items, ops_list, shared = mc.forms_case(oracle)
    scripts, shapes0 = [], []
    for k, (it, ops) in enumerate(zip(items, ops_list)):
        scripts.append(_both(oracle, ("forms", k), bases[it], ops)[0])
        shapes0.append(bases[it][0].shape)
    _well_formed(scripts, shapes0)
    assert not sb.fits_g(*bases[3][0].shape)
    assert all(items[k] != 3 and sb.fits_g(bases[items[k]][0].shape[0] + 3,
                                           bases[items[k]][0].shape[1] + 3) for k in shared)


def test_constructed_tableaux_hold_what_they_are_built_for(oracle):
    seen_minus_one = 0
    for name, T in mc.disagreement_tableaux():
        assert T.shape[1] >= T.shape[0] and (T[0, :-1] >= 0).all(), name
        base = mc.tableau_base(oracle, T)
        st = oracle.sens(*base).state()
        assert st["T"].tobytes() == T.tobytes() and st["z"] == T[0, -1], name
        seen_minus_one += -1 in st["basic"]
        for q, ops in enumerate(mc.tableau_ops(T)):
            _both(oracle, (name, q), base, ops)
        if name == "twin_unit_columns":
            assert st["basic"] == [0, 1, -1]                       # the first of the twins
            assert (T[1:, 1] == T[1:, 5]).all() and base[1][1] == T[2, -1]
            assert T[1, -1] == 0.0 and base[1][0] == 0.0           # degenerate: basic at 0
        if name == "two_ones_in_a_column":
            assert abs(T[2, 0] - 1.0) < EPS and T[2, 0] != 1.0
            assert base[1][0] == 0.0 and base[1][1] == 0.0 and base[1][2] == T[3, -1]
            assert 0 not in st["basic"] and 1 not in st["basic"]
        if name == "threshold_entries":
            x = base[1]
            inside = [abs(T[1, q] - 1.0) < EPS for q in range(6)]
            assert True in inside and False in inside
            assert [x[q] == T[1, -1] for q in range(6)] == inside
            small = [not abs(T[3, 6 + q]) > EPS for q in range(6)]
            assert True in small and False in small
            assert [x[6 + q] == T[2, -1] for q in range(6)] == small
            first = 6 + small.index(True)
            assert st["basic"][1] == first and st["basic"][0] == inside.index(True)
    assert seen_minus_one >= 1
