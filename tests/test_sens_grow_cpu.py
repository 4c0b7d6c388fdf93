"""CPU tests of the growing scenario batch (lpr_sens_batch_create_grow):
pack_grow_scripts packs the two add edits with their payload pool and passes the five
shape-keeping ops through as pack_scripts does; the ABI declares the new symbols; and the fixtures
of the GPU tests (tests/sens_grow_cases.py) are two-restatement checked -- the C oracle and the
Python restatement agree bit for bit on every one -- and reach the branches they are built for."""
import ctypes
import os
import re

import numpy as np
import pytest

import ref_py_sens as rp
import sens_batch_cases
import sens_grow_cases as grow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lpr_engine.h")


def test_header_and_bindings_declare_the_grow_calls():
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "csharp", "NativeMethods.cs")).read()
    for name in ("lpr_sens_batch_create_grow", "lpr_sens_batch_shape_read"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.SIGNATURES, name
        assert len(re.findall(r"static extern \w+ " + name + r"\(", cs)) == 1, name
    for op, code in [("ADD_ACTIVITY", 5), ("ADD_CONSTRAINT", 6)]:
        assert re.search(r"LPR_SENS_EDIT_%s = %d\b" % (op, code), text), op
        assert getattr(N, "LPR_SENS_EDIT_" + op) == code
    assert ctypes.sizeof(N.SensEdit) == 24
    assert pkg.SensitivityGrowBatch is pkg.sens_batch.SensitivityGrowBatch
    assert issubclass(pkg.SensitivityGrowBatch, pkg.SensitivityBatch)
    assert {"SensitivityGrowBatch", "pack_grow_scripts"} <= set(pkg.__all__)


def test_pack_grow_scripts_packs_edits_and_payload():
    from lpr_381_group_v22_amd.sens_batch import pack_grow_scripts, pack_scripts
    scripts = [[("add_activity", 5.5, [1.0, 2.0, 3.0]), ("change_rhs", 3, -50.0)],
               [],
               [("add_constraint", ([0.5, -0.25], 7.0)), ("resolve_all",),
                ("add_activity", (9.0, np.array([4.0]))), ("add_constraint", [], 1.5)]]
    p = pack_grow_scripts(scripts)
    assert p.nedits.tolist() == [2, 0, 4] and p.nedits.dtype == np.int32
    assert p.payload.dtype == np.float64
    assert p.payload.tobytes() == np.array([1.0, 2.0, 3.0, 0.5, -0.25, 4.0]).tobytes()
    assert p.edits.tobytes() == b"".join(
        np.array([op, a, b, 0], dtype=np.int32).tobytes() + np.float64(v).tobytes()
        for op, a, b, v in [(5, 0, 3, 5.5), (3, 3, 0, -50.0), (6, 3, 2, 7.0), (0, 0, 0, 0.0),
                            (5, 5, 1, 9.0), (6, 6, 0, 1.5)])
    # the five shape-keeping ops: exactly what pack_scripts gives
    old = [[("change_rhs", 3, -50.0), ("resolve_all",)], [],
           [("change_nonbasic_column", (2, 8, 0.5)), ("change_basic", (1, 0.25)),
            ("change_nonbasic_cbar", -1, 1.0), ("change_nonbasic_cbar", 10 ** 12, 1.0)]]
    a, b = pack_grow_scripts(old), pack_scripts(old)
    assert a.nedits.tobytes() == b.nedits.tobytes() and a.edits.tobytes() == b.edits.tobytes()
    assert a.payload.size == 0


def test_pack_grow_scripts_refuses():
    from lpr_381_group_v22_amd.sens_batch import pack_grow_scripts, pack_scripts
    bad = [
        [],                                              # no scenarios
        [[("add_activity", 5.0, ["x", 2.0])]],           # a non-numeric vector
        [[("add_activity", 5.0, 2.0)]],                  # a scalar where the vector goes
        [[("add_constraint", [[1.0], [2.0]], 1.0)]],     # not one-dimensional
        [[("add_constraint", [1.0, 2.0], "rhs")]],       # a non-numeric value
        [[("add_activity", 5.0)]],                       # a missing argument
        [[("add_constraint", [1.0])]],
        [[("resolve_all",)], [("add_everything", [1.0], 1.0)]],   # unknown op
        [[("change_rhs", 1)]],                           # the old ops keep their checks
        [[("change_rhs", 1.5, 2.0)]],
    ]
    for scripts in bad:
        with pytest.raises(ValueError):
            pack_grow_scripts(scripts)
    with pytest.raises(ValueError, match="single handle"):       # the old call keeps refusing
        pack_scripts([[("add_constraint", [1.0], 1.0)]])


def _both(oracle, name, base, ops, prefix=()):
    """The oracle and the Python restatement on one script: the same outcome and the same bits
    after every edit.  Returns what grow.follow returns."""
    T, x, z, basis = base
    script, ref, shapes = grow.follow(oracle, base, ops, prefix)
    o = oracle.sens(T, x, z, basis)
    p = rp.PySens(T.tolist(), list(map(float, x)), float(z), [int(b) for b in basis])
    for k, (op, args) in enumerate(list(prefix) + script):
        rc = getattr(o, op)(*args)
        prc = rp.run(getattr(p, op), *args)
        assert (0 if prc is None else prc) == rc, (name, k, op, rc, prc)
        st = o.state()
        assert np.array(p.t).tobytes() == st["T"].tobytes(), (name, k, op)
        assert np.array(p.t).shape == st["T"].shape, (name, k, op)
        assert p.basic == st["basic"], (name, k, op)
        assert np.array(p.sol).tobytes() == st["sol"].tobytes(), (name, k, op)
        assert p.z == st["z"] or (p.z != p.z and st["z"] != st["z"]), (name, k, op)
        assert p.log == o.log(), (name, k, op)
    assert shapes[-1:] == [o.state()["T"].shape][:len(shapes)], name
    return script, ref, shapes


def test_fixtures_agree_between_the_two_restatements_and_reach_their_branches(oracle):
    from lpr_381_group_v22_amd import sens_batch as sb
    # (1) every op alone and in order, and the constructed outcomes with a script after them
    seen, hit = set(), {1: 0, 2: 0}
    for name, base, scripts in grow.all_edit_cases(oracle):
        R0, C0 = base[0].shape
        for ops in scripts:
            script, ref, shapes = _both(oracle, name, base, ops)
            seen |= set(ref[1])
        for tail, code in ((scripts[-2], 2), (scripts[-1], 1)):
            script, ref, shapes = grow.follow(oracle, base, tail)
            hit[code] += ref[1][-4] == code
            assert shapes[-4][0] > R0 and shapes[-1][1] == shapes[-4][1] + 1, (name, shapes)
    assert hit[2] >= 4 and hit[1] == 5, hit
    assert {0, 1, 2, 8, -1} <= seen, seen
    # (2) mixed shapes: 0..3 growth edits in one batch
    base, scripts = grow.mixed_shapes(oracle)
    finals = set()
    for q, ops in enumerate(scripts):
        shapes = _both(oracle, ("mixed", q), base, ops)[2]
        finals.add(shapes[-1] if shapes else base[0].shape)
    assert len(finals) >= 5, finals
    # (3) the stale base: 9 from add_constraint, nothing changed, the script goes on
    base, prefix, _ = sens_batch_cases.stale_base()
    R, Cc = base[0].shape
    before = sens_batch_cases.oracle_run(oracle, base, [], prefix)[0].state()
    assert before["basic"][4] == -1
    scripts = grow.stale_scripts(Cc - 1, R)
    refs = [_both(oracle, ("stale", q), base, ops, prefix) for q, ops in enumerate(scripts)]
    assert refs[0][1][1] == [9] and refs[1][1][1][0] == 9 and refs[1][1][1][1] != 9
    after = refs[0][1][0].state()
    assert after["T"].tobytes() == before["T"].tobytes() and after["basic"] == before["basic"]
    assert after["z"] == before["z"]
    assert refs[2][1][1] == [0] and refs[2][2] == [(R, Cc + 1)]
    # (4) aX over a stale solution vector
    base, ops = grow.stale_solution_case()
    script, ref, shapes = _both(oracle, "stale sol", base, ops)
    assert ref[1][0] == 1 and ref[2][0] >= 1, (ref[1], ref[2])
    o1 = sens_batch_cases.oracle_run(oracle, base, script[:1])[0].state()
    assert o1["sol"].tobytes() == np.asarray(base[1], dtype=np.float64).tobytes()   # not refreshed
    assert o1["T"].tobytes() != np.asarray(base[0]).tobytes()                       # but moved
    tech = np.array(script[1][1][0])
    assert float(tech[:len(base[1])] @ o1["sol"]) != 0.0
    assert ref[1][1] != -1 and ref[1][1] != 9
    # (5) the rollback restores the grown tableau
    base, ops = grow.rollback_growth_case()
    script, ref, shapes = _both(oracle, "rollback", base, ops)
    R, Cc = base[0].shape
    assert ref[1][0] == 0 and ref[1][1] == 8 and ref[1][2] in (0, 2) and ref[1][3] in (0, 8)
    assert shapes == [(R, Cc + 1), (R, Cc + 1), (R + 1, Cc + 2), (R + 1, Cc + 2)]
    # (6) lane strides, with pivots after the growth
    for name, base, ops, form in grow.stride_cases():
        script, ref, shapes = _both(oracle, name, base, ops)
        R, Cc = base[0].shape
        grown = shapes[[op for op, _ in script].index("change_nonbasic_cbar")]
        assert sb.fits_g(*grown) == (form == 1), (name, grown)
        assert sum(ref[2]) > 0 and -1 not in ref[1] and 9 not in ref[1], (name, ref[1], ref[2])
        assert {"cols_255_257": (Cc, grown[1]) == (255, 257),
                "cols_63_65": (Cc, grown[1]) == (63, 65),
                "rows_64_65": (R, grown[0]) == (64, 65)}[name], (name, base[0].shape, grown)
    # (7) the form boundary
    ne = sens_batch_cases.largest_g_extra(60)
    base, scripts = grow.boundary_case(ne)
    R, Cc = base[0].shape
    assert sb.fits_g(R, Cc) and not sb.fits_g(R, Cc + 1)
    for ops in scripts:
        _both(oracle, "boundary", base, ops)
    base, scripts = grow.boundary_case(ne - 1)
    assert sb.fits_g(base[0].shape[0], base[0].shape[1] + 1)
    assert sum(sum(_both(oracle, "below boundary", base, ops)[1][2]) for ops in scripts) > 0
