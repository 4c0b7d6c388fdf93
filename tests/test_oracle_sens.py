"""CPU tests: the C oracle of the sensitivity re-solve (SensitivityAnalyzer.cs) against the
independent Python restatement, edit by edit.  PARITY UNPINNED by the reference (no tests)."""
import numpy as np

import ref_py_sens as rp
import sens_cases


def test_edit_scripts(oracle):
    codes = set()
    for name, (T, x, z, basis), ops in sens_cases.scripts(oracle):
        o = oracle.sens(T, x, z, basis)
        p = rp.PySens(T.tolist(), list(map(float, x)), float(z), [int(b) for b in basis])
        st = o.state()
        assert np.array(p.t).tobytes() == st["T"].tobytes() and p.basic == st["basic"], name
        for k, (op, args) in enumerate(ops):
            op, args = sens_cases.materialize(op, args, o.state()["T"], k)
            rc = getattr(o, op)(*args)
            prc = rp.run(getattr(p, op), *args)
            prc = 0 if prc is None else prc
            assert prc == rc, (name, k, op, rc, prc)
            st = o.state()
            assert np.array(p.t).tobytes() == st["T"].tobytes(), (name, k, op)
            assert p.basic == st["basic"], (name, k, op)
            assert np.array(p.sol).tobytes() == st["sol"].tobytes(), (name, k, op)
            assert p.z == st["z"], (name, k, op)
            assert p.log == o.log(), (name, k, op)
            codes.add(rc)
    assert {0, -1, 8} <= codes and (1 in codes or 2 in codes), codes


def test_resolve_keeps_an_optimal_tableau_unchanged(oracle):
    T, x, z, basis = sens_cases.solved_lp(oracle, 8, 12, 1)
    o = oracle.sens(T, x, z, basis)
    before = o.state()
    assert o.resolve_all() == 0
    after = o.state()
    assert after["T"].tobytes() == before["T"].tobytes()
    assert abs(after["z"] - z) == 0.0


def _replay(oracle, base, ops):
    T, x, z, basis = base
    o = oracle.sens(T, x, z, basis)
    codes, logs = [], []
    for k, (op, args) in enumerate(ops):
        n0 = len(o.log())
        op, args = sens_cases.materialize(op, args, o.state()["T"], k)
        codes.append(getattr(o, op)(*args))
        logs.append(o.log()[n0:])
    return o, codes, logs


def test_stride_scripts_are_decided_by_the_planted_candidates(oracle):
    """The GPU shape tests (test_side_shapes_gpu.py) plant the deciding candidates of the
    sensitivity folds one or more 1024-lane strides apart; the oracle confirms that they decide."""
    scripts = sens_cases.stride_scripts()
    shapes = set()
    for name, base, ops, expect in scripts:
        T = base[0]
        R, C = T.shape
        o, codes, logs = _replay(oracle, base, ops)
        assert codes == [0] * len(ops), (name, codes)
        for op_i, k, field, value in expect:
            assert len(logs[op_i]) > k, (name, op_i)
            assert logs[op_i][k][field] == value, (name, op_i, logs[op_i][k], value)
        if R - 1 > 1024:
            shapes.add("tall")
        if C - 1 > 16384:
            shapes.add("uncached")
        elif C - 1 > 1024 and R - 1 > 64:
            shapes.add("wide")
    assert shapes == {"tall", "uncached", "wide"}


def test_stride_scripts_reach_their_branches(oracle):
    """The preconditions the GPU shape tests rely on."""
    by_name = {s[0]: s for s in sens_cases.stride_scripts()}
    # change_basic on a column whose basic row lies past the first stride
    _, base, ops, _ = by_name["leave_rows_exact"]
    col = ops[1][1][0]
    o, codes, logs = _replay(oracle, base, ops[:1])
    assert o.state()["basic"].index(col) + 1 > 1024
    # more than kFoldCap = 1024 strictly decreasing prefix minima on the leaving row
    for name in ("prefix_minima_step1", "prefix_minima_in_band"):
        _, (T, *_), ops, _ = by_name[name]
        r = ops[0][1][0]
        cand = [j for j in range(T.shape[1] - 1) if T[r, j] < -1e-9]
        ratios = [T[0, j] / -T[r, j] for j in cand]
        assert len(cand) > 1024 and all(a > b for a, b in zip(ratios, ratios[1:])), name
    # the analyzer grows past 1024 rows twice and by four columns
    _, base, ops, _ = by_name["grow_tall"]
    o, codes, logs = _replay(oracle, base, ops)
    R0, C0 = base[0].shape
    assert R0 - 1 > 1024 and o.state()["T"].shape == (R0 + 2, C0 + 4)
