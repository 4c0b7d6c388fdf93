"""Bases and scripts for the sensitivity scenario batch tests (TEST ONLY).  A script here is a list
of (op, args) with the five ops that keep the tableau's shape; the oracle runs each script alone on
a fresh analyzer, and that run is what a scenario of a batch is compared with."""
from __future__ import annotations

import math

import numpy as np

import sens_cases

SHAPE_KEEPING = ("resolve_all", "change_nonbasic_cbar", "change_basic", "change_rhs",
                 "change_nonbasic_column")


def keep_shape(ops):
    return [(op, tuple(args)) for op, args in ops if op in SHAPE_KEEPING]


def oracle_run(oracle, base, script, prefix=()):
    """The script alone on a fresh oracle analyzer holding `base` (after `prefix`, edits that
    bring the analyzer to the base state of a stale handle).  Returns (analyzer, outcomes, pivots
    per edit, log entries the prefix left)."""
    T, x, z, basis = base
    o = oracle.sens(T, x, z, basis)
    for op, args in prefix:
        getattr(o, op)(*args)
    skip = len(o.log())
    outs, pivs = [], []
    for op, args in script:
        n0 = len(o.log())
        outs.append(getattr(o, op)(*args))
        pivs.append(len(o.log()) - n0)
    return o, outs, pivs, skip


def same_scenario(batch, k, ref, tag):
    """Scenario k against oracle_run's result, as sens_cases.same_state compares: outcome and
    pivots per edit, log, tableau bytes, basicVars, z, and the solution bytes and length."""
    o, outs, pivs, skip = ref
    st = o.state()
    assert batch.Outcomes(k) == outs, (tag, batch.Outcomes(k), outs)
    assert batch.Pivots(k) == pivs, (tag, batch.Pivots(k), pivs)
    log = o.log()[skip:]
    assert batch.LogCount(k) == len(log), tag
    assert batch.Log(k) == log[:batch.LogCap], tag
    got = batch.State(k)
    assert got["T"].shape == st["T"].shape, tag
    assert got["T"].tobytes() == st["T"].tobytes(), tag
    assert got["basic"] == st["basic"], tag
    assert got["sol"].shape == st["sol"].shape, tag
    assert got["sol"].tobytes() == st["sol"].tobytes(), tag
    assert got["z"] == st["z"] or (math.isnan(st["z"]) and math.isnan(got["z"])), tag


def unbounded_base(seed):
    """identity_basis(6, 4) with nonbasic column 7 made <= 0: a negative reduced cost there has no
    leaving row.  change_nonbasic_cbar(7, -1.0) gives outcome 1."""
    T, x, z, basis = sens_cases.identity_basis(6, 4, seed)
    T[1:, 7] = -np.abs(T[1:, 7])
    return (T, x, z, basis), [[("change_nonbasic_cbar", (7, -1.0))],
                              [("change_nonbasic_cbar", (7, -1.0)), ("resolve_all", ())]]


def infeasible_base(seed):
    """identity_basis(6, 4) with row 3 made non-negative and its RHS -2: the dual simplex finds no
    entering column.  resolve_all gives outcome 2."""
    T, x, z, basis = sens_cases.identity_basis(6, 4, seed)
    T[3, :-1] = np.abs(T[3, :-1])
    T[3, -1] = -2.0
    x[2] = -2.0
    return (T, x, z, basis), [[("resolve_all", ())],
                              [("resolve_all", ()), ("change_basic", (1, 0.5))]]


def rollback_base(seed):
    """identity_basis(6, 4) with row 3 made non-negative: change_rhs(3, -50.0) is rolled back
    (outcome 8), and the script goes on: change_rhs(3, 7.0), change_basic and
    change_nonbasic_column give 0, the invalid index -1."""
    T, x, z, basis = sens_cases.identity_basis(6, 4, seed)
    T[3, :-1] = np.abs(T[3, :-1])
    script = [("change_rhs", (3, -50.0)), ("change_rhs", (3, 7.0)), ("change_basic", (2, 0.25)),
              ("change_nonbasic_cbar", (-1, 1.0)), ("change_nonbasic_column", (2, 8, 0.5))]
    return (T, x, z, basis), [script, script[:1], script[:2]]


def all_edit_cases(oracle):
    """[(name, base, [script, ...])]: the five bases of sens_cases.scripts with every
    shape-keeping op alone and the full script in order, plus the three constructed bases."""
    out = []
    for name, base, ops in sens_cases.scripts(oracle):
        full = keep_shape(ops)
        out.append((name, base, [[e] for e in full] + [full]))
    out.append(("unbounded", *unbounded_base(31)))
    out.append(("infeasible", *infeasible_base(32)))
    out.append(("rollback", *rollback_base(33)))
    return out


def rhs_sweep(oracle):
    """The 32 change_rhs scenarios on solved_lp(oracle, 8, 12, 1): k = 1..8, new b in
    {0, b / 2, 2 b, -3}."""
    base = sens_cases.solved_lp(oracle, 8, 12, 1)
    T = base[0]
    scripts = []
    for k in range(1, 9):
        b = float(T[k, -1])
        for nb in (0.0, 0.5 * b, 2.0 * b, -3.0):
            scripts.append([("change_rhs", (k, nb))])
    return base, scripts


def largest_g_extra(m):
    """n_extra of the widest identity_basis(m, n_extra) that form G takes."""
    from lpr_381_group_v22_amd.sens_batch import fits_g
    n_extra = 1
    while fits_g(m + 1, 2 * m + n_extra + 2):
        n_extra += 1
    return n_extra


def threshold_case(m, n_extra, seed):
    """An identity basis with work in it: a negative reduced cost, then an RHS pushed negative."""
    base = sens_cases.identity_basis(m, n_extra, seed)
    T = base[0]
    k = m // 2
    script = [("change_nonbasic_cbar", (m + 1, -0.75)),
              ("change_rhs", (k, -float(T[k, -1]))),
              ("change_basic", (3, 0.5)),
              ("resolve_all", ())]
    return base, [script, script[:2], script[1:2]]


def stale_base(seed=34):
    """(base, prefix, scripts): identity_basis(6, 4) whose stored basicVars, after `prefix` has run
    on it, is not what a rebuild gives.  Columns 7 and 9 hold the same constraint rows, and column
    9 has the cheaper dual ratio in row 3: the prefix change_rhs drives row 3 to -0.4 and pivots
    (3, 9), after which both are the unit column of row 3.  The pivot stored 9 in basicVars[2]; a
    rebuild takes the first such column, 7.  Row 5 has no unit column (its basic entry is 2), so
    basicVars[4] is -1 from the constructor on.  The scripts start with change_nonbasic_cbar or
    change_basic on every column, so those on 7 and 9 read the stale entry."""
    T, x, z, basis = sens_cases.identity_basis(6, 4, seed)
    T[3, 6:10] = np.abs(T[3, 6:10])
    T[1:, 9] = T[1:, 7]
    T[3, 7] = T[3, 9] = -4.0
    T[0, 7], T[0, 9] = 1.0, 0.5
    T[5, 4] = 2.0
    b, s3 = float(T[3, -1]), float(T[3, 10 + 2])
    prefix = [("change_rhs", (3, b + (-0.4 - b) / s3))]
    ncols = T.shape[1] - 1
    scripts = [[("change_nonbasic_cbar", (j, 0.75))] for j in range(ncols)]
    scripts += [[("change_basic", (j, 0.25)), ("change_rhs", (2, 1.0))] for j in range(ncols)]
    scripts += [[("change_nonbasic_column", (1, j, 0.5))] for j in (7, 9)]
    return (T, x, z, basis), prefix, scripts


def stale_differs(oracle, base, prefix, scripts):
    """(stored basicVars after the prefix, basicVars a rebuild gives, scripts whose first outcome
    differs between the stale base and the rebuilt one)."""
    T, x, z, basis = base
    o = oracle.sens(T, x, z, basis)
    for op, args in prefix:
        assert getattr(o, op)(*args) == 0
    stored = o.state()["basic"]
    assert o.resolve_all() == 0
    rebuilt = o.state()["basic"]
    differ = [q for q, s in enumerate(scripts)
              if oracle_run(oracle, base, s, prefix)[1][0]
              != oracle_run(oracle, base, s, list(prefix) + [("resolve_all", ())])[1][0]]
    return stored, rebuilt, differ
