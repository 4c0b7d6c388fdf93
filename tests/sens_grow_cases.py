"""Bases and scripts for the tests of the growing scenario batch (TEST ONLY): scripts that hold
add_activity and add_constraint beside the five shape-keeping ops.  The arguments of an add edit
depend on the shape the analyzer has when the edit runs, so a script is written with callables
where that matters and `follow` fills them in along an oracle run of the script alone; that run is
also what a scenario of a batch is compared with (sens_batch_cases.same_scenario)."""
from __future__ import annotations

import numpy as np

import sens_batch_cases
import sens_cases


def follow(oracle, base, ops, prefix=()):
    """(script, ref, shapes): `ops` with the sens_cases placeholders and callables (T -> args)
    filled in from the tableau the oracle holds at that point; ref as sens_batch_cases.oracle_run
    returns it; shapes[q] the oracle's tableau shape after edit q."""
    T, x, z, basis = base
    o = oracle.sens(T, x, z, basis)
    for op, args in prefix:
        getattr(o, op)(*args)
    skip = len(o.log())
    script, outs, pivs, shapes = [], [], [], []
    for k, (op, args) in enumerate(ops):
        now = o.state()["T"]
        if callable(args):
            args = args(now)
        op, args = sens_cases.materialize(op, tuple(args), now, k)
        n0 = len(o.log())
        outs.append(getattr(o, op)(*args))
        pivs.append(len(o.log()) - n0)
        shapes.append(o.state()["T"].shape)
        script.append((op, tuple(args)))
    return script, (o, outs, pivs, skip), shapes


def activity(seed, c_new=7.0):
    """add_activity arguments for whatever shape the analyzer has: a column in [0.1, 1)."""
    return lambda T: (c_new, np.random.RandomState(seed).uniform(0.1, 1.0,
                                                                 size=T.shape[0] - 1).tolist())


def constraint(seed, rhs=1.0):
    """add_constraint arguments for whatever shape the analyzer has: sens_cases.make_tech, 1..3 on
    the first third of the columns."""
    return lambda T: (sens_cases.make_tech(T.shape[1] - 1, seed), rhs)


def cap(col):
    """add_constraint arguments on an identity basis: x_col <= its value less 1, so the new row is
    row col + 1 with RHS -1 and the dual simplex pivots."""
    def args(T):
        tech = np.zeros(T.shape[1] - 1)
        tech[col] = 1.0
        return tech.tolist(), float(T[col + 1, -1]) - 1.0
    return args


def all_edit_cases(oracle):
    """[(name, base, [ops, ...])]: the five bases of sens_cases.scripts with every op of their
    lists alone and the full list in order, and that list up to each of its two constructed add
    edits (outcome 2 with the state left mid-way on four of the bases, outcome 1 on all) followed
    by change_rhs, change_basic and a second add.  The last two scripts are those."""
    out = []
    for name, base, ops in sens_cases.scripts(oracle):
        ops, basis = list(ops), base[3]
        after = [("change_rhs", (1, 2.0)), ("change_basic", (int(basis[0]), 0.5))]
        at2 = [op for op, _ in ops].index("add_constraint_infeasible") + 1
        at1 = [op for op, _ in ops].index("add_activity_unbounded") + 1
        tails = [ops[:at2] + after + [("add_activity", activity(51))],
                 ops[:at1] + after + [("add_constraint", constraint(52))]]
        out.append((name, base, [[e] for e in ops] + [list(ops)] + tails))
    return out


def mixed_shapes(oracle):
    """(base, [ops, ...]) on solved_lp(8, 12, 1): 0, 1, 2 and 3 growth edits, both orders of the
    two kinds, three of the RHS sweep's scripts and an empty one, interleaved."""
    base, sweep = sens_batch_cases.rhs_sweep(oracle)
    T = base[0]
    scripts = [
        [("add_activity", activity(61)), ("add_constraint", constraint(62))],
        sweep[3],
        [],
        [("add_constraint", constraint(63)), ("add_activity", activity(64)),
         ("change_rhs", (9, 0.5))],
        [("add_activity", activity(65, 9.0))],
        sweep[7],
        [("add_activity", activity(66)), ("change_rhs", (2, float(T[2, -1]) * 0.5)),
         ("add_constraint", constraint(67, 2.0)), ("add_activity", activity(68, 8.5))],
        [("add_constraint", constraint(69, 3.0))],
        sweep[21],
        [("change_basic", (int(base[3][0]), 0.5)), ("add_constraint", constraint(70)),
         ("add_constraint", constraint(71, 0.5))],
    ]
    return base, scripts


def stale_scripts(width, rows):
    """Scripts for sens_batch_cases.stale_base() after its prefix (basicVars[4] = -1): an
    add_constraint there is outcome 9 and the script goes on; an add_activity reads the row 0 the
    prefix's pivot left."""
    tech = sens_cases.make_tech(width, 81)
    return [
        [("add_constraint", (tech, 1.0))],
        [("add_constraint", (tech, 1.0)), ("change_nonbasic_cbar", (8, 0.75))],
        [("add_activity", activity(82))],
        [("add_activity", activity(83)), ("add_constraint", constraint(84)),
         ("change_rhs", (2, 1.0))],
    ]


def stale_solution_case():
    """(base, ops): identity_basis(6, 4) where change_nonbasic_cbar(7, -1.0) pivots column 7 in
    and then finds column 8 (all <= 0, its reduced cost driven negative by that pivot) unbounded:
    outcome 1 after a pivot, so the tableau has moved and solutionVector has not.  The
    add_constraint that follows has non-zero tech on the decision columns, and its aX reads that
    stale vector."""
    T, x, z, basis = sens_cases.identity_basis(6, 4, 35)
    T[1:, 7] = np.abs(T[1:, 7]) + 0.5
    T[1:, 8] = -8.0 * (np.abs(T[1:, 8]) + 0.5)
    T[0, 8] = 1.0
    ops = [("change_nonbasic_cbar", (7, -1.0)), ("add_constraint", constraint(85, 4.0)),
           ("resolve_all", ())]
    return (T, x, z, basis), ops


def rollback_growth_case():
    """(base, ops): rollback_base with an activity added first, so the snapshot change_rhs(3,
    -50.0) restores is the grown tableau; then a constraint, and a change_rhs that holds."""
    base, _ = sens_batch_cases.rollback_base(33)
    ops = [("add_activity", activity(86)), ("change_rhs", (3, -50.0)),
           ("add_constraint", constraint(87)), ("change_rhs", (3, 7.0))]
    return base, ops


def stride_cases():
    """[(name, base, ops, form)]: identity bases whose column or row count crosses a lane stride
    as the script grows them, each with a change_nonbasic_cbar that pivots afterwards.
      cols 255 -> 256 -> 257 on 101 rows (form H: 102 x 257 doubles are past G's LDS)
      cols 63 -> 65 on 21 rows (form G)
      rows 64 -> 65 (form G)"""
    def case(m, n_extra, seed, ops, col=1):
        return sens_cases.identity_basis(m, n_extra, seed), ops + [
            ("change_nonbasic_cbar", (m + col, -0.75)), ("resolve_all", ())]
    out = []
    base, ops = case(100, 54, 91, [("add_activity", activity(92)),
                                   ("add_constraint", cap(3))])
    out.append(("cols_255_257", base, ops, 2))
    base, ops = case(20, 22, 94, [("add_activity", activity(95)),
                                  ("add_constraint", cap(5))])
    out.append(("cols_63_65", base, ops, 1))
    base, ops = case(63, 4, 97, [("add_constraint", cap(40))], col=2)
    out.append(("rows_64_65", base, ops, 1))
    return out


def boundary_case(n_extra, seed=41):
    """identity_basis(60, n_extra) with one add_activity and work after it."""
    base = sens_cases.identity_basis(60, n_extra, seed)
    ops = [("add_activity", activity(99, 1.0)), ("change_nonbasic_cbar", (61, -0.75)),
           ("change_rhs", (30, -float(base[0][30, -1])))]
    return base, [ops, ops[:1], ops[1:]]
