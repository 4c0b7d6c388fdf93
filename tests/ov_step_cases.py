"""Small LPs and leg patterns shared by test_tall_tiles_gpu.py and test_heads_rhs_gpu.py (TEST
ONLY): the smallest shapes at which the two-stream K-pivot path (csrc/overlap_kernels.hip) takes
each of its side paths, every leg compared with the oracle the way test_block_gpu.py does."""
from __future__ import annotations

import lp_cases

OV2 = 0x3008        # the two-stream overlap forced on a small tableau
FLATQ = 0x1000000   # opts.variant bit 24: the sweep's queue without 64-row tiles (the form before)

# (m, n): what the shape exercises
SHAPES = {
    (300, 700): "R=301: nine full row-tiles + a ragged tenth of 13 rows (it pairs on odd sweeps), "
                "two column strips, the last ragged; two head workgroups",
    (270, 700): "R=271: nine row-tiles, an odd count: one cannot pair",
    (40, 60): "fewer rows than one tall tile; one column strip, one head workgroup",
    (600, 50): "R=601 > 512 rows per head trip: the heads' further-rows path",
    (8, 3000): "six head workgroups, few rows: pivot rows repeat inside two consecutive blocks",
}
ONE_CALL = (55,)             # three full blocks and a partial one, sweeps in both directions
LEGS = (16, 23, 9, 17)       # the direction is carried across calls, limits fall inside a block


def _negated(case, unbounded_column):
    """Constraint rows negated as in test_block_gpu.py's fuzz; unbounded_column: one column (the
    middle one) also gets no positive entry at all, so the solve ends unbounded once it enters."""
    obj, cons, is_max = case
    j0 = len(obj) // 2 if unbounded_column else -1
    cons = [type(c)([-abs(v) if j == j0 else (-v if (k + j) % 3 == 0 else v)
                     for j, v in enumerate(c.Coefficients)], c.Relation, c.RHS)
            for k, c in enumerate(cons)]
    return obj, cons, is_max


def case(m, n, kind):
    """kind "optimal" / "unbounded": how the full solve ends (seeds picked on the CPU oracle; the
    tests assert the status).  Pivots of the full solves: 121 / 1130, 121 / 945, 50 / 43, 78 / 131,
    33 / 7."""
    if (m, n) == (8, 3000):
        # plain rows: 33 pivots over 8 rows, so rows repeat within a block and the block before
        return lp_cases.random_dense(m, n, 5) if kind == "optimal" else \
            _negated(lp_cases.random_dense(m, n, 0), True)
    seed = 1 if (m, n) in ((40, 60), (600, 50)) else 0
    return _negated(lp_cases.random_dense(m, n, seed), kind == "unbounded")


_REF = {}


def reference(oracle, m, n, kind, legs):
    """[(status, pivots, log, basis, tableau bytes)] after each leg (0 = no pivot limit), computed
    once per (shape, kind, legs) and shared by every variant."""
    key = (m, n, kind, legs)
    if key not in _REF:
        obj, cons, is_max = case(m, n, kind)
        o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
        T, basis = oracle.primal_build(o, A, rel, rhs, is_max, ncoef)
        T0, b0 = T.copy(), basis.copy()
        states = []
        for leg in legs:
            st, piv, log = oracle.primal_solve(T, basis, leg if leg else 100000)
            states.append((st, piv, log.tolist(), basis.tolist(), T.tobytes()))
            if st != 5:
                break
        _REF[key] = (T0, b0, states)
    return _REF[key]


def run_and_check(engine, oracle, m, n, kind, legs, variant, block=16):
    """The legs on the device against the oracle's state after each; returns the final status."""
    from lpr_381_group_v22_amd import Tableau
    T0, b0, states = reference(oracle, m, n, kind, legs)
    tab = Tableau.from_array(engine, T0, b0)
    total = 0
    for leg, (st, piv, log, basis, tbytes) in zip(legs, states):
        res = tab.solve(max_pivots=leg if leg else 100000, block=block, variant=variant)
        total += piv
        tag = (m, n, kind, leg, hex(variant))
        assert res.block == block, tag
        assert res.status == st and res.pivots == piv and res.total_pivots == total, \
            (tag, res.status, st, res.pivots, piv)
        assert tab.pivot_log(1 << 16).tolist()[total - piv:] == log, tag
        assert tab.basis().tolist() == basis, tag
        assert tab.read().tobytes() == tbytes, tag
    tab.destroy()
    return states[-1][0]


def row_repeats(log):
    """(pivots whose row was a pivot row of the block of 16 before, ... of an earlier pivot of
    their own block) in a pivot log [(row, col)]."""
    rows = [r for r, _ in log]
    rep_a = rep_n = 0
    for q, r in enumerate(rows):
        b = q // 16
        rep_n += r in rows[b * 16:q]
        rep_a += b > 0 and r in rows[(b - 1) * 16:b * 16]
    return rep_a, rep_n
