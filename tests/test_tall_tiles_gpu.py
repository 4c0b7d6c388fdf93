"""GPU parity tests of the two-stream sweep's work queue (csrc/overlap_kernels.hip, ov_tiles):
64-row tiles at the head of the queue (a lane's pivot-row slices are loaded once for both 32-row
halves), 32-row tiles after them, 16-row half tiles at the tail.  FLATQ (opts.variant bit 24) is
the queue before: no 64-row tiles.  Only which workgroup computes which rows changes, so neither
may change a bit: status, pivot count, pivot log, basis and every byte of the tableau against the
oracle after every leg -- with the ragged last row-tile inside a pair (on sweeps that walk the
queue backwards), an odd number of row-tiles, fewer rows than one tall tile, a ragged last column
strip, pivot rows of the block in either half of a tall tile, partial blocks, and the sweep
direction carried from call to call."""
import pytest

import ov_step_cases as cs

pytestmark = pytest.mark.gpu

VARIANTS = [cs.OV2, cs.OV2 | cs.FLATQ]
IDS = ["tall", "flatq"]
SHAPE_IDS = ["%dx%d" % s for s in cs.SHAPES]


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("m,n", list(cs.SHAPES), ids=SHAPE_IDS)
def test_one_call_and_ragged_legs_vs_oracle(engine, oracle, m, n, variant):
    """55 pivots in one call: three full blocks and a partial one, sweeps in both directions; then
    legs of 16, 23, 9 and 17: the direction is carried across calls, limits fall inside a block."""
    for legs in (cs.ONE_CALL, cs.LEGS):
        cs.run_and_check(engine, oracle, m, n, "optimal", legs, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("m,n", list(cs.SHAPES), ids=SHAPE_IDS)
def test_full_solves_end_optimal_and_unbounded(engine, oracle, m, n, variant):
    assert cs.run_and_check(engine, oracle, m, n, "optimal", (0,), variant) == 0
    assert cs.run_and_check(engine, oracle, m, n, "unbounded", (0,), variant) == 1


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_pivot_rows_in_both_halves_of_a_tall_tile(engine, oracle, variant):
    """m=300: the first tall tiles cover rows 0..63 on forward sweeps (the 1st, 3rd, ... of a call).
    The oracle's log must hold such a full block with pivot rows in rows 1..31 and in rows 32..63,
    so that one tall tile recomputes pivot rows in both of its halves."""
    _, _, states = cs.reference(oracle, 300, 700, "optimal", (0,))
    rows = [r for r, _ in states[-1][2]]
    fwd = [rows[k:k + 16] for k in range(0, len(rows) - 15, 32)]
    assert any(any(r < 32 for r in b) and any(32 <= r < 64 for r in b) for b in fwd)
    cs.run_and_check(engine, oracle, 300, 700, "optimal", (0,), variant)
