"""GPU parity tests of the loop heads' RHS entry of the pivot row (csrc/overlap_kernels.hip,
ov_heads phase B): T^(q-1)[r, rhs] is no longer taken through the two blocks' pivots by a chain of
its own; one lane loads it from bvec, where the head before (or the launch / the prologue before)
left it.  That must not change a bit -- when r was a pivot row of the block being swept or of this
block (bvec then holds p_t[rhs]), in the first head of a launch and of a solve call, for rows no
lane holds in a register (R > G x 256), and for either parity of the pivot index.  Status, pivot
count, pivot log, basis and every byte of the tableau against the oracle after every leg; both
K-pivot forms share the heads, so the in-place form runs the same cases."""
import pytest

import ov_step_cases as cs

pytestmark = pytest.mark.gpu

SEQ = 0x4008
VARIANTS = [cs.OV2, SEQ]
IDS = ["ov2", "seq"]
SHAPE_IDS = ["%dx%d" % s for s in cs.SHAPES]


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("m,n", list(cs.SHAPES), ids=SHAPE_IDS)
def test_one_call_and_ragged_legs_vs_oracle(engine, oracle, m, n, variant):
    """55 pivots in one call (three full blocks and a partial one), then the same LP in legs of
    16, 23, 9 and 17: every call starts from the bvec bank of its first pivot's parity (16 + 23
    leaves an odd count) and limits fall inside a block."""
    for legs in (cs.ONE_CALL, cs.LEGS):
        cs.run_and_check(engine, oracle, m, n, "optimal", legs, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("m,n", list(cs.SHAPES), ids=SHAPE_IDS)
def test_full_solves_end_optimal_and_unbounded(engine, oracle, m, n, variant):
    assert cs.run_and_check(engine, oracle, m, n, "optimal", (0,), variant) == 0
    assert cs.run_and_check(engine, oracle, m, n, "unbounded", (0,), variant) == 1


@pytest.mark.parametrize("variant,block", [(cs.OV2, 16), (cs.OV2, 5), (SEQ, 16)],
                         ids=["ov2", "ov2-block5", "seq"])
def test_pivot_row_repeats_in_two_consecutive_blocks(engine, oracle, variant, block):
    """m=8, n=3000: 33 pivots over 8 rows with six head workgroups.  The oracle's log must show
    rows that were a pivot row of the block before AND rows that were one earlier in their own
    block (for block = 16; smaller blocks repeat all the more) -- the two cases in which the RHS
    entry the head needs is a p_t[rhs] that replaced the row's own."""
    _, _, states = cs.reference(oracle, 8, 3000, "optimal", (0,))
    rep_a, rep_n = cs.row_repeats(states[-1][2])
    assert rep_a >= 4 and rep_n >= 4, (rep_a, rep_n)
    assert cs.run_and_check(engine, oracle, 8, 3000, "optimal", (0,), variant, block) == 0
    cs.run_and_check(engine, oracle, 8, 3000, "optimal", (7, 16, 0), variant, block)
