"""GPU tests of the condensed working layout of the two-stream K-pivot path (condensed_cases.py:
what it is, how the cases are picked).  The layout is forced on small tableaux (opts.variant bit
26) and everything a solve leaves -- status, pivot count, pivot log, basis, every byte of the
tableau read back -- is compared with the oracle after every call.  LPR_TEST_OV_SPARES (read by
every solve call) fixes the number of spare columns: with 1 or 2 the driver expands and condenses
again every few pivots."""
import contextlib
import hashlib
import math
import os

import numpy as np
import pytest

import condensed_cases as cc
import ov_step_cases as cs
import special_values as sv

pytestmark = pytest.mark.gpu

COND = cc.OV2 | cc.FORCE
SPARES = (None, 1, 2)          # None: the driver's own number
SPARE_IDS = ["S-default", "S1", "S2"]


@contextlib.contextmanager
def spares(s):
    if s is None:
        yield
        return
    os.environ[cc.SPARES_HOOK] = str(s)
    try:
        yield
    finally:
        del os.environ[cc.SPARES_HOOK]


def run_legs(engine, ref, legs, variant, s, tag, exact_bytes=True):
    """`legs` (0 = no limit) on one handle; the state after each against the oracle's."""
    from lpr_381_group_v22_amd import Tableau
    T0, b0, states = ref
    tab = Tableau.from_array(engine, T0, b0)
    total = 0
    with spares(s):
        for leg, (st, piv, log, basis, tbytes) in zip(legs, states):
            res = tab.solve(max_pivots=leg, block=16, variant=variant)
            total += piv
            t = (tag, legs, leg, hex(variant), s)
            assert res.block == 16, t
            assert (res.status, res.pivots, res.total_pivots) == (st, piv, total), \
                (t, res.status, res.pivots, res.total_pivots, st, piv, total)
            assert tab.pivot_log(1 << 16).tolist()[total - piv:] == log, t
            assert tab.basis().tolist() == basis, t
            got = tab.read()
            if exact_bytes:
                assert got.tobytes() == tbytes, t
            else:  # NaN payloads are outside parity (special_values.same)
                sv.assert_same(got, np.frombuffer(tbytes).reshape(got.shape), t)
    tab.destroy()
    return states[-1][0]


def small_ref(oracle, m, n, seed, legs):
    T0, b0 = cc.build(oracle, cc.small_case(m, n, seed))
    return cc.legs_reference(oracle, ("small", m, n, seed), T0, b0, legs)


@pytest.mark.parametrize("s", SPARES, ids=SPARE_IDS)
def test_small_odd_shapes_vs_oracle(engine, oracle, s):
    """m, n from 3 to 40, odd widths (the physical width is padded to a column pair and beyond),
    more rows than columns and the reverse; whole solves."""
    for m, n, seed in cc.SMALL:
        assert run_legs(engine, small_ref(oracle, m, n, seed, (0,)), (0,), COND, s, (m, n)) == 0


@pytest.mark.parametrize("s", SPARES, ids=SPARE_IDS)
@pytest.mark.parametrize("m,n,kind", cc.STEP_SHAPES)
def test_step_shapes_vs_oracle(engine, oracle, m, n, kind, s):
    """Whole solves, optimal and unbounded exits, on the shapes of ov_step_cases: omitted variables
    leave in the first / last pivot of a block and in consecutive pivots, variables enter and leave
    again inside a block and across two, pivot rows repeat (test_condensed_cpu.py shows it)."""
    ref = cs.reference(oracle, m, n, kind, (0,))
    assert run_legs(engine, ref, (0,), COND, s, (m, n, kind)) == (0 if kind == "optimal" else 1)


@pytest.mark.parametrize("s", (None, 2), ids=["S-default", "S2"])
def test_pivot_limit_at_every_position_of_a_block(engine, oracle, s):
    """A first call of 1 .. 17 pivots, then the rest of the solve in a second call."""
    T0, b0, _ = cs.reference(oracle, 40, 60, "optimal", (0,))
    for k in range(1, 18):
        legs = (k, 0)
        ref = cc.legs_reference(oracle, ("limit", 40, 60), T0, b0, legs)
        assert run_legs(engine, ref, legs, COND, s, ("limit", k)) == 0


@pytest.mark.parametrize("s", (None, 1), ids=["S-default", "S1"])
def test_legs_on_one_handle(engine, oracle, s):
    """Limits inside blocks, four calls on one handle, then the rest."""
    for m, n in ((40, 60), (300, 700), (8, 3000)):
        T0, b0, _ = cs.reference(oracle, m, n, "optimal", (0,))
        legs = cs.LEGS + (0,)
        ref = cc.legs_reference(oracle, ("legs", m, n), T0, b0, legs)
        run_legs(engine, ref, legs, COND, s, ("legs", m, n))


@pytest.mark.parametrize("s", SPARES, ids=SPARE_IDS)
@pytest.mark.parametrize("m,n,seed", sorted(cc.INT_TIES))
def test_integer_ties_go_to_the_lower_original_index(engine, oracle, m, n, seed, s):
    """Equal reduced costs where a tied column sits in a spare slot (condensed_cases.ties_of)."""
    T0, b0 = cc.build(oracle, cc.int_lp(m, n, seed))
    ref = cc.legs_reference(oracle, ("ties", m, n, seed), T0, b0, (0,))
    run_legs(engine, ref, (0,), COND, s, ("ties", m, n, seed))


@pytest.mark.parametrize("value,own_row", [(-0.0, False), (2.0, True), (2.0, False)],
                         ids=["minus-zero", "two-on-the-diagonal", "two-elsewhere"])
def test_start_basis_that_is_not_exact_unit_columns(engine, oracle, value, own_row):
    """A basic column with -0.0 or 2.0 in it is not left out: the call runs on the full layout."""
    m, n, seed = 13, 37, 3
    T0, b0 = cc.build(oracle, cc.small_case(m, n, seed))
    T0 = T0.copy()
    row = 5
    T0[row if own_row else row + 2, b0[row - 1]] = value
    ref = cc.legs_reference(oracle, ("dirty", sv.bits(value), own_row), T0, b0, (0,))
    run_legs(engine, ref, (0,), COND, None, ("dirty", value, own_row))


@pytest.mark.parametrize("s", (None, 2), ids=["S-default", "S2"])
@pytest.mark.parametrize("value", sv.IN_BLOCK_VALUES, ids=["inf", "nan", "1e308"])
@pytest.mark.parametrize("m,n", ((300, 700), (8, 3000)))
def test_nonfinite_factor_after_omitted_variables_have_left(engine, oracle, m, n, value, s):
    """special_values.in_block_case: the value becomes a pivot-row / pivot-column entry inside a
    later block, when spare slots are in use; the call goes on in the full layout."""
    legs = (sv.IN_BLOCK_CAP,)
    T0, b0, states = sv.in_block_reference(oracle, m, n, value, legs)
    ref = (T0, b0, [(st, piv, log, basis, T.tobytes()) for st, piv, log, basis, T in states])
    run_legs(engine, ref, legs, COND, s, ("in-block", m, n, value), exact_bytes=False)


@pytest.mark.parametrize("value", (math.nan, math.inf), ids=["nan", "inf"])
def test_nonfinite_factor_in_the_first_pivot(engine, oracle, value):
    """The entering column of the first pivot holds the value: no omitted variable has left yet."""
    m, n = 40, 60
    T0, b0, _ = cs.reference(oracle, m, n, "optimal", (0,))
    T0 = T0.copy()
    T0[m // 2, sv.first_entering(T0)] = value
    legs = (64,)
    ref = cc.legs_reference(oracle, ("first", sv.bits(value)), T0, b0, legs)
    run_legs(engine, ref, legs, COND, None, ("first", value), exact_bytes=False)


def test_short_call_and_the_form_before(engine, oracle):
    """Without the force bit a call below the length threshold stays on the full layout; bit 25
    keeps a long one there.  Same results."""
    legs = (100, 0)
    T0, b0, _ = cs.reference(oracle, 300, 700, "optimal", (0,))
    ref = cc.legs_reference(oracle, ("short", 300, 700), T0, b0, legs)
    run_legs(engine, ref, legs, cc.OV2, None, "short")
    run_legs(engine, ref, legs, cc.OV2 | cc.BEFORE, None, "before")


def test_headline_shape_64_pivots(engine, oracle):
    """4097 x 12289, the default path with the layout forced (64 pivots are below the threshold)."""
    from lpr_381_group_v22_amd import Tableau
    T, basis = oracle.gen_dense_tableau(4096, 8192, 0)
    st, piv, log = oracle.primal_solve(T, basis, 64)
    tab = Tableau.synthetic(engine, 4096, 8192, 0)
    res = tab.solve(max_pivots=64, variant=cc.FORCE)
    assert (res.status, res.pivots, res.block) == (st, piv, 16)
    assert tab.pivot_log().tolist() == log.tolist()
    assert tab.basis().tolist() == basis.tolist()
    assert hashlib.sha256(tab.read().tobytes()).hexdigest() == hashlib.sha256(T.tobytes()).hexdigest()
    tab.destroy()
