"""The cases of test_condensed_gpu.py are not vacuous: on the oracle alone, the pivot logs of the
shapes it runs meet every class of event the condensed layout has to get right, and the integer
LPs tie the way their table says (condensed_cases.py)."""
import condensed_cases as cc
import ov_step_cases as cs


def test_step_shapes_meet_every_class(oracle):
    seen = {}
    for m, n, kind in cc.STEP_SHAPES:
        T0, b0, states = cs.reference(oracle, m, n, kind, (0,))
        seen[(m, n, kind)] = cc.classify(b0.tolist(), states[-1][2])
    for m, n in ((40, 60), (300, 700)):
        assert seen[(m, n, "optimal")] == set(cc.CLASSES), (m, n, seen[(m, n, "optimal")])
    everything = set().union(*seen.values())
    assert everything == set(cc.CLASSES)


def test_small_shapes_are_odd_and_leave_from_the_first_pivot(oracle):
    for m, n, seed in cc.SMALL:
        T0, b0 = cc.build(oracle, cc.small_case(m, n, seed))
        assert T0.shape == (m + 1, n + m + 1)
        T, b = T0.copy(), b0.copy()
        st, piv, log = oracle.primal_solve(T, b, 100000)
        assert st == 0 and piv >= 3
        assert "omitted-first" in cc.classify(b0.tolist(), log.tolist())
    assert any((n + 1) % 2 for _, n, _ in cc.SMALL) and any((n + 2) % 2 for _, n, _ in cc.SMALL)


def test_integer_cases_tie_in_a_spare_slot(oracle):
    for (m, n, seed), want in cc.INT_TIES.items():
        T0, b0 = cc.build(oracle, cc.int_lp(m, n, seed))
        assert sorted(b0.tolist()) == list(range(n, n + m))  # the slack columns
        assert want in cc.ties_of(oracle, T0, b0), (m, n, seed)
