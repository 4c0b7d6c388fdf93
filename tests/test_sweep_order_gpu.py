"""GPU parity tests of the two-stream sweep's tile order and cache policy (csrc/overlap_kernels.hip,
ov_tiles): every sweep that applies pivots walks the tableau the other way round from the one
before -- across solve calls too -- and the tiles at both ends of its work queue keep the default
cache policy (kOvIcMB), the rest is non-temporal.  ALLNT (opts.variant bit 23) is the form before:
every tile non-temporal.  Neither may change a bit: status, pivot log, basis and every byte of the
tableau against the oracle, for an odd and an even number of sweeps, pivot limits that cut a block
in either direction, and legs of one solve spread over several calls."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu

OV2 = 0x3008
ALLNT = 0x800000
# 3073 x 9217 (227 MB): 1 843 tiles of 32 rows, more than the 2 x 512 tiles of the two 64 MB queue
# ends, so every sweep has non-temporal tiles between the default-policy ones
M, N, SEED = 3072, 6144, 7
_REF = {}


def _oracle_after(oracle, pivots):
    if pivots not in _REF:
        T, basis = oracle.gen_dense_tableau(M, N, SEED)
        st, piv, log = oracle.primal_solve(T, basis, pivots)
        _REF[pivots] = (st, piv, log, basis, hashlib.sha256(T.tobytes()).hexdigest())
    return _REF[pivots]


def _check(tab, ref, total):
    st, piv, log, basis, sha = ref
    assert total == piv
    assert tab.pivot_log().tolist() == log.tolist()
    assert tab.basis().tolist() == basis.tolist()
    assert hashlib.sha256(tab.read().tobytes()).hexdigest() == sha


@pytest.mark.parametrize("variant", [0, ALLNT, OV2, OV2 | ALLNT],
                         ids=["default", "allnt", "ov2", "ov2-allnt"])
@pytest.mark.parametrize("pivots", [80, 96, 55, 39])
def test_alternating_order_vs_oracle(engine, oracle, variant, pivots):
    """One call: 80 / 96 pivots are 5 / 6 full sweeps (an odd and an even number of direction
    flips); 55 and 39 end in a partial block, swept forwards and backwards respectively."""
    from lpr_381_group_v22_amd import Tableau
    ref = _oracle_after(oracle, pivots)
    tab = Tableau.synthetic(engine, M, N, SEED)
    res = tab.solve(max_pivots=pivots, variant=variant)
    assert res.status == ref[0] and res.block == 16
    _check(tab, ref, res.pivots)
    tab.destroy()


@pytest.mark.parametrize("variant", [0, ALLNT], ids=["default", "allnt"])
def test_direction_carried_across_calls_vs_oracle(engine, oracle, variant):
    """Legs of 16, 23, 9, 32 and 17 pivots: the direction of the first sweep of a call follows the
    last sweep of the call before (partial blocks included), not the call count."""
    from lpr_381_group_v22_amd import Tableau
    legs = (16, 23, 9, 32, 17)
    ref = _oracle_after(oracle, sum(legs))
    tab = Tableau.synthetic(engine, M, N, SEED)
    total = 0
    for leg in legs:
        res = tab.solve(max_pivots=leg, variant=variant)
        assert res.pivots == leg and res.status == 5
        total += res.pivots
    assert res.status == ref[0]
    _check(tab, ref, total)
    tab.destroy()


def test_north_star_size_64_pivots_all_nontemporal_vs_oracle(engine, oracle):
    """The headline size (4097 x 12289, 402.8 MB) on the default path with every tile non-temporal
    (the form before the queue ends kept the default policy): the oracle's 64-pivot result."""
    from lpr_381_group_v22_amd import Tableau
    T, basis = oracle.gen_dense_tableau(4096, 8192, 0)
    st, piv, log = oracle.primal_solve(T, basis, 64)
    assert st == 5 and piv == 64
    sha = hashlib.sha256(T.tobytes()).hexdigest()
    del T
    tab = Tableau.synthetic(engine, 4096, 8192, 0)
    res = tab.solve(max_pivots=64, variant=ALLNT)
    assert res.status == st and res.pivots == 64 and res.block == 16
    assert tab.pivot_log().tolist() == log.tolist()
    assert tab.basis().tolist() == basis.tolist()
    assert hashlib.sha256(tab.read().tobytes()).hexdigest() == sha
    tab.destroy()
