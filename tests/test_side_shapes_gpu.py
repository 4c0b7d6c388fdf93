"""GPU parity of the side paths at the shapes where their single-workgroup folds change
behaviour: tableaux grown by cuts across the primal paths (a handle's lazily built contexts must
follow its shape), cut-path and sensitivity selections whose deciding candidates sit one or more
1024-lane strides apart, the uncached and overflow regimes of eps_fold, and repeated growth of a
sensitivity analyzer past 1024 rows.  Every leg is checked against the C oracle bit for bit."""
import numpy as np
import pytest

import cut_cases
import sens_cases

pytestmark = pytest.mark.gpu

DUAL_STATUS = {0: 0, 1: 2, 3: 3, 5: 5}    # oracle rc -> lpr_status (as test_cut_gpu.py)
PRIM_STATUS = {0: 0, 1: 1, 3: 3, 5: 5}

SMALL_MAX_R, SMALL_MAX_LD, SMALL_LDS = 1024, 2048, 140 << 10   # small_kernels.hip: small_fits


def align_up(x, a):
    return (x + a - 1) // a * a


def small_fits(rows, ld):
    return 2 <= rows <= SMALL_MAX_R and ld <= SMALL_MAX_LD and 16 * align_up(rows, 16) * 8 <= SMALL_LDS


# ---- growth by cuts across the primal paths -----------------------------------------------------
# (m, n, cuts): R0 = m + 1 = 16 (the first cut already passes Rp = 16), 41, 1010 (the cuts push R
# past 1024, so the default path leaves the small path in the middle of the handle's life).
GROWTH = [(15, 400, 12), (40, 56, 12), (1009, 300, 16)]
VARIANTS = [dict(variant=0), dict(variant=0x2000), dict(variant=0x4008, block=4),
            dict(variant=0x7fff, batch=4)]
RESOLVE_CAP = 400
_legs = {}


def _oracle_legs(oracle, m, n, cuts):
    """The oracle's legs of one growth case (cached: every variant replays the same script)."""
    key = (m, n, cuts)
    if key not in _legs:
        T0, basis = oracle.gen_dense_tableau(m, n, 7)
        T1 = T0.copy()
        b1 = basis.copy()
        solved = oracle.primal_solve(T1, b1)
        rc, ncuts, T2, clog = oracle.cutting_plane(T1, max_cuts=cuts, hard_cap=300)
        # the disturbing pivot: among the largest positive reduced costs, the first column whose
        # smallest positive entry as pivot leaves a re-solve of >= 16 pivots
        r = j = None
        for jj in np.argsort(-T2[0, :-1], kind="stable")[:40]:
            col = T2[1:, jj]
            pos = np.nonzero(col > 1e-6)[0]
            if T2[0, jj] <= 0 or len(pos) == 0:
                continue
            rr = int(pos[np.argmin(col[pos])]) + 1
            T3 = T2.copy()
            oracle.pivot(T3, rr, int(jj))
            if oracle.primal_solve(T3.copy(), None, RESOLVE_CAP)[1] >= 16:
                r, j = rr, int(jj)
                break
        assert r is not None, key
        T3 = T2.copy()
        oracle.pivot(T3, r, j)
        pivoted = T3.copy()
        resolved = oracle.primal_solve(T3, None, RESOLVE_CAP)
        _legs[key] = dict(T0=T0, basis=basis, solved=solved, T1=T1, cut=(rc, ncuts, T2, clog),
                          pivot=(r, j), pivoted=pivoted, resolved=resolved, T3=T3)
    return _legs[key]


@pytest.mark.parametrize("opts", VARIANTS, ids=["default", "small", "kpivot", "graph"])
@pytest.mark.parametrize("m,n,cuts", GROWTH, ids=["R16", "R41", "R1010"])
def test_growth_by_cuts_then_primal_paths(engine, oracle, m, n, cuts, opts):
    from lpr_381_group_v22_amd import Tableau
    L = _oracle_legs(oracle, m, n, cuts)
    R0 = m + 1
    tab = Tableau.from_array(engine, L["T0"], L["basis"])
    assert small_fits(tab.rows, tab.ld), (tab.rows, tab.ld)     # leg 1 runs on the small path
    # 1. primal solve on the default path (variant 0: the cache-resident small path)
    st, piv, log = L["solved"]
    res = tab.solve()
    assert (res.status, res.pivots) == (st, piv)
    assert res.block == 16                                       # the small path's block
    assert np.array_equal(tab.pivot_log(), log)
    assert tab.read().tobytes() == L["T1"].tobytes()
    # 2. cuts: R crosses align_up(R0, 16); > 9 cuts re-allocate the buffer twice
    rc, ncuts, T2, clog = L["cut"]
    ex, got_cuts = tab.cutting_plane(max_cuts=cuts, hard_cap=300)
    assert (ex, got_cuts) == (rc, ncuts) == (6, cuts)
    assert tab.cut_log() == clog
    assert tab.rows == R0 + cuts > align_up(R0, 16)
    got = tab.read()
    assert got.shape == T2.shape and got.tobytes() == T2.tobytes()
    # 3. one pivot on a column with a positive reduced cost: the tableau is no longer optimal
    r, j = L["pivot"]
    assert T2[0, j] > 0
    tab.pivot(r, j)
    assert tab.read().tobytes() == L["pivoted"].tobytes()
    # 4. primal solve on the grown tableau through the path under test
    if opts["variant"] == 0x2000 and not small_fits(tab.rows, tab.ld):
        opts = dict(variant=0)      # forcing the small path needs a tableau it fits
    st, piv, log = L["resolved"]
    assert piv >= 16                # at least one full small-path block on the grown rows
    res = tab.solve(max_pivots=RESOLVE_CAP, **opts)
    assert (res.status, res.pivots) == (st, piv), opts
    assert np.array_equal(tab.pivot_log()[-piv:], log), opts
    assert tab.read().tobytes() == L["T3"].tobytes(), opts
    tab.destroy()


def test_growth_cases_cover_their_preconditions():
    assert any(cuts > 9 for _, _, cuts in GROWTH)                     # two re-allocations
    assert any(m + 1 <= 1024 < m + 1 + cuts for m, _, cuts in GROWTH)  # crosses R = 1024
    assert all(m + 1 + cuts > align_up(m + 1, 16) for m, _, cuts in GROWTH)


# ---- cut path past one workgroup stride ---------------------------------------------------------

def _side_call(tab, solver, hard_cap, max_cuts=1):
    if solver == "dual":
        return tab.dual_solve(print_steps=True, hard_cap=hard_cap)
    if solver == "primal2":
        return tab.primal2_solve(print_steps=False, hard_cap=hard_cap)
    return tab.cutting_plane(max_cuts=max_cuts, hard_cap=hard_cap)


def test_cut_path_ties_across_strides(engine, oracle):
    from lpr_381_group_v22_amd import Tableau
    for name, solver, T0, field, planted in cut_cases.stride_cases():
        rc, k, T, log = cut_cases.run_oracle(oracle, solver, T0, hard_cap=200)
        assert log[0][field] == planted, name
        tab = Tableau.from_array(engine, T0)
        res = _side_call(tab, solver, 200)
        if solver == "cut":
            assert res == (rc, k), name
        else:
            status = (DUAL_STATUS if solver == "dual" else PRIM_STATUS)[rc]
            assert (res.status, res.pivots) == (status, k), name
        assert tab.cut_log() == log, name
        got = tab.read()
        assert got.shape == T.shape and got.tobytes() == T.tobytes(), name
        tab.destroy()


def test_many_cuts_on_a_tall_tableau(engine, oracle):
    from lpr_381_group_v22_amd import Tableau
    T0 = cut_cases.many_cuts_tall()
    assert T0.shape[0] - 1 > 1024
    rc, cuts, T, log = oracle.cutting_plane(T0, max_cuts=12, hard_cap=300)
    assert (rc, cuts) == (6, 12)
    tab = Tableau.from_array(engine, T0)
    assert tab.cutting_plane(max_cuts=12, hard_cap=300) == (rc, cuts)
    assert tab.cut_log() == log
    got = tab.read()
    assert got.shape == T.shape and got.tobytes() == T.tobytes()
    tab.destroy()


# ---- sensitivity re-solve past one workgroup stride ---------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in sens_cases.stride_scripts()])
def test_sens_scripts_across_strides(engine, oracle, name):
    _, base, ops, _ = next(s for s in sens_cases.stride_scripts() if s[0] == name)
    codes = sens_cases.run_script(engine, oracle, name, base, ops)
    assert codes == [0] * len(ops)


def test_sens_basic_row_and_column_fold_wide(engine):
    """k_sens_basic_row and column_fold with more than 1024 columns and more than 64 rows."""
    from lpr_381_group_v22_amd.engine import SensState
    T, x, z, _ = sens_cases.identity_basis(80, 1200, 27)
    R, C = T.shape
    d = SensState.create(engine, T, x, z)
    for col in (0, 5, 79, 80, 1100, C - 2):
        assert d.basic_row(col) == (col + 1 if col < 80 else -1), col
    rng = np.random.RandomState(4)
    w = rng.uniform(-1, 1, size=R - 1)
    init = rng.uniform(-1, 1, size=C - 1)
    got = d.column_fold(w, init, C - 1)
    exp = init.copy()
    for i in range(R - 1):          # same order, every product rounded on its own
        exp = exp + w[i] * T[i + 1, :C - 1]
    assert got.tobytes() == exp.tobytes()
    d.destroy()
