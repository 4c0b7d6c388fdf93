"""CPU checks that keep the Branch & Bound edge instances of bb_cases honest (no GPU): each still
hits the edge it is named for on the oracle, and the rounding property two device-side skips rest
on (k_bb_finish reusing untouched rows, the pop skipping RoundAllTableaux :1047) holds."""
import struct

import numpy as np
import pytest

import bb_cases
from oracle_evaluator import OracleEvaluator


def bits(x):
    return struct.pack(">d", float(x)).hex()


def _dfs(oracle, c):
    return oracle.bb_solve(c["T"], c["nvars"], node_cap=c["cap"], rec_cap=1 << 12,
                           piv_cap=1 << 18)


@pytest.mark.parametrize("name", bb_cases.EDGE_CASE_NAMES)
def test_edge_case_builds_a_real_tree_within_its_depth(oracle, name):
    """At least min_children children solved at the DFS cap, and no expanded parent as deep as
    max_depth: the device never stops at its depth limit where the reference goes on."""
    c = bb_cases.edge_case(oracle, name)
    ref = _dfs(oracle, c)
    kids = sum(1 for r in ref["records"][1:] if r["status"] == 0)
    assert kids >= c["min_children"], (name, kids)
    assert max(r["depth"] for r in ref["records"]) <= c["max_depth"], name
    R, C = c["T"].shape
    assert 0 <= c["nvars"] <= C - 1
    assert R + c["max_depth"] <= bb_cases.ROWS_CAP_MAX
    assert bb_cases.align16(C + c["max_depth"]) <= bb_cases.ELIMINATE_LDS_COLS


@pytest.mark.parametrize("name", [n for n in bb_cases.EDGE_CASE_NAMES if n.startswith("flag_")])
def test_flag_case_hits_the_old_flag_room_edge(oracle, name):
    """rows_cap against the 8 (ld - 1 - nvars) bytes the -0.0 flags had in the score row: equal,
    one over, or far over, as the tag says.  (Before the flags got rows of their own, every
    child of an over case wrote rows_cap - room bytes past its node buffer.)"""
    c = bb_cases.edge_case(oracle, name)
    R, C = c["T"].shape
    rows_cap = R + c["max_depth"]
    room = bb_cases.legacy_flag_room(R, C, c["nvars"], c["max_depth"])
    if c["tag"] == "flag_exact":
        assert rows_cap == room
    elif c["tag"] == "flag_over_by_1":
        assert rows_cap == room + 1
    else:
        assert c["tag"] == "flag_over" and rows_cap >= room + 4


def test_flag_cases_cover_the_layout_residues(oracle):
    """Across the set: the ld padding, the touched map's rows_cap16, k_bb_finish's 64-lane grid
    and the multi-block score kernels each see their corner values."""
    cases = [bb_cases.edge_case(oracle, n) for n in bb_cases.EDGE_CASE_NAMES
             if n.startswith("flag_")]
    shapes = [(c["T"].shape[0], c["T"].shape[1], c["nvars"], c["max_depth"]) for c in cases]
    assert {0, 1, 15} <= {(C + md) % 16 for R, C, nv, md in shapes}
    assert {0, 1, 15} <= {(R + md) % 16 for R, C, nv, md in shapes}
    assert {0, 1, 63} <= {C % 64 for R, C, nv, md in shapes}
    assert any(nv > 256 for R, C, nv, md in shapes)
    assert {"flag_exact", "flag_over_by_1", "flag_over"} == {c["tag"] for c in cases}
    big_over = [bb_cases.legacy_flag_room(R, C, nv, md) - (R + md) for R, C, nv, md in shapes]
    assert min(big_over) <= -80  # the 40 x 300 program: 87 bytes past the old room


def test_tall_cases_are_tall(oracle):
    tall = [bb_cases.edge_case(oracle, n) for n in bb_cases.EDGE_CASE_NAMES
            if n.startswith("tall_")]
    assert all(c["T"].shape[0] > c["T"].shape[1] for c in tall)
    assert any(c["nvars"] == c["T"].shape[1] - 1 and c["T"].shape[1] > 2 for c in tall)
    assert any(c["T"].shape[1] == 2 for c in tall)
    assert any(c["nvars"] == 0 for c in tall)
    # and a tall one with pivots in its children, not only AddConstraint
    assert any(len(_dfs(oracle, c)["trace"]) >= 40 for c in tall)


def test_widest_case_sits_on_the_lds_limit(oracle):
    c = bb_cases.edge_case(oracle, "widest_lds")
    R, C = c["T"].shape
    assert bb_cases.align16(C + c["max_depth"]) == bb_cases.ELIMINATE_LDS_COLS
    assert bb_cases.align16(C + 1 + c["max_depth"]) > bb_cases.ELIMINATE_LDS_COLS
    assert np.all(c["T"][0, :-1] >= 0) and np.all(c["T"][1:, -1] >= 0)  # still a final tableau
    over = bb_cases.widest_lds_case(oracle, extra_cols=1)
    assert over["T"].shape[1] == C + 1


@pytest.mark.parametrize("M", bb_cases.BIG_M)
def test_big_value_case_expands_parents_that_hold_big_entries(oracle, M):
    """The oracle's own nodes: a parent other than the root that the search expands holds an entry
    with |v| >= 1e11 (slot.big on the device: k_bb_round at the pop, k_bb_node_info,
    dn_round4_thrice_clean in child init); M >= 1e16 leaves Math.Round's identity branch."""
    from lpr_381_group_v22_amd import solve_level_synchronous
    c = bb_cases.edge_case(oracle, f"big_m_{M:.1e}")
    assert np.max(np.abs(c["T"])) >= min(M, 1e16) * 0.5
    ev = OracleEvaluator(oracle, c["T"], c["nvars"])
    seen = {"big": 0, "parents": 0}
    inner = ev.expand

    def expand(parents, var, bound, kind):
        for p in set(int(x) for x in parents):
            if p != 0:
                seen["parents"] += 1
                if np.max(np.abs(ev.nodes[p])) >= 1e11:
                    seen["big"] += 1
        return inner(parents, var, bound, kind)

    ev.expand = expand
    solve_level_synchronous(ev, c["nvars"], max_levels=4)
    assert seen["big"] >= 3, seen
    ref = _dfs(oracle, c)
    assert ref["status"] == 0 and ref["processed"] >= 30


def _round4_operands():
    rng = np.random.RandomState(4)
    xs = []
    for e in range(-6, 11):  # every decade from 1e-6 to 1e11
        m = rng.uniform(1.0, 10.0, size=4000) * 10.0 ** e
        xs.append(m)
        xs.append(-m)
    k = rng.randint(-10 ** 9, 10 ** 9, size=20000).astype(np.float64)
    half = (k + 0.5) * 1e-4  # exact decimal half-way values (as doubles: next to them)
    xs += [half, np.round(half, 4)]
    for c in (1e11, 2.2e11, 2.0 ** 53 / 1e4):
        near = [c]
        v = c
        for _ in range(300):
            v = np.nextafter(v, 0.0)
            near.append(v)
        v = c
        for _ in range(300):
            v = np.nextafter(v, np.inf)
            near.append(v)
        near = np.array(near)
        xs += [near, -near, c * (1 + rng.uniform(-1e-4, 1e-4, size=2000))]
    return np.concatenate(xs)


def test_round4_is_idempotent_bit_for_bit(oracle):
    """round4(round4(x)) == round4(x), bits included, over every decade from 1e-6 up to 1e11,
    both signs, decimal half-way values and the neighbourhoods of 1e11, 2.2e11 and 2^53 / 1e4."""
    xs = _round4_operands()
    assert len(xs) > 150000
    bad = []
    for x in xs.tolist():
        r = oracle.round4(x)
        if bits(oracle.round4(r)) != bits(r):
            bad.append(x)
    assert not bad, bad[:5]
    assert bits(oracle.round4(-0.00001)) == bits(-0.0)  # the -0.0 the flags are about
