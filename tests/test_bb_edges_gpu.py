"""GPU parity tests of the Branch & Bound path at the shapes and magnitudes the product fixtures
never reach (bb_cases.edge_cases): -0.0 flag bytes at and past their old room in the score row,
tall tableaux, nvars = 0 and nvars > 256, the widest tableau k_bb_eliminate ranks in LDS, big-M rows
(slot.big) -- against the CPU oracle, node by node and bit for bit -- and the create-time limits."""
import struct

import numpy as np
import pytest

import bb_cases
from oracle_evaluator import OracleEvaluator

pytestmark = pytest.mark.gpu


def bits(x):
    return struct.pack(">d", float(x)).hex()


@pytest.mark.parametrize("name", bb_cases.EDGE_CASE_NAMES)
def test_edge_dfs_run_matches_oracle(engine, oracle, name):
    from lpr_381_group_v22_amd import BranchBoundTree
    c = bb_cases.edge_case(oracle, name)
    T, n, cap = c["T"], c["nvars"], c["cap"]
    ref = oracle.bb_solve(T, n, node_cap=cap, rec_cap=1 << 12, piv_cap=1 << 18)
    tree = BranchBoundTree.from_array(engine, T, n, max_depth=c["max_depth"])
    res, x = tree.run(node_cap=cap)
    records, pop, trace = tree.records(), tree.pop_order(), tree.trace()
    tree.destroy()
    assert res.status == ref["status"]
    assert res.processed == ref["processed"]
    assert pop == ref["pop_order"]
    assert records == ref["records"]
    assert trace == ref["trace"]
    assert bool(res.found) == ref["found"] and bits(res.z) == bits(ref["z"])
    if ref["found"]:
        assert [bits(v) for v in x] == [bits(v) for v in ref["x"]]
        assert res.best_node == ref["best_node"]


@pytest.mark.parametrize("name", bb_cases.EDGE_CASE_NAMES)
def test_edge_level_sync_matches_oracle_evaluator(engine, oracle, name):
    """lpr_bb_solve_level_sync (every child of a level in one batch: in-place second children,
    shared parent scans) against the Python mirror over the oracle, for a few levels."""
    from lpr_381_group_v22_amd import (BranchBoundTree, solve_level_sync_native,
                                       solve_level_synchronous)
    c = bb_cases.edge_case(oracle, name)
    T, n = c["T"], c["nvars"]
    levels = min(4, c["max_depth"])
    tree = BranchBoundTree.from_array(engine, T, n, max_depth=c["max_depth"])
    got = solve_level_sync_native(tree, max_levels=levels)
    tree.destroy()
    want = solve_level_synchronous(OracleEvaluator(oracle, T, n), n, max_levels=levels)
    for key in ("processed", "pivots", "levels", "found", "status"):
        assert got[key] == want[key], key
    if want["found"]:
        assert bits(got["z"]) == bits(want["z"]) and got["path"] == tuple(want["path"])
        assert [bits(v) for v in got["x"]] == [bits(v) for v in want["x"]]


def _create_error(engine, T, nvars, max_depth):
    from lpr_381_group_v22_amd import BranchBoundTree
    from lpr_381_group_v22_amd import _native as N
    with pytest.raises(N.EngineError) as exc:
        BranchBoundTree.from_array(engine, T, nvars, max_depth=max_depth)
    assert exc.value.status == N.LPR_BAD_ARGUMENT
    return str(exc.value)


def test_one_column_past_the_lds_limit_is_refused(engine, oracle):
    over = bb_cases.widest_lds_case(oracle, extra_cols=1)
    msg = _create_error(engine, over["T"], over["nvars"], over["max_depth"])
    assert "36864" in msg and "LDS" in msg, msg


def test_rows_plus_depth_limit(engine, oracle):
    """rows + max_depth = 65 535 is taken (root scored like the oracle), 65 536 is refused."""
    from lpr_381_group_v22_amd import BranchBoundTree
    md = 8
    rng = np.random.RandomState(65535)
    T = np.zeros((bb_cases.ROWS_CAP_MAX - md, 2))
    T[:, 0] = np.round(rng.uniform(-1, 2, size=T.shape[0]), 2)
    T[:, 1] = np.round(rng.uniform(0, 5, size=T.shape[0]), 3)
    T[0, 0] = 0.25
    T[T.shape[0] // 2, 0] = 1.0
    tree = BranchBoundTree.from_array(engine, T, 1, max_depth=md)
    z, vals = tree.node_info([0])
    root = tree.node_read(0)
    tree.destroy()
    want_T, want_z, want_v = oracle.bb_node_info(T, 1)
    assert bits(z[0]) == bits(want_z) and [bits(v) for v in vals[0]] == [bits(v) for v in want_v]
    assert root.tobytes() == want_T.tobytes()
    msg = _create_error(engine, T, 1, md + 1)
    assert "65535" in msg, msg
    msg = _create_error(engine, np.vstack([T, T[-1:]]), 1, md)
    assert "65535" in msg, msg


def test_depth_limit_then_a_new_tree_on_the_same_engine(engine, oracle):
    """A tree whose DFS reaches max_depth stops with a non-OK status and can be destroyed; a new
    tree on the same engine (recycled device state) then matches the oracle node for node."""
    from lpr_381_group_v22_amd import BranchBoundTree
    from lpr_381_group_v22_amd import _native as N
    c = bb_cases.edge_case(oracle, "flag_over_bin40x300s1_nv380_md26")
    T, n, cap = c["T"], c["nvars"], c["cap"]
    ref = oracle.bb_solve(T, n, node_cap=cap, rec_cap=1 << 12, piv_cap=1 << 18)
    assert max(r["depth"] for r in ref["records"]) > 4
    short = BranchBoundTree.from_array(engine, T, n, max_depth=4)
    res, _ = short.run(node_cap=cap)
    assert res.status == N.LPR_BB_NODE_CAP
    assert res.processed < ref["processed"]
    assert all(r["depth"] <= 4 for r in short.records())
    short.destroy()
    tree = BranchBoundTree.from_array(engine, T, n, max_depth=c["max_depth"])
    res, x = tree.run(node_cap=cap)
    assert res.status == ref["status"] and res.processed == ref["processed"]
    assert tree.pop_order() == ref["pop_order"] and tree.records() == ref["records"]
    assert tree.trace() == ref["trace"]
    assert bits(res.z) == bits(ref["z"])
    tree.destroy()
