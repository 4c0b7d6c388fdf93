#!/usr/bin/env python3
"""Time-bounded randomised comparison of the Branch & Bound path on the device with the C oracle:
node records, pop order, every dual / primal pivot of every child (incl. dropped last tableaux),
incumbent bits -- lpr_bb_run (the reference's DFS) and, on the same instance, the level-synchronous
driver against the oracle-backed evaluator:  python tools/fuzz_bb_gpu.py [seconds] [first seed]
Every third seed (seed % 3 == 0) draws from the edge space instead: up to 160 constraints, nvars
anywhere from n up to cols - 1, max_depth near the point where rows_cap meets the old -0.0 flag
room of the score row (bb_cases.legacy_flag_room), and in half of them a big-M row."""
import struct
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import bb_cases  # noqa: E402
from oracle_evaluator import OracleEvaluator  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
import lpr_381_group_v22_amd as pkg  # noqa: E402
from lpr_381_group_v22_amd import BranchBoundTree, solve_level_sync_native, solve_level_synchronous  # noqa: E402


def bits(x):
    return struct.pack(">d", float(x)).hex()


budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
oracle = Oracle()
eng = pkg.Engine(0)
t_end = time.time() + budget
cases = drops = primal = 0
edge_cases = 0


def edge_draw(seed):
    """(obj, cons, n, nvars, max_depth, cap) of an edge seed."""
    rng = np.random.RandomState([seed, 1])
    n, mc = int(rng.randint(3, 14)), int(rng.randint(1, 161))
    big_m = float(rng.choice(bb_cases.BIG_M)) if rng.randint(0, 2) else 0.0
    if big_m and n >= 2:
        obj, cons = bb_cases.fractional_program(n, mc, int(rng.randint(0, 1 << 30)), big_m=big_m)
    else:
        gen = bb_cases.random_binary_program if rng.randint(0, 2) else bb_cases.fractional_program
        obj, cons = gen(n, mc, int(rng.randint(0, 1 << 30)))
    rows, cols = 1 + len(cons), len(obj) + len(cons) + 1  # product route: one slack per row
    nv = int(rng.randint(n, cols))
    gap = [(abs(rows + md - bb_cases.legacy_flag_room(rows, cols, nv, md)), md) for md in range(2, 41)]
    near = [md for g, md in gap if g <= 8] or [min(gap)[1]]
    md = int(rng.choice(near))
    return obj, cons, n, nv, md, min(20, md)


while time.time() < t_end:
    rng = np.random.RandomState(seed)
    n, mc = int(rng.randint(3, 14)), int(rng.randint(1, 6))
    gen = bb_cases.random_binary_program if rng.randint(0, 2) else bb_cases.fractional_program
    obj, cons = gen(n, mc, int(rng.randint(0, 1 << 30)))
    edge = seed % 3 == 0
    if edge:
        obj, cons, n, nv, md, cap = edge_draw(seed)
        mc = len(cons) - n
    st, T, nn = bb_cases.primal_final_tableau(oracle, obj, cons)
    if st != 0:
        seed += 1
        continue
    if edge:
        assert T.shape == (1 + len(cons), len(obj) + len(cons) + 1)
        nn = nv
    else:
        cap = int(rng.choice([20, 20, 40, 7]))
        md = max(cap, 20)
    ref = oracle.bb_solve(T, nn, node_cap=cap, rec_cap=1 << 12, piv_cap=1 << 18)
    tree = BranchBoundTree.from_array(eng, T, nn, max_depth=md)
    res, x = tree.run(node_cap=cap)
    tag = (seed, n, mc, cap, nn, md)
    assert res.status == ref["status"] and bool(res.found) == ref["found"], tag
    assert tree.pop_order() == ref["pop_order"] and tree.records() == ref["records"], tag
    assert tree.trace() == ref["trace"], tag
    if ref["found"]:
        assert bits(res.z) == bits(ref["z"]) and [bits(v) for v in x] == [bits(v) for v in ref["x"]], tag
    tree.destroy()
    drops += sum(1 for t in ref["trace"] if t[1] == 2)
    primal += sum(1 for t in ref["trace"] if t[1] == 1)
    # level-synchronous driver, 4 levels, against the oracle-backed evaluator
    levels = min(4, md)
    t2 = BranchBoundTree.from_array(eng, T, nn, max_depth=md if edge else 24)
    got = solve_level_sync_native(t2, max_levels=levels)
    t2.destroy()
    want = solve_level_synchronous(OracleEvaluator(oracle, T, nn), nn, max_levels=levels)
    for k in ("processed", "pivots", "levels", "found", "status"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    if want["found"]:
        assert bits(got["z"]) == bits(want["z"]) and got["path"] == tuple(want["path"]), tag
    cases += 1
    edge_cases += edge
    seed += 1
    if cases % 50 == 0:
        print(f"{cases} cases, seed {seed}, {primal} primal pivots, {drops} dropped tableaux", flush=True)
print(f"OK: {cases} instances ({edge_cases} from the edge space), seeds {seed0}..{seed - 1}: records, pop order, pivot traces ({primal} primal "
      f"pivots, {drops} dropped tableaux), incumbents identical to the oracle")
eng.close()
