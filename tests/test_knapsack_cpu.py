"""CPU tests of the knapsack rules as restated in tests/ref_py_knapsack.py:
brute force agreement, the sample table of the menu's hard-coded instance, tie ranking and the
node-cap rule.  No GPU, no product import."""
import random
import struct

import ref_py_knapsack as K

SAMPLE = (40, [11, 8, 6, 14, 10, 10], [2, 3, 3, 5, 2, 4])


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_sample_table_exactly():
    r = K.branch_and_bound(*SAMPLE)
    rank = r["rank"]
    got = [(lab, rec[2], bits(rec[3]), rank[rec[4]] if rec[4] >= 0 else None, rec[5])
           for lab, rec in zip(K.labels(r["records"]), r["records"])]
    want = [("0", K.FRACTIONAL, bits(15.4), 4, 15),
            ("1", K.FRACTIONAL, bits(15.363636363636363), 0, 15),
            ("2", K.PRUNED, bits(14.142857142857142), 3, 12),
            ("1.1", K.INTEGRAL, bits(15.0), None, 15),
            ("1.2", K.PRUNED, bits(13.785714285714286), 3, 12)]
    assert got == want
    assert r["z"] == 15 and r["selected"] == [1, 2, 3, 5]
    assert (r["levels"], r["evaluated"], r["widest"], r["status"]) == (3, 5, 2, K.OK)
    assert K.dp(*SAMPLE) == 15 == K.brute_force(*SAMPLE)


def test_against_brute_force():
    rng = random.Random(1234)
    for trial in range(300):
        n = rng.randint(1, 16)
        top = rng.choice([5, 30, 1000])
        w = [rng.randint(1, top) for _ in range(n)]
        v = [rng.randint(0, top) for _ in range(n)]
        if trial % 3 == 0:  # equal ratios
            v = [x * rng.choice([1, 2]) for x in w]
        C = rng.randint(0, sum(w))
        bf = K.brute_force(C, w, v)
        r = K.branch_and_bound(C, w, v)
        assert r["z"] == bf, (C, w, v)
        assert K.dp(C, w, v) == bf
        sel = r["selected"]
        assert sel == sorted(set(sel))
        assert sum(w[i] for i in sel) <= C and sum(v[i] for i in sel) == bf


def test_tie_ranking():
    # equal ratios keep the original order; exact products decide ratios a double would merge
    assert K.rank_items([2, 4, 1, 3], [4, 8, 2, 6]) == [0, 1, 2, 3]
    assert K.rank_items([3, 1, 2], [3, 1, 2]) == [0, 1, 2]
    w = [2147483647, 2147483646]
    v = [2147483646, 2147483645]
    # 2147483646/2147483647 > 2147483645/2147483646 (cross products differ by 1)
    assert K.rank_items(w, v) == [0, 1]
    assert K.rank_items(w[::-1], v[::-1]) == [1, 0]
    assert K.rank_items([5, 5, 1], [0, 0, 0]) == [0, 1, 2]


def test_node_cap_rule():
    full = K.branch_and_bound(*SAMPLE)
    # a level is evaluated only if the evaluated total stays within the cap
    for cap, levels, z in ((1, 1, 15), (2, 1, 15), (3, 2, 15), (4, 2, 15), (5, 3, 15)):
        r = K.branch_and_bound(*SAMPLE, node_cap=cap)
        assert r["levels"] == levels and r["z"] == z
        assert r["status"] == (K.OK if cap >= 5 else K.NODE_CAP)
        assert r["records"] == full["records"][:r["evaluated"]]
    rng = random.Random(3)
    w = [rng.randint(1, 1000) for _ in range(100)]
    v = [x + 100 for x in w]
    r = K.branch_and_bound(sum(w) // 2, w, v, node_cap=3000, records=False)
    assert r["status"] == K.NODE_CAP and r["evaluated"] <= 3000 and r["z"] is not None


def test_dp_edges():
    assert K.dp(0, [], []) == 0
    assert K.dp(10, [0, 0], [5, -3]) == 5
    assert K.dp(5, [6, 2], [100, -1]) == 0
    assert K.dp(0, [0, 1], [7, 9]) == 7
