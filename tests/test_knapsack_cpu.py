"""CPU tests of the knapsack rules as restated in tests/ref_py_knapsack.py:
brute force agreement, the sample table of the menu's hard-coded instance, tie ranking and the
node-cap rule, and the fixtures of tests/knapsack_cases.py: every property a case is meant to have
is asserted here, and every fractional record's bound is recomputed from the case's own numbers.
No GPU, no product import."""
import random
import struct
from fractions import Fraction

import pytest

import knapsack_cases as KC
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


# ---------------------------------------------------------------- fixtures of knapsack_cases.py
def audit_records(case, r):
    """Recompute every FRACTIONAL / PRUNED record from the case's numbers alone: the node's fixings
    from its parent chain, R and V by prefix sums, the bound as three correctly rounded steps taken
    through exact rationals, and the pruning rule against the running Z*.  Returns the count."""
    C, rank, recs = case["C"], r["rank"], r["records"]
    w = [case["w"][i] for i in rank]
    v = [case["v"][i] for i in rank]
    pw, pv = [0], [0]
    for a, b in zip(w, v):
        pw.append(pw[-1] + a)
        pv.append(pv[-1] + b)
    fixed = []  # per record: tuple of (rank position, value) fixings, root first
    checked = 0
    for base, W, _ in KC.level_split(recs):
        level = recs[base:base + W]
        for par, br, *_ in level:
            fixed.append(() if par < 0 else fixed[par] + ((recs[par][4], br),))
        zstar = max(rec[5] for rec in recs[:base + W] if rec[2] != K.INFEASIBLE)
        for i, (par, br, st, bound, k, V) in enumerate(level):
            if st not in (K.FRACTIONAL, K.PRUNED):
                continue
            fx = fixed[base + i]
            w1 = sum(w[p] for p, x in fx if x)
            v1 = sum(v[p] for p, x in fx if x)
            R = C - w1 - (pw[k] - sum(w[p] for p, _ in fx if p < k))
            assert V == v1 + pv[k] - sum(v[p] for p, _ in fx if p < k)
            assert 0 < R < w[k] and all(p != k for p, _ in fx)
            q = float(Fraction(R, w[k]))
            t = float(Fraction(v[k]) * Fraction(q))
            want = float(Fraction(V) + Fraction(t))
            assert bits(bound) == bits(want), (case["name"], base + i)
            assert (st == K.FRACTIONAL) == (Fraction(want) > zstar), (case["name"], base + i)
            checked += 1
    return checked


@pytest.mark.parametrize("name", KC.case_names())
def test_case_properties(name):
    c = KC.by_name(name)
    r = KC.reference(name)
    recs, fam, n = r["records"], c["family"], len(c["w"])
    # the inputs the engine accepts
    assert 1 <= n <= 8192 and c["C"] >= 0
    assert all(1 <= x <= KC.BIG_HI for x in c["w"]) and all(0 <= x <= KC.BIG_HI for x in c["v"])
    assert len(recs) == r["evaluated"] <= c["node_cap"]
    assert sum(W for _, W, _ in KC.level_split(recs)) == r["evaluated"]
    assert len(KC.level_split(recs)) == r["levels"]
    assert max(W for _, W, _ in KC.level_split(recs)) == r["widest"]
    ks = [rec[4] for rec in recs if rec[4] >= 0]
    vmax = max(rec[5] for rec in recs)
    if c.get("status") is not None:
        assert r["status"] == c["status"], "fixture no longer ends with the status it is meant to"
    if c.get("k_min") is not None:
        assert ks and max(ks) >= c["k_min"], f"fixture no longer has a record with k >= {c['k_min']}"
    sel = r["selected"]
    assert sel == sorted(set(sel)) and sum(c["w"][i] for i in sel) <= c["C"]
    assert sum(c["v"][i] for i in sel) == r["z"]
    if fam in ("big", "big_multiword", "max_items", "max_items_late", "all_branch_wide") or \
            name == "wide_mixed_big":
        assert all(KC.BIG_LO <= x <= KC.BIG_HI for x in c["w"])
        if n >= 6:
            assert c["C"] > KC.TWO32, "fixture no longer has C > 2^32"
            assert vmax >= KC.TWO32, "fixture no longer has a record with V >= 2^32"
    if fam == "big" and n <= 14:
        assert r["z"] == K.brute_force(c["C"], c["w"], c["v"])
    if fam == "max_items_late":
        sts = {rec[2] for rec in recs}
        assert K.INTEGRAL in sts and K.FRACTIONAL in sts, \
            "fixture no longer mixes integral and fractional records"
        assert max(ks) // 64 == (n - 1) // 64, "fixture no longer puts k in the last bitmap word"
    if fam == "wide_mixed":
        mixed = KC.mixed_wide_levels(recs)
        assert r["widest"] > 2048, "fixture no longer has a level wider than 2048"
        assert len(mixed) >= 3, "fixture no longer has three wide levels of mixed branching"
    if fam == "all_branch_wide":
        wide = [(W, b) for _, W, b in KC.level_split(recs) if W >= 2048]
        assert [W for W, _ in wide] == [2048, 4096, 8192, 16384] and all(W == b for W, b in wide), \
            "fixture no longer has wide levels in which every node branches"
        assert r["rank"] == list(range(n))
        if c.get("tied_incumbent"):
            # a level over 1024 wide that replaces the incumbent, with its largest V at several
            # nodes and not at the first
            tied, zstar = [], -1
            for base, W, _ in KC.level_split(recs):
                Vs = [rec[5] for rec in recs[base:base + W]]
                if max(Vs) > zstar:
                    zstar = max(Vs)
                    if W > 1024 and Vs.count(zstar) > 1 and Vs.index(zstar) > 0:
                        tied.append((W, Vs.count(zstar), Vs.index(zstar)))
            assert tied, "fixture no longer takes an incumbent from a wide level of equal V"
    if fam == "degenerate":
        for key in ("z", "selected", "evaluated"):
            if key in c:
                assert r[key] == c[key], (key, r[key])
        if "never_selected" in c:
            assert c["never_selected"] not in sel and r["rank"][0] == c["never_selected"]
            assert r["z"] == K.brute_force(c["C"], c["w"], c["v"])
        if c["C"] >= sum(c["w"]):
            assert recs == [(-1, 0, K.INTEGRAL, float(sum(c["v"])), -1, sum(c["v"]))]
    checked = audit_records(c, r)
    assert checked == sum(1 for rec in recs if rec[2] in (K.FRACTIONAL, K.PRUNED))


def test_case_families_reach_what_they_are_for():
    """Properties that hold over a family, not per case."""
    fam = {}
    for c in KC.all_cases():
        fam.setdefault(c["family"], []).append(c)
    assert {len(c["w"]) for c in fam["big"]} == {1, 6, 12, 20}
    assert {len(c["w"]) for c in fam["big_multiword"]} == {64, 65, 128, 129, 200}
    assert {len(c["w"]) for c in fam["max_items"]} == {8192, 8129} == \
        {len(c["w"]) for c in fam["max_items_late"]}
    sts = set()
    for c in fam["big_multiword"]:
        sts |= {rec[2] for rec in KC.reference(c["name"])["records"]}
    assert sts == {K.FRACTIONAL, K.PRUNED, K.INTEGRAL, K.INFEASIBLE}, \
        "big_multiword no longer shows records of all four statuses"
    # k crosses a word boundary inside one search: records with k in word 0 and in a later word
    for c in fam["big_multiword"]:
        if len(c["w"]) > 64:
            words = {rec[4] // 64 for rec in KC.reference(c["name"])["records"] if rec[4] >= 0}
            assert len(words) >= 2, c["name"]
    assert len(fam["wide_mixed"]) == 2


def test_level_split_on_the_sample():
    r = K.branch_and_bound(*SAMPLE)
    assert KC.level_split(r["records"]) == [(0, 1, 1), (1, 2, 1), (3, 2, 0)]
    assert KC.level_of(r["records"], 0) == (0, 0, 1) and KC.level_of(r["records"], 4) == (2, 3, 2)
    assert KC.level_split(r["records"][:2]) == [(0, 1, 1), (1, 2, 1)]
