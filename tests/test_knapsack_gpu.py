"""GPU tests of menu option 5 (Program.cs:430-470): the device branch-and-bound node by node against
tests/ref_py_knapsack.py, the device DP against numpy, bad arguments, and the option's console text.
The instances of tests/knapsack_cases.py (sums over 2^32, n > 64 up to 8192, levels over 2048 wide)
have their properties asserted in tests/test_knapsack_cpu.py; here each is compared record by
record, and so are short logs, node caps at and around the evaluated total, and repeated solves on
one handle.  Every comparison is exact: integers, or doubles by their bits."""
import random
import struct

import numpy as np
import pytest

import knapsack_cases as KC
import ref_py_knapsack as K

pytestmark = pytest.mark.gpu

SAMPLE = (40, [11, 8, 6, 14, 10, 10], [2, 3, 3, 5, 2, 4])


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def device_bb(engine, C, w, v, node_cap=0, narrate=1 << 16):
    from lpr_381_group_v22_amd.knapsack import KnapsackBranchBoundSimplex
    s = KnapsackBranchBoundSimplex(C, [float(x) for x in w], [float(x) for x in v], engine=engine,
                                   node_cap=node_cap, narrate=narrate)
    s.Solve()
    return s


def ref_nodes(r):
    return [(par, br, st, bits(b), r["rank"][k] if k >= 0 else -1, V)
            for (par, br, st, b, k, V) in r["records"]]


def dev_nodes(s):
    return [(n.parent, n.branch, n.status, bits(n.bound), n.k, n.V) for n in s.Nodes()]


def compare_with_ref(s, r, narrate):
    """A solved handle against a restatement run with the same node cap: status, Z*, the selected
    ids, the counters, the rank, and the node log (the first `narrate` records, or all of them)."""
    assert s.Status == r["status"]
    assert s.Z == r["z"] and s.SelectedIds() == r["selected"]
    assert (s.Evaluated, s.Levels, s.Widest) == (r["evaluated"], r["levels"], r["widest"])
    assert s.Rank() == r["rank"]
    got, want = dev_nodes(s), ref_nodes(r)[:max(narrate, 0)]
    if got != want:
        assert len(got) == len(want), f"{len(got)} records kept, {len(want)} expected"
        i = next(j for j, (a, b) in enumerate(zip(got, want)) if a != b)
        lv, base, width = KC.level_of(r["records"], i)
        raise AssertionError(
            f"record {i} differs (level {lv}: records {base}..{base + width - 1}, "
            f"{dict((b, n) for b, _, n in KC.level_split(r['records']))[base]} of them branched): "
            f"device {got[i]}, restatement {want[i]}")


def check_against_ref(engine, C, w, v, node_cap=K.DEFAULT_NODE_CAP, records=True,
                      narrate=1 << 16, ref=None):
    """ref: a restatement run of the same instance and node cap made earlier (with records)."""
    r = ref if ref is not None else K.branch_and_bound(C, w, v, node_cap=node_cap, records=records)
    narrate = narrate if records else 0
    s = device_bb(engine, C, w, v, node_cap=node_cap, narrate=narrate)
    compare_with_ref(s, r, narrate)
    s.destroy()
    return r


def test_sample_table(engine):
    from lpr_381_group_v22_amd.knapsack import KnapsackBranchBoundSolver, node_labels
    s = device_bb(engine, *SAMPLE, narrate=-1)  # auto: n <= 64
    nodes = s.Nodes()
    got = [(lab, n.status, bits(n.bound), n.k, n.V) for lab, n in zip(node_labels(nodes), nodes)]
    assert got == [("0", K.FRACTIONAL, bits(15.4), 4, 15),
                   ("1", K.FRACTIONAL, bits(15.363636363636363), 0, 15),
                   ("2", K.PRUNED, bits(14.142857142857142), 3, 12),
                   ("1.1", K.INTEGRAL, bits(15.0), -1, 15),
                   ("1.2", K.PRUNED, bits(13.785714285714286), 3, 12)]
    assert s.Z == 15.0 and s.Status == 0 and (s.Levels, s.Evaluated) == (3, 5)
    assert [it.Id for it in s.GetSelectedItemsOriginal()] == [1, 2, 3, 5]
    assert KnapsackBranchBoundSolver.Solve(*SAMPLE, engine=engine) == 15.0
    s.destroy()


def test_random_branch_and_bound(engine):
    rng = random.Random(7)
    for trial in range(60):
        n = rng.randint(1, 20)
        top = rng.choice([10, 100, 1000])
        w = [rng.randint(1, top) for _ in range(n)]
        if trial % 2:  # ties in ratio
            v = [x * rng.choice([1, 2, 3]) for x in w]
        else:
            v = [rng.randint(0, top) for _ in range(n)]
        C = rng.randint(0, sum(w))
        r = check_against_ref(engine, C, w, v)
        if n <= 14:
            assert r["z"] == K.brute_force(C, w, v)


def test_large_branch_and_bound(engine):
    rng = random.Random(2)
    w = [rng.randint(1, 1000) for _ in range(200)]
    v = [rng.randint(1, 1000) for _ in range(200)]
    r = check_against_ref(engine, sum(w) // 2, w, v, records=False)
    assert r["status"] == K.OK
    random.seed(3)
    w = [random.randint(1, 1000) for _ in range(100)]
    v = [x + 100 for x in w]
    r = check_against_ref(engine, sum(w) // 2, w, v, node_cap=100000, records=False)
    assert r["status"] == K.NODE_CAP


@pytest.mark.parametrize("name", KC.case_names())
def test_bb_cases(engine, name):
    c = KC.by_name(name)
    r = KC.reference(name)
    assert r["evaluated"] <= c["node_cap"]
    check_against_ref(engine, c["C"], c["w"], c["v"], node_cap=c["node_cap"],
                      narrate=max(1 << 16, c["node_cap"]), ref=r)


def not_recorded_line(r, kept):
    return f"({r['evaluated'] - kept} of {r['evaluated']} nodes in {r['levels']} levels not recorded)"


@pytest.mark.parametrize("name", ["wide_mixed_small", "wide_mixed_big"])
def test_truncated_log(engine, name):
    """A log shorter than the search keeps the first records and changes nothing else."""
    from lpr_381_group_v22_amd.knapsack import KnapsackNode, narration_lines
    c = KC.by_name(name)
    r = KC.reference(name)
    E = r["evaluated"]
    assert E > 1025
    s = device_bb(engine, c["C"], c["w"], c["v"], node_cap=c["node_cap"], narrate=E)
    assert len(s.Nodes()) == E
    full_lines = s.IterationLines()
    assert len(full_lines) == E  # nothing left out, no count line
    for narrate in (1, 1000, 1025, E - 1):
        s.narrate = narrate
        s.Solve()
        assert len(s.Nodes()) == narrate
        compare_with_ref(s, r, narrate)
        lines = s.IterationLines()
        assert len(lines) == narrate + 1 and lines[-1] == not_recorded_line(r, narrate)
        assert lines[:-1] == full_lines[:narrate]
    # the text of the kept records, built from the restatement alone
    want = narration_lines([KnapsackNode(*rec[:3], rec[3], r["rank"][rec[4]] if rec[4] >= 0 else -1,
                                         rec[5]) for rec in r["records"][:1000]], E, r["levels"])
    s.narrate = 1000
    s.Solve()
    assert s.IterationLines() == want and want[-1] == not_recorded_line(r, 1000)
    # a log longer than the node cap holds min(evaluated, node_cap) records
    cap = 2000
    rc = KC.reference(name, cap)
    assert rc["status"] == K.NODE_CAP and 1024 < rc["evaluated"] <= cap
    s.node_cap, s.narrate = cap, 3 * cap
    s.Solve()
    assert len(s.Nodes()) == rc["evaluated"]
    compare_with_ref(s, rc, 3 * cap)
    assert len(s.IterationLines()) == rc["evaluated"]
    s.destroy()


def test_node_cap_boundaries(engine):
    """node_cap exactly at the evaluated total finishes; one below, and 1, stop with NODE_CAP and
    the incumbent so far."""
    name = "big_multiword_n128"
    c = KC.by_name(name)
    full = KC.reference(name)
    E = full["evaluated"]
    assert full["status"] == K.OK and E < c["node_cap"]
    at = KC.reference(name, E)
    assert at["status"] == K.OK and at["records"] == full["records"] and at["z"] == full["z"]
    check_against_ref(engine, c["C"], c["w"], c["v"], node_cap=E, ref=at)
    below = KC.reference(name, E - 1)
    assert below["status"] == K.NODE_CAP and below["evaluated"] < E
    assert below["records"] == full["records"][:below["evaluated"]]
    check_against_ref(engine, c["C"], c["w"], c["v"], node_cap=E - 1, ref=below)
    one = KC.reference(name, 1)
    assert one["status"] == K.NODE_CAP and (one["evaluated"], one["levels"]) == (1, 1)
    assert one["z"] is not None and one["z"] < full["z"]
    check_against_ref(engine, c["C"], c["w"], c["v"], node_cap=1, ref=one)


def test_resolve_on_one_handle(engine):
    """Solve() again on one handle with another node cap and log length: the log is re-allocated,
    and the incumbent, its bitmaps and the selected ids start afresh each time."""
    name = "wide_mixed_big"
    c = KC.by_name(name)
    full = KC.reference(name)
    assert full["status"] == K.OK  # node_cap 0 (the default 2^22) then runs the same search
    short, mid = KC.reference(name, 500), KC.reference(name, 2000)
    assert short["status"] == mid["status"] == K.NODE_CAP
    assert short["selected"] != full["selected"] and mid["selected"] != full["selected"]
    assert short["z"] <= mid["z"] < full["z"]
    big = max(1 << 16, c["node_cap"])
    s = device_bb(engine, c["C"], c["w"], c["v"], node_cap=500, narrate=0)
    compare_with_ref(s, short, 0)
    for node_cap, narrate, r in ((0, big, full), (2000, 100, mid), (c["node_cap"], big, full),
                                 (500, 0, short)):
        s.node_cap, s.narrate = node_cap, narrate
        s.Solve()
        compare_with_ref(s, r, narrate)
    s.destroy()


def np_dp(C, w, v):
    row = np.zeros(C + 1, dtype=np.int64)
    for a, b in zip(w, v):
        if a <= C:
            row[a:] = np.maximum(row[a:], row[:C + 1 - a] + b)
    return int(row[C])


@pytest.mark.parametrize("case", [
    "multi_block", "wide_items", "zero_weights", "heavier_than_capacity", "zero_capacity",
    "no_items", "negative_values", "mixed", "big_row"])
def test_dp(engine, case):
    from lpr_381_group_v22_amd.knapsack import knapsack_dp
    rng = np.random.default_rng(sum(map(ord, case)))
    if case == "multi_block":  # many blocks of the 6144-cell halo, many 4096-cell tiles
        C, w, v = 60000, rng.integers(1, 2049, 300), rng.integers(1, 1001, 300)
    elif case == "wide_items":  # weights over the halo take streaming passes
        C = 100000
        w = np.array([7000, 20000, 6144, 6145, 3, 50000, 99999, 100000])
        v = rng.integers(1, 1000, len(w))
    elif case == "zero_weights":
        C, w, v = 5000, np.array([0, 0, 5, 0, 4000, 0]), np.array([3, 9, 7, -2, 11, 1])
    elif case == "heavier_than_capacity":
        C, w, v = 100, np.array([101, 5000, 7, 200000]), np.array([50, 60, 2, 70])
    elif case == "zero_capacity":
        C, w, v = 0, np.array([0, 1, 2, 0]), np.array([4, 9, 9, -1])
    elif case == "no_items":
        C, w, v = 12345, np.array([], dtype=np.int64), np.array([], dtype=np.int64)
    elif case == "negative_values":
        C, w, v = 9000, rng.integers(0, 3000, 40), rng.integers(-500, 500, 40)
    elif case == "mixed":
        C = 40000
        w = rng.integers(0, 12000, 200)
        v = rng.integers(-100, 2 ** 31 - 1, 200)
    else:  # C = 2^24, n = 64
        C, w, v = 1 << 24, rng.integers(1, 2049, 64), rng.integers(1, 1001, 64)
    want = np_dp(C, w.tolist(), v.tolist())
    assert knapsack_dp(C, w, v, engine=engine) == want
    assert knapsack_dp(C, w, v, engine=engine, variant=1) == want
    if len(w) <= 16 and C <= 10000:
        assert want == K.dp(C, w.tolist(), v.tolist())


DP_BOUNDARY_CAPACITIES = (4094, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 10239, 10240, 10241,
                          12288, 14335, 14336)


def dp_boundary_lists(C):
    """Item lists (weights, values) placed on the edges of the blocked DP: the 4096-cell tile, the
    6144-cell halo and the 1024-cell chunk walk."""
    rng = random.Random(11)
    big = lambda n: [rng.randint(1 << 30, (1 << 31) - 1) for _ in range(n)]  # noqa: E731
    a_w = [2048, 2048, 2048, 1, 5, 6139, 1]   # a block of exactly 6144, a flush, 6144 again, a flush
    b_w = [0, 3000, 0, 3144, 0]               # zero weights first and last in a full-halo block
    c_w = [7, 6145, 11, 9000, 13]             # streamed items between one-item blocks
    e_w = [rng.randint(900, 1100) for _ in range(60)]  # blocks of 5-6 items with S > 4096
    return {
        "a": (a_w, [rng.randint(1, 1000) for _ in a_w]),
        "b": (b_w, [5, 700, -3, 650, 2]),
        "c": (c_w, [rng.randint(1, 1000) for _ in c_w]),
        "d1": ([C], [17]),
        "d2": ([C, 1], [17, 20]),
        "e": (e_w, big(60)),
    }


@pytest.mark.parametrize("which", ["a", "b", "c", "d1", "d2", "e"])
def test_dp_boundaries(engine, which):
    """Only dp[C] comes back, so the other cells are observed by solving one item list at many
    capacities: C + 1 on and beside a tile edge, the halo and multiples of the chunk."""
    from lpr_381_group_v22_amd.knapsack import knapsack_dp
    top = max(DP_BOUNDARY_CAPACITIES)
    if which in ("d1", "d2"):
        rows = None
    else:  # one numpy row per item list: dp[C] of a shorter row is the same cell of a longer one
        w, v = dp_boundary_lists(top)[which]
        row = np.zeros(top + 1, dtype=np.int64)
        for a, b in zip(w, v):
            row[a:] = np.maximum(row[a:], row[:top + 1 - a] + b)
        rows = row
    bad = []
    for C in DP_BOUNDARY_CAPACITIES:
        w, v = dp_boundary_lists(C)[which]
        want = np_dp(C, w, v) if rows is None else int(rows[C])
        if which == "e" and C >= 8191:
            assert want > 1 << 32  # the int64 cells carry more than 32 bits
        for variant in (0, 1):
            got = knapsack_dp(C, w, v, engine=engine, variant=variant)
            if got != want:
                bad.append((C, variant, got, want))
    assert not bad, f"(C, variant, device, numpy): {bad}"


def test_bad_arguments_leave_the_engine_usable(engine):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.knapsack import KnapsackBranchBoundSimplex, knapsack_dp
    cases = [
        (lambda: KnapsackBranchBoundSimplex(40, [11, 8.5], [2, 3], engine=engine), "weights[1]"),
        (lambda: KnapsackBranchBoundSimplex(40, [11, 0], [2, 3], engine=engine), "weights[1]"),
        (lambda: KnapsackBranchBoundSimplex(40, [1.0] * 8193, [1.0] * 8193, engine=engine),
         "8193"),
        (lambda: KnapsackBranchBoundSimplex(40, [3, 4], [2, -1], engine=engine), "values[1]"),
        (lambda: knapsack_dp(40, [3, -4, 5], [1, 1, 1], engine=engine), "weights[1]"),
        (lambda: knapsack_dp(-1, [3], [1], engine=engine), "capacity"),
    ]
    for make, text in cases:
        with pytest.raises(N.EngineError) as ei:
            make()
        assert ei.value.status == N.LPR_BAD_ARGUMENT
        assert text in str(ei.value)
    s = device_bb(engine, *SAMPLE)
    assert s.Z == 15.0 and knapsack_dp(*SAMPLE, engine=engine) == 15
    # a handle outlives the engine it was made on: orphaned, then refused, then destroyable
    eng2 = pkg.Engine(0)
    s2 = KnapsackBranchBoundSimplex(*SAMPLE, engine=eng2)
    eng2.close()
    with pytest.raises(N.EngineError):
        s2.Solve()
    s2.destroy()
    s.destroy()


def test_program_option5(engine, capsys, tmp_path):
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd.program import run_option
    p = pkg.InputFileParser()
    r = run_option(p, "5", str(tmp_path / "o.txt"), engine=engine)
    out = capsys.readouterr().out
    lines = out.splitlines()
    assert lines[:10] == [
        "Solving with Branch and Bound Knapsack Algorithm...", "Knapsack Problem", "Capacity: 40",
        "Items (Value, Weight):", "  Item 1: Value=2, Weight=11", "  Item 2: Value=3, Weight=8",
        "  Item 3: Value=3, Weight=6", "  Item 4: Value=5, Weight=14",
        "  Item 5: Value=2, Weight=10", "  Item 6: Value=4, Weight=10"]
    i = lines.index("=== Branch and Bound Detailed Steps ===")
    assert lines[i + 1:i + 6] == [
        "Node 0: fixed none; fractional; bound = 15.4; k = x5; V = 15",
        "Node 1: fixed x5=0; fractional; bound = 15.3636363636364; k = x1; V = 15",
        "Node 2: fixed x5=1; fractional, pruned; bound = 14.1428571428571; k = x4; V = 12",
        "Node 1.1: fixed x5=0 x1=0; integral; bound = 15; k = -; V = 15",
        "Node 1.2: fixed x5=0 x1=1; fractional, pruned; bound = 13.7857142857143; k = x4; V = 12"]
    assert lines[i + 6:i + 8] == ["", "Chosen items (original numbering):"]
    assert lines[i + 8:] == [
        "  x2 = 1  (Value=3, Weight=8)", "  x3 = 1  (Value=3, Weight=6)",
        "  x4 = 1  (Value=5, Weight=14)", "  x6 = 1  (Value=4, Weight=10)",
        "Total Weight = 38", "Branch & Bound Best Value Z* = 15", "",
        "=== Comparison with Dynamic Programming ===", "Dynamic Programming Result: 15",
        "Results Match: True"]
    assert r["z"] == 15.0 and r["dp"] == 15.0
