"""GPU parity tests of the knapsack batch (lpr_knap_batch_*): every instance
of a batch against the restatement (tests/ref_py_knapsack.py) at the same node cap -- status, Z*,
selected items, rank, evaluated / levels / widest and the node records kept, integers by equality
and bounds by their bytes -- and the batch DP against the restatement's dp.  The instances are
those of tests/knapsack_batch_cases.py, whose properties tests/test_knapsack_batch_cpu.py pins."""
import ctypes
import struct

import numpy as np
import pytest

import knapsack_batch_cases as kb
import knapsack_cases as KC
import ref_py_knapsack as K

pytestmark = pytest.mark.gpu

NARRATE = 4096


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def make(engine, cases, narrate=NARRATE, caps=None):
    from lpr_381_group_v22_amd import KnapsackBatch
    C, w, v, cap = kb.pack(cases)
    return KnapsackBatch(C, w, v, node_cap=cap if caps is None else caps, narrate=narrate,
                         engine=engine)


def outputs(batch):
    """Everything the ABI gives for every instance, in comparable form."""
    s = batch.Stats()
    return dict(status=s["status"].tolist(), found=s["found"].tolist(), z=batch.Z(),
                evaluated=s["evaluated"].tolist(), widest=s["widest"].tolist(),
                levels=s["levels"].tolist(), selected=batch.SelectedIds(), rank=batch.Rank(),
                nodes=[[(nd.parent, nd.branch, nd.status, bits(nd.bound), nd.k, nd.V)
                        for nd in batch.Nodes(k)] for k in range(batch.count)])


def check_instance(out, k, ref, narrate=NARRATE, name=""):
    assert out["status"][k] == ref["status"], name
    assert out["evaluated"][k] == ref["evaluated"], name
    assert out["levels"][k] == ref["levels"], name
    assert out["widest"][k] == ref["widest"], name
    assert out["found"][k] == (0 if ref["z"] is None else 1), name
    assert out["z"][k] == (None if ref["z"] is None else float(ref["z"])), name
    assert out["selected"][k] == ref["selected"], name
    assert out["rank"][k] == ref["rank"], name
    rank = ref["rank"]
    want = [(p, br, st, bits(bd), rank[kk] if kk >= 0 else -1, V)
            for (p, br, st, bd, kk, V) in ref["records"][:narrate]]
    got = out["nodes"][k]
    assert len(got) == len(want), name
    if got != want:
        first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError(f"{name}: record {first}: {got[first]} != {want[first]}")


@pytest.fixture(scope="module")
def main(engine):
    """The main batch solved once with every default; the other tests compare against it."""
    cases = kb.main_batch()
    b = make(engine, cases)
    res = b.Solve()
    out = outputs(b)
    yield dict(cases=cases, batch=b, out=out, launches=res.launches,
               forms=(res.items_w, res.items_g, res.items_h),
               counts=(res.finished, res.capped, res.nodes))
    b.destroy()


def test_all_knapsack_cases_in_one_batch(main):
    """Test 1: all of knapsack_cases.all_cases() (and the LDS instances among them) as ONE batch,
    each instance at its own node cap, against the restatement."""
    cases, out = main["cases"], main["out"]
    want_forms = [kb.form_of(len(c["w"]), c["node_cap"]) for c in cases]
    assert main["forms"] == tuple(want_forms.count(f) for f in (0, 1, 2))
    assert min(main["forms"]) > 0
    for k, c in enumerate(cases):
        check_instance(out, k, kb.reference(c), name=c["name"])
    refs = [kb.reference(c) for c in cases]
    assert main["counts"] == (sum(r["status"] == K.OK for r in refs),
                              sum(r["status"] == K.NODE_CAP for r in refs),
                              sum(r["evaluated"] for r in refs))
    # the worked-out answers of the degenerate roots
    for k, c in enumerate(cases):
        if "z" in c:
            assert out["z"][k] == float(c["z"]), c["name"]
        if "selected" in c:
            assert out["selected"][k] == c["selected"], c["name"]


@pytest.mark.parametrize("variant, chunk", [(1, 0), (2, 0), (3, 0), (0, 1)])
def test_forms_and_chunks_give_the_same_bits(main, variant, chunk):
    """Test 2: the same batch with a form forced where it fits, and with chunk = 1, where every
    level boundary is a launch boundary and all state passes through the descriptor."""
    b = main["batch"]
    res = b.Solve(chunk=chunk, variant=variant)
    cases = main["cases"]
    want_forms = [kb.form_of(len(c["w"]), c["node_cap"], variant) for c in cases]
    assert (res.items_w, res.items_g, res.items_h) == tuple(want_forms.count(f) for f in (0, 1, 2))
    out = outputs(b)
    for key in main["out"]:
        assert out[key] == main["out"][key], key
    if chunk == 1:
        assert res.launches > main["launches"]
        assert res.launches >= max(main["out"]["levels"])


@pytest.mark.parametrize("count", [1, 3, 4, 5])
def test_small_counts(engine, count):
    """Test 3: W packs four instances per workgroup."""
    pool = [kb.sample(64), kb.strongly_correlated(11, 30, 200), kb.sample(5),
            kb.small_random(3, 9, 100), kb.strongly_correlated(13, 65, 150)]
    cases = pool[:count]
    assert all(kb.form_of(len(c["w"]), c["node_cap"]) == kb.FORM_W for c in cases)
    b = make(engine, cases)
    res = b.Solve()
    assert res.items_w == count and res.launches == 1
    out = outputs(b)
    for k, c in enumerate(cases):
        check_instance(out, k, kb.reference(c), name=c["name"])
    b.destroy()


def test_the_sample_257_times(engine):
    """Test 3: every copy equals the five-node table of DESIGN.md section 11."""
    b = make(engine, [kb.sample(64)] * 257)
    b.Solve()
    out = outputs(b)
    table = [(-1, 0, K.FRACTIONAL, bits(15.4), 4, 15), (0, 0, K.FRACTIONAL, bits(15.363636363636363), 0, 15),
             (0, 1, K.PRUNED, bits(14.142857142857142), 3, 12), (1, 0, K.INTEGRAL, bits(15.0), -1, 15),
             (1, 1, K.PRUNED, bits(13.785714285714286), 3, 12)]
    for k in range(257):
        assert out["nodes"][k] == table, k
        assert out["z"][k] == 15.0 and out["selected"][k] == [1, 2, 3, 5]
        assert (out["status"][k], out["evaluated"][k], out["levels"][k], out["widest"][k]) == (0, 5, 3, 2)
    lines = b.IterationLines(256)
    assert lines[0] == "Node 0: fixed none; fractional; bound = 15.4; k = x5; V = 15"
    assert lines[4] == "Node 1.2: fixed x5=0 x1=1; fractional, pruned; bound = 13.7857142857143; k = x4; V = 12"
    b.destroy()


def test_n64_next_to_n65_and_one_instance_per_form(engine):
    """Test 3: lane-per-node next to wave-per-node, and H, W, G in that order in one batch."""
    cases = [kb.strongly_correlated(13, 64, 150), kb.strongly_correlated(13, 65, 150),
             KC.by_name("big_multiword_n64"), KC.by_name("big_multiword_n65")] + kb.form_order_cases()
    b = make(engine, cases)
    res = b.Solve()
    assert (res.items_w, res.items_g, res.items_h) == (3, 1, 3)
    out = outputs(b)
    for k, c in enumerate(cases):
        check_instance(out, k, kb.reference(c), name=c["name"])
    b.destroy()


def test_footprint_at_and_beside_the_form_limits(engine):
    """Test 3: one node below, at and one node past the W and the G limit."""
    pairs = kb.limit_cases()
    cases = [c for c, _ in pairs]
    b = make(engine, cases)
    res = b.Solve()
    forms = [f for _, f in pairs]
    assert (res.items_w, res.items_g, res.items_h) == tuple(forms.count(f) for f in (0, 1, 2))
    out = outputs(b)
    for k, c in enumerate(cases):
        check_instance(out, k, kb.reference(c), name=c["name"])
    b.destroy()


def test_form_h_above_64_kib_of_items(engine):
    """n = 8065 at node cap 64 is form H by its footprint, and its ranked items (8 bytes each)
    with the workgroup's 1 KiB are 65 544 bytes of dynamic LDS: the fewest items that take form
    H's launch above the 64 KiB a kernel gets without the dynamic-LDS attribute."""
    c = kb.strongly_correlated(5, 8065, 64)
    assert kb.form_of(8065, 64) == 2
    assert 1024 + 8 * 8064 <= 64 * 1024 < 1024 + 8 * 8065
    b = make(engine, [c])
    res = b.Solve()
    assert (res.items_w, res.items_g, res.items_h) == (0, 0, 1)
    check_instance(outputs(b), 0, kb.reference(c), name=c["name"])
    b.destroy()


@pytest.mark.parametrize("which", [0, 1])
def test_node_cap(engine, which):
    """Test 4: caps of E, E - 1, E + 1 and one that stops the search after the root, all in one
    batch; twice on one handle; and a log shorter than the search."""
    c = kb.cap_cases()[which]
    E = kb.reference(c)["evaluated"]
    caps = [E, E - 1, E + 1, 2]
    b = make(engine, [c] * 4, caps=caps)
    b.Solve()
    out = outputs(b)
    for k, cap in enumerate(caps):
        check_instance(out, k, kb.reference(c, cap), name=f"{c['name']} cap {cap}")
    assert out["status"] == [K.OK, K.NODE_CAP, K.OK, K.NODE_CAP]
    b.Solve()
    again = outputs(b)
    assert again == out
    b.destroy()
    short = 7
    b = make(engine, [c, c], narrate=short, caps=[E, 2])
    b.Solve()
    out = outputs(b)
    check_instance(out, 0, kb.reference(c, E), narrate=short, name="short log")
    check_instance(out, 1, kb.reference(c, 2), narrate=short, name="short log, root only")
    assert len(out["nodes"][0]) == short and len(out["nodes"][1]) == 1
    b.destroy()


def test_dp(engine, main):
    """Test 5: the DP of the main batch where the restatement's dp is quick, and the edges."""
    cases = main["cases"]
    which = [c["C"] * len(c["w"]) <= 2_000_000 for c in cases]
    assert sum(which) >= 10 and not all(which)
    best = main["batch"].DP(which)
    for k, c in enumerate(cases):
        assert best[k] == (K.dp(c["C"], c["w"], c["v"]) if which[k] else -1), c["name"]
    edges = kb.dp_edge_cases()
    b = make(engine, edges, narrate=0)
    got = b.DP()
    assert got == [K.dp(c["C"], c["w"], c["v"]) for c in edges]
    skip = [k % 3 != 0 for k in range(len(edges))]
    got2 = b.DP(skip)
    assert got2 == [g if s else -1 for g, s in zip(got, skip)]
    b.destroy()


def test_solve_knapsacks_reports_results_match(engine):
    from lpr_381_group_v22_amd import solve_knapsacks
    c = kb.small_random(15, 10, 1024)
    out = solve_knapsacks([kb.SAMPLE, (c["C"], c["w"], c["v"])], engine=engine)
    assert out[0].Z == 15.0 and out[0].Chosen == [1, 2, 3, 5] and out[0].DP == 15.0
    assert out[0].ResultsMatch is True and out[0].Status == 0
    assert out[1].ResultsMatch is True and out[1].DP == K.dp(c["C"], c["w"], c["v"])


def test_refusals(engine, main):
    """Test 6."""
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    lib = N.lib
    I64, I32, D = (ctypes.POINTER(t) for t in (ctypes.c_int64, ctypes.c_int32, ctypes.c_double))

    def create(C, ns, w, v, caps=None, eng=engine):
        C = np.asarray(C, dtype=np.int64)
        ns = np.asarray(ns, dtype=np.int32)
        w = np.asarray(w, dtype=np.float64)
        v = np.asarray(v, dtype=np.float64)
        cp = None if caps is None else np.asarray(caps, dtype=np.int64)
        h = ctypes.c_void_p()
        rc = lib.lpr_knap_batch_create(eng._h, len(C), C.ctypes.data_as(I64), ns.ctypes.data_as(I32),
                                       w.ctypes.data_as(D), v.ctypes.data_as(D),
                                       None if cp is None else cp.ctypes.data_as(I64), 0,
                                       ctypes.byref(h))
        return rc, lib.lpr_last_error().decode(), h

    w = [1.0, 2.0, 3.0, 4.0] * 3
    w[2 * 4 + 3] = 2.5   # instance 2, index 3
    rc, msg, _ = create([9, 9, 9], [4, 4, 4], w, [1.0] * 12)
    assert rc == N.LPR_BAD_ARGUMENT and "instance 2" in msg and "weights[3]" in msg and "2.5" in msg
    rc, msg, _ = create([9, 9], [2, 0], [1.0, 2.0], [1.0, 1.0])
    assert rc == N.LPR_BAD_ARGUMENT and "instance 1" in msg and "n = 0" in msg
    rc, msg, _ = create([9], [8193], [1.0] * 8193, [1.0] * 8193)
    assert rc == N.LPR_BAD_ARGUMENT and "n = 8193" in msg
    rc, msg, _ = create([9, 9], [1, 1], [1.0, 1.0], [1.0, 1.0], caps=[5, (1 << 22) + 1])
    assert rc == N.LPR_BAD_ARGUMENT and "instance 1" in msg and "2^22" in msg
    rc, msg, h = create([9], [1], [1.0], [1.0], caps=[1 << 22])   # at the limit: accepted
    assert rc == 0, msg
    assert lib.lpr_knap_batch_destroy(h) == 0
    # the DP of the main batch: its first instance over the cell limit is refused by name
    b, cases = main["batch"], main["cases"]
    first = next(k for k, c in enumerate(cases) if c["C"] + 1 > kb.DP_MAX_CELLS)
    best = np.zeros(len(cases), dtype=np.int64)
    rc = lib.lpr_knap_batch_dp(b._h, None, best.ctypes.data_as(I64))
    assert rc == N.LPR_BAD_ARGUMENT
    msg = lib.lpr_last_error().decode()
    assert f"instance {first} " in msg and "lpr_knap_dp" in msg
    res = N.KnapBatchResult()
    opts = N.KnapBatchOpts(chunk=0, variant=4)
    assert lib.lpr_knap_batch_solve(b._h, ctypes.byref(opts), ctypes.byref(res)) == N.LPR_BAD_ARGUMENT
    assert lib.lpr_knap_batch_solve(b._h, None, None) == N.LPR_BAD_ARGUMENT
    cnt = ctypes.c_int64()
    assert lib.lpr_knap_batch_nodes_read(b._h, len(cases), None, None, None, None, None, None, 0,
                                         ctypes.byref(cnt)) == N.LPR_BAD_ARGUMENT
    # a destroyed engine orphans the handle
    eng2 = pkg.Engine(0)
    rc, msg, h = create([9], [1], [1.0], [1.0], eng=eng2)
    assert rc == 0, msg
    eng2.close()
    assert lib.lpr_knap_batch_solve(h, None, ctypes.byref(res)) == N.LPR_BAD_ARGUMENT
    assert "orphaned" in lib.lpr_last_error().decode()
    assert lib.lpr_knap_batch_dp(h, None, best.ctypes.data_as(I64)) == N.LPR_BAD_ARGUMENT
    assert lib.lpr_knap_batch_destroy(h) == 0
