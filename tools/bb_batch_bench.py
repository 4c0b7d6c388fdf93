"""Measures the batched Branch & Bound and prints one JSON line per workload:

  W   65536 option-3 IPs: n ~ U{6..10} binaries, m ~ U{1..3} integer-weight knapsack rows
      (c ~ U{1..19}, a ~ U{1..14}, b = floor(sum(a) * U(0.3, 0.6))), node_cap 20
  G   4096 IPs of 24 binaries x 8 rows, the same style
  H   256 IPs of 96 binaries x 32 rows, the same style

Every model goes through option 3 up to the root: the n rows "x_i <= 1", PrimalSimplexSolver (one
PrimalSimplexBatch, not timed), FinalTableau and SetNumVars as SolveFromPrimal sets them.
Per workload: IPs/s, pops/s and pivots/s end to end (lpr_bb_batch_create from the host roots,
lpr_bb_batch_run, the bulk reads of results and x, closed by an engine sync) and for
lpr_bb_batch_run alone (best of --repeat); launches; the forms the IPs took; the same roots one at
a time through BranchBoundTree.from_array + run in a Python loop (a time-bounded prefix); the CPU
oracle on one core (a prefix).  256 IPs per workload are checked against the oracle's orc_bb_solve
bit for bit (status, found, processed, best_node, z, x, every record, pop order, pivot count, the
kept trace); any mismatch makes the exit status non-zero.  Inputs are seeded (numpy
RandomState(seed + workload)).

--narrate measures the narrated batch instead, per workload (--ips N keeps
the first N IPs of each): (a) narrated end to end -- create, the two-pass reserve (reserve 0, run,
read the needs, reserve them), run, lpr_bb_batch_narrate_read_all; (a') that narrated run alone;
(b) the un-narrated end to end and run in the same process; (c) the per-model number-gathering
loop of the single-handle path (gather_branch_and_bound_numbers, no formatting) on a timed prefix,
marked "extrapolated" where scaled to the whole workload.  The only speed-up stated is (c)/(a).
256 IPs per workload are compared record by record with that loop's numbers (pop scores, child
status, pivots and every child tableau, the incumbent's tableau); mismatches make the exit status
non-zero.

--narrate --device-text measures the device text of the narrated batch on
the same three workloads, cut by --text-ips (default W=2048,G=512,H=32: the slab of child tableaux
and its text, about 6.5 bytes per cell, are both on the device and the text is read back whole, so
the 20 GB slabs of G and H are cut to about 2.5 GB) and writes one JSON line per workload and a
summary line to profiles/bb_batch_narr_text_bench.json: (a) the kernels of one
lpr_bb_batch_narrate_text (kernel_ms of lpr_text_info) and the call's wall-clock, one warm-up and
--repeat recorded passes; (b) end to end, FormatNarration() and NarrationTextDevice(k) for every
IP, --repeat passes; (c) the host path on the same handle, NarrationText(k) over evenly spaced IPs
in a fixed shuffled order, each pass cut at --host-seconds (an IP that has begun is finished), per
IP.  clears_bar: on every workload the slowest device pass per IP is below the fastest host pass
per IP.  NarrationTextDevice(k) == NarrationText(k) is checked on up to 256 of those IPs, as many
as --check-seconds of host formatting allow; the mismatch count is recorded and makes the exit
status non-zero.

Run it under a time limit:  timeout -k 10 1200 python tools/bb_batch_bench.py [--out FILE]
Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python
tools/bb_batch_bench.py --no-check --repeat 1
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

CHECK = 256
NODE_CAP = 20
TRACE_CAP = 256
W_MAX, G_MAX = (64 * 1024 - 1024) // 4, 160 * 1024 - 1024  # kBatchMaxLdsW / kBatchMaxLdsG


def gen_models(name: str, seed: int, limit: int = 0):
    """Option-3 models (objective, constraints with the unit rows, True) of one workload; with
    ``limit`` its first ``limit`` models (the generator draws model by model)."""
    from lpr_381_group_v22_amd import Constraint
    rng = np.random.RandomState(seed)
    count, fixed = {"W": (65536, None), "G": (4096, (24, 8)), "H": (256, (96, 32))}[name]
    models = []
    for _ in range(min(count, limit) if limit > 0 else count):
        n, m = fixed if fixed else (int(rng.randint(6, 11)), int(rng.randint(1, 4)))
        c = rng.randint(1, 20, size=n).astype(float)
        A = rng.randint(1, 15, size=(m, n)).astype(float)
        b = np.floor(A.sum(axis=1) * rng.uniform(0.3, 0.6, size=m))
        cons = [Constraint(A[i].tolist(), "<=", float(b[i])) for i in range(m)]
        for i in range(n):  # program._append_unit_bound_rows
            co = [0.0] * (n + 3)
            co[i] = 1.0
            co[n + 1] = 1.0
            cons.append(Constraint(co, "<=", 1.0))
        models.append((c.tolist(), cons, True))
    return models


def roots_of(pkg, N, eng, models):
    """FinalTableau and SetNumVars (BranchAndBoundAdapter.cs:20) of every model."""
    lp = pkg.PrimalSimplexBatch(models, engine=eng)
    lp.Solve()
    roots, nvars = [], []
    for k in range(lp.Count):
        T = lp.GetFinalTableau(k)
        roots.append(T)
        nvars.append(lp.Shape(k)[2] if lp.Status[k] == N.LPR_OK_OPTIMAL
                     else max(1, T.shape[1] - 1))
    lp.destroy()
    return roots, nvars


def form_of(T):
    r, c = T.shape[0] + NODE_CAP, T.shape[1] + NODE_CAP
    b = 8 * (2 * r * c + r)
    return "W" if b <= W_MAX else ("G" if b <= G_MAX else "H")


T0 = time.perf_counter()


def progress(msg: str) -> None:
    print(f"[{time.perf_counter() - T0:8.1f}s] {msg}", file=sys.stderr, flush=True)


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a.size else None


def run_batch(N, eng, packed):
    """One end-to-end pass: (seconds end to end, seconds of the run, result, outputs)."""
    rows, cols, flat, nv = packed
    count = len(rows)
    out = dict(status=np.zeros(count, dtype=np.int32), found=np.zeros(count, dtype=np.int32),
               processed=np.zeros(count, dtype=np.int64),
               best_node=np.zeros(count, dtype=np.int32), z=np.zeros(count),
               pivots=np.zeros(count, dtype=np.int64),
               nodes_created=np.zeros(count, dtype=np.int64),
               x=np.zeros(max(int(nv.sum()), 1)))
    h = C.c_void_p()
    opts = N.BBBatchOpts(enable_pruning=0, chunk=0, variant=0, max_child_pivots=0)
    res = N.BBBatchResult()
    eng.sync()
    t0 = time.perf_counter()
    N.check(N.lib.lpr_bb_batch_create(eng._h, count, ptr(rows, C.c_int32), ptr(cols, C.c_int32),
                                      ptr(flat, C.c_double), ptr(nv, C.c_int32), NODE_CAP,
                                      TRACE_CAP, C.byref(h)), "lpr_bb_batch_create")
    t1 = time.perf_counter()
    N.check(N.lib.lpr_bb_batch_run(h, C.byref(opts), C.byref(res)), "lpr_bb_batch_run")
    t2 = time.perf_counter()
    N.check(N.lib.lpr_bb_batch_result_read(
        h, ptr(out["status"], C.c_int32), ptr(out["found"], C.c_int32),
        ptr(out["processed"], C.c_int64), ptr(out["best_node"], C.c_int32),
        ptr(out["z"], C.c_double), ptr(out["pivots"], C.c_int64),
        ptr(out["nodes_created"], C.c_int64)), "lpr_bb_batch_result_read")
    N.check(N.lib.lpr_bb_batch_solution_read(h, ptr(out["x"], C.c_double)),
            "lpr_bb_batch_solution_read")
    eng.sync()
    t3 = time.perf_counter()
    out["h"] = h
    return t3 - t0, t2 - t1, res, out


def run_narrated(N, eng, packed):
    """One narrated end-to-end pass: (seconds end to end, seconds of the second run, result,
    info arrays, the slab, the handle)."""
    rows, cols, flat, nv = packed
    count = len(rows)
    h = C.c_void_p()
    opts = N.BBBatchOpts(enable_pruning=0, chunk=0, variant=0, max_child_pivots=0)
    res = N.BBBatchResult()
    need, kept, off = (np.zeros(count, dtype=np.int64) for _ in range(3))
    eng.sync()
    t0 = time.perf_counter()
    N.check(N.lib.lpr_bb_batch_create(eng._h, count, ptr(rows, C.c_int32), ptr(cols, C.c_int32),
                                      ptr(flat, C.c_double), ptr(nv, C.c_int32), NODE_CAP,
                                      TRACE_CAP, C.byref(h)), "lpr_bb_batch_create")
    N.check(N.lib.lpr_bb_batch_narrate_reserve(h, ptr(need, C.c_int64)), "narrate_reserve")
    N.check(N.lib.lpr_bb_batch_run(h, C.byref(opts), C.byref(res)), "lpr_bb_batch_run")
    N.check(N.lib.lpr_bb_batch_narrate_info(h, None, ptr(need, C.c_int64), None, None),
            "narrate_info")
    N.check(N.lib.lpr_bb_batch_narrate_reserve(h, ptr(need, C.c_int64)), "narrate_reserve")
    t1 = time.perf_counter()
    N.check(N.lib.lpr_bb_batch_run(h, C.byref(opts), C.byref(res)), "lpr_bb_batch_run")
    t2 = time.perf_counter()
    N.check(N.lib.lpr_bb_batch_narrate_info(h, None, None, ptr(kept, C.c_int64),
                                            ptr(off, C.c_int64)), "narrate_info")
    slab = np.empty(max(int(need.sum()), 1))
    N.check(N.lib.lpr_bb_batch_narrate_read_all(h, ptr(slab, C.c_double), slab.size),
            "narrate_read_all")
    eng.sync()
    t3 = time.perf_counter()
    return t3 - t0, t2 - t1, res, dict(need=need, kept=kept, off=off), slab, h


def gather_loop(pkg, eng, roots, nvars, budget_s: float, skip):
    """The single-handle number gathering (no formatting) on a timed prefix; the numbers of the
    first CHECK IPs are kept for the record check."""
    from lpr_381_group_v22_amd.branch_and_bound import gather_branch_and_bound_numbers
    done, kept = 0, {}
    t0 = time.perf_counter()
    while done < len(roots) and (time.perf_counter() - t0 < budget_s or done < CHECK):
        if not skip[done]:
            tree = pkg.BranchBoundTree.from_array(eng, roots[done], nvars[done],
                                                  max_depth=NODE_CAP)
            got = gather_branch_and_bound_numbers(tree, roots[done].shape, False, NODE_CAP)
            tree.destroy()
            if done < CHECK:
                kept[done] = got
        done += 1
    dt = time.perf_counter() - t0
    return dict(ips=done, seconds=dt, ips_per_s=done / dt), kept


def narr_check(bb, want) -> int:
    """IPs whose narrated records differ from the single-handle loop's numbers in any bit."""
    def same(a, b):
        return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()
    bad = 0
    for k, (pops, tab, capped) in want.items():
        got, gtab, gcapped = bb.NarrationNumbers(k)
        ok = gcapped == capped and len(got) == len(pops) and (gtab is None) == (tab is None)
        ok = ok and (tab is None or same(gtab, tab))
        for g, w in zip(got, pops) if ok else ():
            ok = ok and same(g.z, w.z) and same(g.vals, w.vals)
            ok = ok and (g.children is None) == (w.children is None)
            for cg, cw in zip(g.children or [], w.children or []):
                ok = ok and cg.status == cw.status and cg.pivots == cw.pivots
                ok = ok and len(cg.tableaux) == len(cw.tableaux)
                ok = ok and all(same(a, b) for a, b in zip(cg.tableaux, cw.tableaux))
        bad += 0 if ok else 1
    return bad


def narrate_workload(pkg, N, eng, name, roots, nvars, packed, args):
    from lpr_381_group_v22_amd.bb_batch import BranchAndBoundBatch, node_cap_of
    count = len(roots)
    plain, narr = [], []
    for _ in range(max(1, args.repeat)):  # alternated, in one process
        e2e, run, res, out = run_batch(N, eng, packed)
        N.lib.lpr_bb_batch_destroy(out.pop("h"))
        plain.append((e2e, run))
        if narr:
            N.lib.lpr_bb_batch_destroy(narr[-1][5])
        narr.append(run_narrated(N, eng, packed))
        progress(f"{name}: plain e2e {e2e:.4f}s run {run:.4f}s; narrated e2e {narr[-1][0]:.4f}s "
                 f"run {narr[-1][1]:.4f}s")
    e2e, run, res, info, slab, h = narr[-1]
    a = min(r[0] for r in narr)
    skip = np.zeros(count, dtype=bool)
    st = np.zeros(count, dtype=np.int32)
    N.check(N.lib.lpr_bb_batch_result_read(h, ptr(st, C.c_int32), None, None, None, None, None,
                                           None), "lpr_bb_batch_result_read")
    skip = st == N.LPR_PIVOT_LIMIT
    rec = dict(workload=name, mode="narrate", ips=count, node_cap=NODE_CAP,
               pops=int(res.pops), pivots=int(res.pivots), launches=res.launches,
               slab_doubles=int(info["need"].sum()), slab_gb=8e-9 * float(info["need"].sum()),
               kept_all=bool((info["kept"] == info["need"]).all()),
               a_narrated_e2e_seconds=a, a_narrated_e2e_all=[r[0] for r in narr],
               a1_narrated_run_seconds=min(r[1] for r in narr),
               a1_narrated_run_all=[r[1] for r in narr],
               b_plain_e2e_seconds=min(r[0] for r in plain), b_plain_e2e_all=[r[0] for r in plain],
               b_plain_run_seconds=min(r[1] for r in plain), b_plain_run_all=[r[1] for r in plain],
               pivot_limit_ips_skipped=int(skip.sum()))
    if not args.no_check:
        loop, want = gather_loop(pkg, eng, roots, nvars, args.single_seconds, skip)
        c = loop["seconds"] * count / loop["ips"]
        rec["c_single_gather"] = dict(loop, whole_workload_seconds=c,
                                      extrapolated=loop["ips"] < count)
        rec["speedup_c_over_a"] = c / a
        bb = BranchAndBoundBatch(h, eng, zip(packed.rows.tolist(), packed.cols.tolist()),
                                 packed.nvars, node_cap_of(NODE_CAP), TRACE_CAP)
        bb._caps = info["need"]
        checked = {k: v for k, v in want.items() if _whole(bb, k)}
        rec["records_checked"] = len(checked)
        rec["record_mismatches"] = narr_check(bb, checked)
        bb._h = None  # the handle is destroyed below
    N.lib.lpr_bb_batch_destroy(h)
    return rec


def device_text_workload(pkg, N, eng, name, packed, args):
    """--narrate --device-text: one narrated batch, then (a), (b), (c) and the comparison of the
    module docstring on that handle."""
    from lpr_381_group_v22_amd.bb_batch import BranchAndBoundBatch, node_cap_of
    count = len(packed.rows)
    _, run_s, res, info, slab, h = run_narrated(N, eng, packed)
    del slab
    bb = BranchAndBoundBatch(h, eng, zip(packed.rows.tolist(), packed.cols.tolist()), packed.nvars,
                             node_cap_of(NODE_CAP), TRACE_CAP)
    bb.Narrated, bb._caps = True, info["need"]
    progress(f"{name}: narrated run {run_s:.4f}s, slab {8e-9 * float(info['need'].sum()):.3f} GB")

    def call_pass():
        bb._drop_narration_text()
        eng.sync()
        t0 = time.perf_counter()
        text, _ = bb.FormatNarration()
        return text.KernelMs, time.perf_counter() - t0, text.Count, text.Bytes

    def e2e_pass():
        bb._drop_narration_text()
        eng.sync()
        t0 = time.perf_counter()
        done = refused = chars = 0
        for k in range(count):
            try:
                chars += len(bb.NarrationTextDevice(k))
                done += 1
            except ValueError:  # a short trace or LPR_PIVOT_LIMIT: the host path refuses it too
                refused += 1
        return done, refused, chars, time.perf_counter() - t0

    call_pass()  # warm-up
    calls = [call_pass() for _ in range(max(1, args.repeat))]
    progress(f"{name}: (a) kernel_ms {[round(c[0], 3) for c in calls]}")
    e2e = [e2e_pass() for _ in range(max(1, args.repeat))]
    progress(f"{name}: (b) e2e seconds {[round(e[3], 3) for e in e2e]} for {e2e[0][0]} IPs")
    picks = np.linspace(0, count - 1, min(CHECK, count)).astype(np.int64)
    np.random.RandomState(args.seed).shuffle(picks)
    host, texts = [], {}
    for _ in range(max(1, args.repeat)):
        done = 0
        t0 = time.perf_counter()
        for k in picks:
            try:
                texts[int(k)] = bb.NarrationText(int(k))
                done += 1
            except ValueError:
                pass
            if time.perf_counter() - t0 > args.host_seconds:
                break
        host.append((done, time.perf_counter() - t0))
        progress(f"{name}: (c) host pass: {done} IPs in {host[-1][1]:.2f}s")
    t0 = time.perf_counter()
    for k in picks:  # more IPs for the comparison, while the budget lasts
        if time.perf_counter() - t0 > args.check_seconds:
            break
        if int(k) not in texts:
            try:
                texts[int(k)] = bb.NarrationText(int(k))
            except ValueError:
                pass
    bad = sum(bb.NarrationTextDevice(k) != t for k, t in texts.items())
    progress(f"{name}: compared {len(texts)} IPs, {bad} mismatches")
    dev_per_ip = max(e[3] / max(e[0], 1) for e in e2e)
    host_per_ip = min(t / max(d, 1) for d, t in host)
    rec = dict(workload=name, mode="narrate-device-text", ips=count, node_cap=NODE_CAP,
               rows=[int(packed.rows.min()), int(packed.rows.max())],
               cols=[int(packed.cols.min()), int(packed.cols.max())],
               slab_doubles=int(info["need"].sum()), slab_gb=8e-9 * float(info["need"].sum()),
               kept_all=bool((info["kept"] == info["need"]).all()),
               blocks=int(calls[0][2]), text_bytes=int(calls[0][3]),
               a_kernel_ms_all=[c[0] for c in calls], a_call_seconds_all=[c[1] for c in calls],
               a_cells_per_s_kernel=float(info["need"].sum()) / (min(c[0] for c in calls) / 1e3),
               b_e2e_ips_refused_chars_seconds_all=e2e,
               b_device_seconds_per_ip_slowest=dev_per_ip,
               c_host_ips_seconds_all=host, c_host_seconds_per_ip_fastest=host_per_ip,
               c_host_seconds_whole_workload_extrapolated=host_per_ip * count,
               speedup_per_ip=host_per_ip / dev_per_ip, clears_bar=bool(dev_per_ip < host_per_ip),
               ips_compared=len(texts), mismatches=int(bad))
    bb.destroy()
    return rec


def _whole(bb, k) -> bool:
    """IP k keeps its whole trace (TRACE_CAP quads): its numbers can be rebuilt."""
    return bb.Result(k)["pivots"] <= bb.trace_cap


def single_loop(pkg, eng, roots, nvars, budget_s: float, skip):
    done = pops = pivots = 0
    t0 = time.perf_counter()
    while done < len(roots) and time.perf_counter() - t0 < budget_s:
        if skip[done]:
            done += 1
            continue
        tree = pkg.BranchBoundTree.from_array(eng, roots[done], nvars[done], max_depth=NODE_CAP)
        r, _ = tree.run(enable_pruning=False, node_cap=NODE_CAP)
        tree.destroy()
        pops += int(r.processed)
        pivots += int(r.pivots)
        done += 1
    dt = time.perf_counter() - t0
    return dict(ips=done, seconds=dt, ips_per_s=done / dt, pops_per_s=pops / dt,
                pivots_per_s=pivots / dt)


def oracle_loop(orc, roots, nvars, budget_s: float, skip):
    done = pops = pivots = 0
    t0 = time.perf_counter()
    while done < len(roots) and time.perf_counter() - t0 < budget_s:
        if skip[done]:
            done += 1
            continue
        r = orc.bb_solve(roots[done], nvars[done], node_cap=NODE_CAP, rec_cap=64,
                         piv_cap=TRACE_CAP)
        pops += r["processed"]
        done += 1
    dt = time.perf_counter() - t0
    return dict(ips=done, seconds=dt, ips_per_s=done / dt, pops_per_s=pops / dt)


def bit_check(N, orc, roots, nvars, out, skip) -> int:
    """IPs among the first CHECK that differ from the oracle in any output."""
    h = out["h"]
    bad = 0
    at = 0
    for k in range(min(CHECK, len(roots))):
        nv = nvars[k]
        if skip[k]:
            at += nv
            continue
        ref = orc.bb_solve(roots[k], nv, node_cap=NODE_CAP, piv_cap=1 << 16)
        ok = (out["status"][k] == ref["status"] and bool(out["found"][k]) == ref["found"]
              and out["processed"][k] == ref["processed"]
              and out["best_node"][k] == ref["best_node"]
              and np.float64(out["z"][k]).tobytes() == np.float64(ref["z"]).tobytes()
              and out["pivots"][k] == len(ref["trace"])
              and out["nodes_created"][k] == len(ref["records"]))
        xk = out["x"][at:at + nv]
        ok = ok and (xk.tobytes() == np.asarray(ref["x"], dtype=np.float64).tobytes()
                     if ref["found"] else not np.any(xk))
        cap = 1 + 2 * NODE_CAP
        p, kd, d, v, s = (np.zeros(cap, dtype=np.int32) for _ in range(5))
        b, z = np.zeros(cap), np.zeros(cap)
        n = C.c_int64()
        N.check(N.lib.lpr_bb_batch_records_read(h, k, ptr(p, C.c_int32), ptr(kd, C.c_int32),
                                                ptr(d, C.c_int32), ptr(v, C.c_int32),
                                                ptr(b, C.c_double), ptr(s, C.c_int32),
                                                ptr(z, C.c_double), cap, C.byref(n)),
                "lpr_bb_batch_records_read")
        recs = [(int(p[i]), int(kd[i]), int(d[i]), int(v[i]), np.float64(b[i]).tobytes(),
                 int(s[i]), np.float64(z[i]).tobytes()) for i in range(n.value)]
        want = [(r["parent"], r["kind"], r["depth"], r["var"], np.float64(r["bound"]).tobytes(),
                 r["status"], np.float64(r["z"]).tobytes()) for r in ref["records"]]
        ok = ok and recs == want
        ids = np.zeros(NODE_CAP, dtype=np.int32)
        N.check(N.lib.lpr_bb_batch_pop_order_read(h, k, ptr(ids, C.c_int32), NODE_CAP,
                                                  C.byref(n)), "lpr_bb_batch_pop_order_read")
        ok = ok and ids[:n.value].tolist() == ref["pop_order"]
        q = np.zeros(4 * TRACE_CAP, dtype=np.int32)
        N.check(N.lib.lpr_bb_batch_trace_read(h, k, ptr(q, C.c_int32), TRACE_CAP, C.byref(n)),
                "lpr_bb_batch_trace_read")
        got = [tuple(t) for t in q[:4 * n.value].reshape(-1, 4).tolist()]
        ok = ok and got == [tuple(t) for t in ref["trace"][:TRACE_CAP]]
        bad += 0 if ok else 1
        at += nv
    return bad


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="W,G,H")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--single-seconds", type=float, default=5.0)
    ap.add_argument("--oracle-seconds", type=float, default=5.0)
    ap.add_argument("--no-check", action="store_true", help="skip the bit check and the loops")
    ap.add_argument("--narrate", action="store_true", help="measure the narrated batch")
    ap.add_argument("--ips", type=int, default=0, help="keep the first N IPs of each workload")
    ap.add_argument("--device-text", action="store_true",
                    help="with --narrate: measure the device text of the narrated batch")
    ap.add_argument("--text-ips", default="W=2048,G=512,H=32",
                    help="--device-text: IPs kept per workload")
    ap.add_argument("--host-seconds", type=float, default=4.0, help="budget of one host pass")
    ap.add_argument("--check-seconds", type=float, default=45.0,
                    help="--device-text: host formatting spent on further IPs to compare")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.bb_batch import pack_roots
    orc = None
    if not args.no_check:
        from oracle_lib import Oracle
        orc = Oracle()
    failures = 0
    lines = []
    text_ips = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in args.text_ips.split(","))
    if args.device_text:
        if not args.narrate:
            ap.error("--device-text goes with --narrate")
        args.out = args.out or os.path.join(ROOT, "profiles", "bb_batch_narr_text_bench.json")
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            progress(f"{name}: generating")
            limit = args.ips if args.ips > 0 else (text_ips.get(name, 0) if args.device_text
                                                   else 0)
            models = gen_models(name, args.seed + i, limit)
            progress(f"{name}: primal batch")
            roots, nvars = roots_of(pkg, N, eng, models)
            packed = pack_roots(roots, nvars, NODE_CAP)
            if args.device_text:
                rec = device_text_workload(pkg, N, eng, name, packed, args)
                failures += rec["mismatches"]
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
                continue
            if args.narrate:
                rec = narrate_workload(pkg, N, eng, name, roots, nvars, packed, args)
                failures += rec.get("record_mismatches", 0)
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
                continue
            count = len(roots)
            forms = {f: 0 for f in "WGH"}
            for T in roots:
                forms[form_of(T)] += 1
            runs = []
            for _ in range(max(1, args.repeat)):
                if runs:  # only the last handle is kept (for the bit check)
                    N.lib.lpr_bb_batch_destroy(runs[-1][3].pop("h"))
                runs.append(run_batch(N, eng, packed))
                progress(f"{name}: run {len(runs)}: e2e {runs[-1][0]:.4f}s, run {runs[-1][1]:.4f}s")
            best_e2e = min(r[0] for r in runs)
            best_run = min(r[1] for r in runs)
            res, out = runs[-1][2], runs[-1][3]
            pops, pivots = int(res.pops), int(res.pivots)
            rec = dict(workload=name, ips=count,
                       rows=[int(packed.rows.min()), int(packed.rows.max())],
                       cols=[int(packed.cols.min()), int(packed.cols.max())],
                       node_cap=NODE_CAP, forms=forms, pops=pops, pivots=pivots,
                       done=res.done, node_capped=res.node_cap, pivot_limit=res.pivot_limit,
                       found=int(out["found"].sum()), launches=res.launches,
                       e2e_seconds=best_e2e, e2e_ips_per_s=count / best_e2e,
                       e2e_pops_per_s=pops / best_e2e, e2e_pivots_per_s=pivots / best_e2e,
                       run_seconds=best_run, run_ips_per_s=count / best_run,
                       run_pops_per_s=pops / best_run, run_pivots_per_s=pivots / best_run,
                       e2e_seconds_all=[r[0] for r in runs],
                       run_seconds_all=[r[1] for r in runs])
            if not args.no_check:
                # an IP whose child LP hit the pivot limit cycles: the oracle, like the C#, would
                # never return from it, so the loops and the check pass over those IPs
                skip = out["status"] == N.LPR_PIVOT_LIMIT
                rec["pivot_limit_ips_skipped_by_loops"] = int(skip.sum())
                bad = bit_check(N, orc, roots, nvars, out, skip)
                progress(f"{name}: bit check, {bad} mismatches")
                rec["bit_checked"] = min(CHECK, count) - int(skip[:CHECK].sum())
                rec["bit_mismatches"] = bad
                failures += bad
                rec["single_handle"] = single_loop(pkg, eng, roots, nvars, args.single_seconds,
                                                    skip)
                progress(f"{name}: single-handle loop done")
                rec["cpu_oracle_1core"] = oracle_loop(orc, roots, nvars, args.oracle_seconds,
                                                      skip)
                rec["speedup_e2e_vs_single"] = rec["e2e_ips_per_s"] / \
                    rec["single_handle"]["ips_per_s"]
                rec["speedup_e2e_vs_oracle"] = rec["e2e_ips_per_s"] / \
                    rec["cpu_oracle_1core"]["ips_per_s"]
            N.lib.lpr_bb_batch_destroy(runs[-1][3]["h"])
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.device_text:
        recs = [json.loads(x) for x in lines]
        lines.append(json.dumps(dict(mode="summary", text_ips=args.text_ips,
                                     clears_bar=all(r["clears_bar"] for r in recs),
                                     mismatches=sum(r["mismatches"] for r in recs),
                                     ips_compared=sum(r["ips_compared"] for r in recs))))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"bit check: {failures} IP(s) differ from the oracle", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
