"""Measures the knapsack batch and prints one JSON line per workload:

  S   65536 instances of 6-10 items, weights and values <= 20, node_cap 200 (form W)
  M   4096 strongly-correlated instances of n = 40 (v = w + 100, w <= 1000), node_cap 4096
  L   256 strongly-correlated instances of n = 200, node_cap 20000 (form H)

Per workload: instances/s end to end (lpr_knap_batch_create, lpr_knap_batch_solve, the bulk reads
of the results, the ranks and the selected items, closed by an engine sync), for the solve alone
and for lpr_knap_batch_dp alone (--repeat passes after one warm-up pass, every one recorded);
launches and nodes/s; the same instances one at a time through KnapsackBranchBoundSimplex (same
node cap, no narration) + SelectedIds + knapsack_dp in a Python loop (a time-bounded prefix, then
the same prefix again for --repeat passes in all); the restatement (tests/ref_py_knapsack.py, its
DP as one numpy row operation per item) on one core.  --check instances per workload (evenly
spaced) are solved again in a narrated batch and compared with the restatement record by record
(bounds by bits), and their DP values with that DP; any mismatch makes the exit status non-zero.
Inputs are seeded.

`clears_bar` says whether the batch's slowest pass (end to end plus the DP call), per instance,
is below the loop's fastest pass, per instance.

Run it under a time limit:  timeout -k 10 900 python tools/knapsack_batch_bench.py --out
profiles/knapsack_batch_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import random
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COUNTS = {"S": 65536, "M": 4096, "L": 256}
CAPS = {"S": 200, "M": 4096, "L": 20000}
CHECK_RECORDS = 4096


def gen_workload(name: str, seed: int):
    """(capacity, weights, values) per instance."""
    rng = random.Random(seed)
    out = []
    for _ in range(COUNTS[name]):
        if name == "S":
            n = rng.randint(6, 10)
            w = [rng.randint(1, 20) for _ in range(n)]
            v = [rng.randint(1, 20) for _ in range(n)]
        else:
            n = 40 if name == "M" else 200
            w = [rng.randint(1, 1000) for _ in range(n)]
            v = [x + 100 for x in w]
        out.append((sum(w) // 2, w, v))
    return out


def make(pkg, eng, inst, cap, narrate=0):
    return pkg.KnapsackBatch([c for c, _, _ in inst], [w for _, w, _ in inst],
                             [v for _, _, v in inst], node_cap=cap, narrate=narrate, engine=eng)


def run_batch(pkg, eng, inst, cap):
    """One pass: (seconds end to end, seconds of the solve, seconds of the DP, result, batch)."""
    eng.sync()
    t0 = time.perf_counter()
    b = make(pkg, eng, inst, cap)
    t1 = time.perf_counter()
    res = b.Solve()
    t2 = time.perf_counter()
    b.Stats()
    b.Rank()
    b.SelectedIds()
    eng.sync()
    t3 = time.perf_counter()
    b.DP()
    t4 = time.perf_counter()
    return t3 - t0, t2 - t1, t4 - t3, res, b


def single_pass(pkg, eng, inst, cap, budget_s=None, items=None):
    done = 0
    t0 = time.perf_counter()
    while done < len(inst) and (done < items if items is not None
                                else time.perf_counter() - t0 < budget_s):
        C, w, v = inst[done]
        s = pkg.KnapsackBranchBoundSimplex(C, w, v, engine=eng, node_cap=cap, narrate=0)
        s.Solve()
        s.SelectedIds()
        s.destroy()
        pkg.knapsack.knapsack_dp(C, w, v, engine=eng)
        done += 1
    return done, time.perf_counter() - t0


def single_loop(pkg, eng, inst, cap, budget_s: float, repeat: int):
    done, dt = single_pass(pkg, eng, inst, cap, budget_s=budget_s)
    secs = [dt] + [single_pass(pkg, eng, inst, cap, items=done)[1] for _ in range(repeat - 1)]
    best = min(secs)
    return dict(items=done, seconds=best, items_per_s=done / best, seconds_all=secs)


def dp_numpy(C: int, w, v) -> int:
    """The DP rule of DESIGN.md section 11 on one int64 numpy row (exact)."""
    import numpy as np
    row = np.zeros(C + 1, dtype=np.int64)
    for wj, vj in zip(w, v):
        if wj <= C:
            row[wj:] = np.maximum(row[wj:], row[:C + 1 - wj] + vj)
    return int(row[C])


def check(pkg, eng, inst, cap, n_check: int):
    """The restatement on one core over n_check evenly spaced instances (timed), and the batch
    against it record by record.  Returns (mismatches, checked, restatement record)."""
    import ref_py_knapsack as K
    step = max(1, len(inst) // n_check)
    picks = list(range(0, len(inst), step))[:n_check]
    sub = [inst[k] for k in picks]
    t0 = time.perf_counter()
    refs = [K.branch_and_bound(C, w, v, node_cap=cap) for C, w, v in sub]
    t1 = time.perf_counter()
    dps = [dp_numpy(C, w, v) for C, w, v in sub]
    t2 = time.perf_counter()
    b = make(pkg, eng, sub, cap, narrate=CHECK_RECORDS)
    b.Solve()
    s, sel, rank, dp = b.Stats(), b.SelectedIds(), b.Rank(), b.DP()
    bad = 0
    for k, r in enumerate(refs):
        want = [(p, br, st, struct.pack("<d", bd), r["rank"][kk] if kk >= 0 else -1, V)
                for p, br, st, bd, kk, V in r["records"][:CHECK_RECORDS]]
        got = [(nd.parent, nd.branch, nd.status, struct.pack("<d", nd.bound), nd.k, nd.V)
               for nd in b.Nodes(k)]
        ok = (int(s["status"][k]) == r["status"] and int(s["evaluated"][k]) == r["evaluated"] and
              int(s["levels"][k]) == r["levels"] and int(s["widest"][k]) == r["widest"] and
              float(s["z"][k]) == float(r["z"] or 0) and sel[k] == r["selected"] and
              rank[k] == r["rank"] and got == want and dp[k] == dps[k])
        bad += not ok
    b.destroy()
    cpu = dict(items=len(sub), bb_seconds=t1 - t0, dp_seconds=t2 - t1,
               items_per_s=len(sub) / (t2 - t0))
    return bad, len(sub), cpu


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S,M,L")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--single-seconds", type=float, default=4.0)
    ap.add_argument("--check", type=int, default=256, help="instances compared per workload")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison and the loops")
    ap.add_argument("--out", default=None,
                    help="also append the JSON lines to this file (the committed record is "
                         "profiles/knapsack_batch_bench.json)")
    args = ap.parse_args()

    import lpr_381_group_v22_amd as pkg
    failures = 0
    lines = []
    repeat = max(1, args.repeat)
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            inst = gen_workload(name, args.seed + 1000 * i)
            cap = CAPS[name]
            run_batch(pkg, eng, inst, cap)[4].destroy()  # warm-up
            runs = [run_batch(pkg, eng, inst, cap) for _ in range(repeat)]
            res = runs[-1][3]
            count = len(inst)
            e2e, solve, dp = ([r[q] for r in runs] for q in range(3))
            med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
            rec = dict(workload=name, instances=count, n=[min(len(w) for _, w, _ in inst),
                                                          max(len(w) for _, w, _ in inst)],
                       node_cap=cap, items_w=res.items_w, items_g=res.items_g,
                       items_h=res.items_h, finished=res.finished, capped=res.capped,
                       launches=res.launches, nodes=int(res.nodes),
                       e2e_seconds=med(e2e), e2e_instances_per_s=count / med(e2e),
                       solve_seconds=med(solve), solve_nodes_per_s=int(res.nodes) / med(solve),
                       dp_seconds=med(dp), dp_instances_per_s=count / med(dp),
                       e2e_seconds_all=e2e, solve_seconds_all=solve, dp_seconds_all=dp)
            for r in runs:
                r[4].destroy()
            if not args.no_check:
                bad, checked, cpu = check(pkg, eng, inst, cap, args.check)
                rec["checked"] = checked
                rec["mismatches"] = bad
                failures += bad
                rec["restatement_1core"] = cpu
                one = single_loop(pkg, eng, inst, cap, args.single_seconds, repeat)
                rec["single_handle"] = one
                both = [a + b for a, b in zip(e2e, dp)]
                rec["speedup_vs_single"] = (count / med(both)) / one["items_per_s"]
                rec["speedup_vs_restatement"] = (count / med(both)) / cpu["items_per_s"]
                rec["clears_bar"] = bool(max(both) / count < min(one["seconds_all"]) / one["items"])
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"check: {failures} instance(s) differ from the restatement", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
