"""Measures the cutting-plane batch and prints one JSON line per workload:

  S   65536 textbook tableaux: the final tableaux of LPs drawn from the bb_cases generators
      (random_binary_program / fractional_program, 512 distinct ones, cycled), max_cuts 6
  G   4096 x side_base(40, 60, seed), max_cuts 8: form G
  H   256 x side_base(200, 40, seed), max_cuts 12: form H

Per workload: items/s end to end (lpr_cut_batch_create, lpr_cut_batch_run, the bulk reads of
code / cuts / rows / log counts / z, closed by an engine sync) and for lpr_cut_batch_run alone
(--repeat passes after one warm-up pass, every one recorded); launches, cuts and pivots; the same
items one at a time through Tableau.from_array + cutting_plane + read + destroy in a Python loop
(a time-bounded prefix, then the same prefix again for --repeat passes in all); the CPU oracle on
one core (a prefix).  256 items per workload (evenly spaced) are checked against the oracle bit for
bit (exit code, cuts, log, shape, tableau); any mismatch makes the exit status non-zero.  Inputs
are seeded.

`clears_bar` says whether the batch's slowest end-to-end pass, per item, is below the loop's
fastest pass, per item: the comparison holds by more than the spread of the repetitions.

Run it under a time limit:  timeout -k 10 900 python tools/cut_batch_bench.py --out
profiles/cut_batch_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

CHECK = 256
HARD_CAP = 2000
COUNTS = {"S": 65536, "G": 4096, "H": 256}
MAX_CUTS = {"S": 6, "G": 8, "H": 12}
S_DISTINCT = 512


def gen_workload(orc, name: str, seed: int):
    """The tableaux of one workload."""
    import bb_cases
    import cut_cases
    count = COUNTS[name]
    if name == "G":
        return [cut_cases.side_base(40, 60, seed + q) for q in range(count)]
    if name == "H":
        return [cut_cases.side_base(200, 40, seed + q) for q in range(count)]
    rng = np.random.RandomState(seed)
    pool = []
    while len(pool) < S_DISTINCT:
        gen = bb_cases.random_binary_program if rng.randint(0, 2) else bb_cases.fractional_program
        obj, cons = gen(int(rng.randint(3, 11)), int(rng.randint(1, 5)),
                        int(rng.randint(0, 1 << 30)))
        st, T, _ = bb_cases.primal_final_tableau(orc, obj, cons)
        if st == 0:
            pool.append(T)
    return [pool[q % S_DISTINCT] for q in range(count)]


def run_batch(pkg, eng, tabs, max_cuts):
    """One end-to-end pass: (seconds end to end, seconds of the run, result, batch)."""
    eng.sync()
    t0 = time.perf_counter()
    b = pkg.CuttingPlaneBatch.from_arrays(eng, tabs, max_cuts=max_cuts, log_cap=64)
    t1 = time.perf_counter()
    res = b.Run(hard_cap=HARD_CAP)
    t2 = time.perf_counter()
    b.result_arrays()
    eng.sync()
    t3 = time.perf_counter()
    return t3 - t0, t2 - t1, res, b


def single_pass(Tableau, eng, tabs, max_cuts, budget_s=None, items=None):
    """The loop over a prefix: bounded by time (budget_s) or by count (items)."""
    done = 0
    t0 = time.perf_counter()
    while done < len(tabs) and (done < items if items is not None
                                else time.perf_counter() - t0 < budget_s):
        tab = Tableau.from_array(eng, tabs[done])
        tab.cutting_plane(max_cuts=max_cuts, hard_cap=HARD_CAP)
        tab.read()
        tab.destroy()
        done += 1
    return done, time.perf_counter() - t0


def single_loop(Tableau, eng, tabs, max_cuts, budget_s: float, repeat: int):
    done, dt = single_pass(Tableau, eng, tabs, max_cuts, budget_s=budget_s)
    secs = [dt] + [single_pass(Tableau, eng, tabs, max_cuts, items=done)[1]
                   for _ in range(repeat - 1)]
    best = min(secs)
    return dict(items=done, seconds=best, items_per_s=done / best, seconds_all=secs)


def oracle_loop(orc, tabs, max_cuts, budget_s: float):
    done = 0
    t0 = time.perf_counter()
    while done < len(tabs) and time.perf_counter() - t0 < budget_s:
        orc.cutting_plane(tabs[done], max_cuts=max_cuts, hard_cap=HARD_CAP)
        done += 1
    dt = time.perf_counter() - t0
    return dict(items=done, seconds=dt, items_per_s=done / dt)


def bit_check(orc, tabs, max_cuts, batch) -> int:
    """Items among CHECK evenly spaced ones that differ from the oracle in any output."""
    bad = 0
    res = batch.result_arrays()
    step = max(1, len(tabs) // CHECK)
    for k in list(range(0, len(tabs), step))[:CHECK]:
        rc, cuts, T, log = orc.cutting_plane(tabs[k], max_cuts=max_cuts, hard_cap=HARD_CAP)
        got = batch.Tableau(k)
        ok = (int(res["code"][k]), int(res["cuts"][k])) == (rc, cuts) and \
            int(res["log_count"][k]) == len(log) and \
            batch.Log(k) == [tuple(t) for t in log][:batch.LogCap(k)] and \
            got.shape == T.shape and got.tobytes() == T.tobytes()
        bad += not ok
    return bad


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S,G,H")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--single-seconds", type=float, default=4.0)
    ap.add_argument("--oracle-seconds", type=float, default=4.0)
    ap.add_argument("--no-check", action="store_true", help="skip the bit check and the loops")
    ap.add_argument("--out", default=None,
                    help="also append the JSON lines to this file (the committed record is "
                         "profiles/cut_batch_bench.json; never pass it to a profiled run)")
    args = ap.parse_args()

    import lpr_381_group_v22_amd as pkg
    from oracle_lib import Oracle
    orc = Oracle()  # the LPs behind S are solved on the CPU, outside every timed region
    failures = 0
    lines = []
    repeat = max(1, args.repeat)
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            tabs = gen_workload(orc, name, args.seed + 1000 * i)
            mc = MAX_CUTS[name]
            run_batch(pkg, eng, tabs, mc)[3].destroy()  # warm-up
            runs = [run_batch(pkg, eng, tabs, mc) for _ in range(repeat)]
            best_e2e = min(r[0] for r in runs)
            best_run = min(r[1] for r in runs)
            res, batch = runs[-1][2], runs[-1][3]
            count = len(tabs)
            rec = dict(workload=name, items=count, rows=int(tabs[0].shape[0]),
                       cols=int(tabs[0].shape[1]), max_cuts=mc, hard_cap=HARD_CAP,
                       items_g=res.items_g, items_h=res.items_h, launches=res.launches,
                       cuts=int(res.cuts), pivots=int(res.pivots),
                       exits={str(c): int(res.by_code[c]) for c in range(8) if res.by_code[c]},
                       e2e_seconds=best_e2e, e2e_items_per_s=count / best_e2e,
                       run_seconds=best_run, run_items_per_s=count / best_run,
                       e2e_seconds_all=[r[0] for r in runs],
                       run_seconds_all=[r[1] for r in runs])
            if not args.no_check:
                bad = bit_check(orc, tabs, mc, batch)
                rec["bit_checked"] = min(CHECK, count)
                rec["bit_mismatches"] = bad
                failures += bad
                one = single_loop(pkg.Tableau, eng, tabs, mc, args.single_seconds, repeat)
                rec["single_handle"] = one
                rec["cpu_oracle_1core"] = oracle_loop(orc, tabs, mc, args.oracle_seconds)
                rec["speedup_e2e_vs_single"] = rec["e2e_items_per_s"] / one["items_per_s"]
                rec["speedup_prefix_items"] = one["items"]
                slowest_batch = max(r[0] for r in runs) / count
                fastest_loop = min(one["seconds_all"]) / one["items"]
                rec["clears_bar"] = bool(slowest_batch < fastest_loop)
            for r in runs:
                r[3].destroy()
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"bit check: {failures} item(s) differ from the oracle", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
