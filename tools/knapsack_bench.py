"""Measures menu option 5's device paths and prints one JSON line per run:

  dp      C = 2^24, n = 4096 (w ~ U[1, 2048], v ~ U[1, 1000], numpy default_rng(0)): cell-updates/s
          of the blocked LDS passes (variant 0) and of one streaming pass per item (variant 1)
  bb      the strongly-correlated instance (n = 100, random.seed(3), w ~ randint(1, 1000),
          v = w + 100, C = sum(w) // 2), node_cap = 2^20: nodes/s, levels, widest, time per level
  cpu_*   the CPU restatement (tests/ref_py_knapsack.py, numpy for the DP) on the same work

Run it under a time limit:  timeout -k 10 900 python tools/knapsack_bench.py [--repeat 3]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def dp_instance():
    rng = np.random.default_rng(0)
    return 1 << 24, rng.integers(1, 2049, 4096), rng.integers(1, 1001, 4096)


def bb_instance():
    random.seed(3)
    w = [random.randint(1, 1000) for _ in range(100)]
    return sum(w) // 2, w, [x + 100 for x in w]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement baselines")
    args = ap.parse_args()

    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd.knapsack import KnapsackBranchBoundSimplex, knapsack_dp
    import ref_py_knapsack as K

    eng = pkg.Engine(0)
    C, w, v = dp_instance()
    cells = int(sum(C + 1 - int(x) for x in w if x <= C))  # cells an item actually updates
    knapsack_dp(C, w[:64], v[:64], engine=eng)  # warm-up: module load, first allocations
    results = {}
    for variant, name in ((0, "blocked"), (1, "streamed")):
        times, best = [], None
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            got = knapsack_dp(C, w, v, engine=eng, variant=variant)
            times.append(time.perf_counter() - t0)
            assert best is None or got == best
            best = got
        t = statistics.median(times)
        results[name] = best
        print(json.dumps({"run": "dp", "form": name, "C": C, "n": len(w), "best": best,
                          "seconds_median": t, "seconds_all": times,
                          "cell_updates": cells, "cell_updates_per_s": cells / t,
                          # streamed: 8 B read (the c - w read hits in cache) + 8 B written per cell
                          "hbm_bytes_per_s_if_16B_per_cell": 16 * cells / t}), flush=True)
    assert results["blocked"] == results["streamed"]

    Cb, wb, vb = bb_instance()
    cap = 1 << 20
    runs = []
    for _ in range(args.repeat):
        s = KnapsackBranchBoundSimplex(Cb, wb, vb, engine=eng, node_cap=cap, narrate=0)
        t0 = time.perf_counter()
        s.Solve()
        runs.append((time.perf_counter() - t0, s.Z, s.Status, s.Evaluated, s.Levels, s.Widest))
        s.destroy()
    t = statistics.median(r[0] for r in runs)
    _, z, st, ev, lv, wd = runs[0]
    print(json.dumps({"run": "bb", "n": len(wb), "C": Cb, "node_cap": cap, "status": st, "z": z,
                      "evaluated": ev, "levels": lv, "widest": wd, "seconds_median": t,
                      "seconds_all": [r[0] for r in runs], "nodes_per_s": ev / t,
                      "seconds_per_level": t / max(lv, 1)}), flush=True)

    if not args.no_cpu:
        t0 = time.perf_counter()
        r = K.branch_and_bound(Cb, wb, vb, node_cap=cap, records=False)
        tc = time.perf_counter() - t0
        assert (r["z"], r["evaluated"], r["levels"]) == (z, ev, lv)
        print(json.dumps({"run": "cpu_bb", "seconds": tc, "evaluated": r["evaluated"],
                          "nodes_per_s": r["evaluated"] / tc}), flush=True)
        # numpy DP over the first 64 items of the same row, the rate extrapolated to all of them
        row = np.zeros(C + 1, dtype=np.int64)
        t0 = time.perf_counter()
        done = 0
        for a, b in zip(w[:64].tolist(), v[:64].tolist()):
            row[a:] = np.maximum(row[a:], row[:C + 1 - a] + b)
            done += C + 1 - a
        tc = time.perf_counter() - t0
        print(json.dumps({"run": "cpu_dp", "items": 64, "seconds": tc, "cell_updates": done,
                          "cell_updates_per_s": done / tc,
                          "seconds_extrapolated_to_all_items": cells * tc / done}), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
