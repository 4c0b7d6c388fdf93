"""Measures the scenario batch's sensitivity report (lpr_sens_batch_ranging)
on the three workloads of tools/sens_batch_bench.py and prints one JSON line per workload:

  S   65536 scenarios of a solved 8 x 14 LP
  G   4096 scenarios of a solved 33 x 97 LP
  H   256 scenarios of a solved 257 x 769 LP (form H)

Per workload, after the scripts have run: reports/s end to end for one ranging_arrays() call (a
host clock around the call, which ends in a stream synchronise; best and median of --repeat after
one warm-up call); the kernel's time from the call's own events (median); the bytes the kernel
reads from the slabs (each scenario's tableau twice -- the column pass and the row pass -- at
8 R C bytes a pass) over that time as a share of the 8 TB/s HBM peak; the bytes of the output
block the call copies to the host.  The baseline is what the batch offers without the call, per
scenario Tableau(k) -> SensState.create -> ranging() -> destroy in a Python loop over a
time-bounded prefix (`scenarios` in its record).  It is a time baseline only: SensState.create
rebuilds basicVars, so it is not the parity reference.  256 evenly spaced scenarios are checked
against tests/ref_py_ranging.py on the state read back from the batch; any mismatch makes the exit
status non-zero.  Inputs are seeded.

Run it under a time limit:  timeout -k 10 600 python tools/sens_batch_ranging_bench.py --out
profiles/sens_batch_ranging_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

CHECK = 256
HBM_PEAK = 8.0e12
FIELDS = ("kind", "var_row", "reduced_cost", "cost_lo", "cost_hi", "shadow", "rhs_lo", "rhs_hi",
          "rhs_now")
COLUMN_FIELDS = FIELDS[:5]


def same(a, b) -> bool:
    """The parity comparator: NaN positions identical, all other bits identical."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def restatement_check(batch, arr) -> int:
    """Scenarios among CHECK evenly spaced ones whose report differs from the restatement."""
    import ref_py_ranging as ref
    _, _, basic = batch.state_arrays()
    R, C = batch.Rows, batch.Cols
    fn = ref.report_literal if R * C <= 3000 else ref.report_numpy
    step = max(1, batch.Count // CHECK)
    bad = 0
    for k in list(range(0, batch.Count, step))[:CHECK]:
        want = fn(batch.Tableau(k), basic[k].tolist())
        bad += not all(same(getattr(arr, f)[k], want[f]) for f in FIELDS)
    return bad


def loop_baseline(SensState, eng, batch, budget_s: float):
    done = 0
    t0 = time.perf_counter()
    while done < batch.Count and time.perf_counter() - t0 < budget_s:
        T = batch.Tableau(done)
        d = SensState.create(eng, T, np.zeros(T.shape[1] - T.shape[0]), 0.0)
        d.ranging()
        d.destroy()
        done += 1
    dt = time.perf_counter() - t0
    return dict(scenarios=done, seconds=dt, reports_per_s=done / dt)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S,G,H")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--loop-seconds", type=float, default=4.0)
    ap.add_argument("--no-check", action="store_true", help="skip the check and the loop")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd.engine import SensState
    from oracle_lib import Oracle
    from sens_batch_bench import gen_workload
    orc = Oracle()  # the bases are solved on the CPU, outside every timed region
    failures = 0
    lines = []
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            base, scripts = gen_workload(orc, name, args.seed + i)
            T, x, z, _ = base
            d = SensState.create(eng, T, x, z)
            batch = pkg.SensitivityBatch(d, scripts)
            d.destroy()
            res = batch.Run()
            arr = batch.ranging_arrays()  # warm-up: allocates the output block and its mirror
            calls, kernels = [], []
            for _ in range(max(1, args.repeat)):
                eng.sync()
                t0 = time.perf_counter()
                arr = batch.ranging_arrays()
                calls.append(time.perf_counter() - t0)
                kernels.append(batch.RangingTime() * 1e-3)
            count, (R, C) = batch.Count, T.shape
            kernel_s = statistics.median(kernels)
            read_bytes = 2 * 8 * R * C * count
            out_bytes = count * ((C - 1) * (3 * 8 + 2 * 4) + (R - 1) * 4 * 8)
            rec = dict(workload=name, scenarios=count, rows=int(R), cols=int(C),
                       form={1: "G", 2: "H"}[res.form], finished=res.finished,
                       call_seconds_best=min(calls), call_seconds_median=statistics.median(calls),
                       reports_per_s=count / min(calls),
                       kernel_seconds_median=kernel_s, kernel_seconds_min=min(kernels),
                       slab_bytes_read=read_bytes, output_bytes=out_bytes,
                       read_rate_bytes_per_s=read_bytes / kernel_s,
                       share_of_hbm_peak=read_bytes / kernel_s / HBM_PEAK)
            if not args.no_check:
                bad = restatement_check(batch, arr)
                rec["checked"] = min(CHECK, count)
                rec["mismatches"] = bad
                failures += bad
                rec["per_scenario_loop"] = loop_baseline(SensState, eng, batch, args.loop_seconds)
                rec["speedup_vs_loop"] = rec["reports_per_s"] / \
                    rec["per_scenario_loop"]["reports_per_s"]
            batch.destroy()
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"check: {failures} report(s) differ from the restatement", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
