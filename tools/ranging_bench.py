"""Measures the sensitivity report (lpr_sens_ranging) and prints one JSON line
per shape; --out writes them all to one file (the committed record is profiles/ranging_bench.json).

Shapes (rows x cols): 8 x 14, 33 x 97, 257 x 769, 513 x 1537 and the headline 4097 x 12289, on
identity-basis data from a seed: every row basic in a unit column (a structural one, or its own
slack column where there are fewer structural columns than rows), every other column dense in
[-1, 1), reduced costs and right-hand sides of both signs.  The headline shape is also run at
density 0.05 (the other entries are exact zeros, which take no division), to show what the
divisions cost.

Per shape:
  e2e_ms            one SensState.ranging() call end to end, host clock (the call ends in a stream
                    synchronise): warmed up, then repeated for at least --window seconds
  sweep_ms, finish_ms   device time of the two kernels, from the events the call records
                    (lpr_sens_ranging_times), median over the timed calls
  sweep_bytes       m * ld * 8: what the sweep must read (ld = cols rounded up to 16)
  divisions         ieee_div calls of the sweep, counted on the host from the data
  hbm_share         sweep_bytes / sweep time over the 8 TB/s HBM peak
  bound             "HBM" when the sweep runs at half the peak or better, else "ALU/latency"
  loop_ms           the per-index host loop the report replaces: SensitivityAnalyzer.BasicRange for
                    every basic column plus RHSRange for every constraint.  Over all indices at
                    the three smaller shapes; at the two larger ones over a fixed sample of 64
                    basic columns and 64 constraints, scaled (loop_extrapolated: true)
  speedup           loop_ms / e2e_ms
One call per shape is checked against tests/ref_py_ranging.py (numpy formulation) under the parity
comparator; a mismatch makes the exit status non-zero.

Run it under a time limit:  timeout -k 10 600 python tools/ranging_bench.py --out
profiles/ranging_bench.json
Kernel times from a profiler come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR --
python tools/ranging_bench.py --no-loop --no-check   (no --out: profiled times stay out of the record)
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

import numpy as np  # noqa: E402

# (m, n, density): rows = m + 1, cols = n + m + 1
SHAPES = [(7, 6, 1.0), (32, 64, 1.0), (256, 512, 1.0), (512, 1024, 1.0), (4096, 8192, 1.0),
          (4096, 8192, 0.05)]
LOOP_ALL_UP_TO = 256      # m: the loop runs over all indices up to here
LOOP_SAMPLE = 64
HBM_PEAK = 8.0e12         # bytes / s
EPS = 1e-9


def gen_state(m: int, n: int, density: float, seed: int):
    """(T, x, z, basicVars): rows 1..k (k = min(m, n)) are basic in structural columns 0..k-1,
    rows k+1..m in their own slack column; every other column is dense in [-1, 1)."""
    rng = np.random.RandomState(seed)
    k = min(m, n)
    T = np.zeros((m + 1, n + m + 1))
    body = rng.uniform(-1.0, 1.0, size=(m, n + m))
    if density < 1.0:
        body *= rng.random_sample(size=(m, n + m)) < density
    T[1:, :n + m] = body
    T[0, :n + m] = rng.uniform(-1.0, 2.0, size=n + m)
    basic = list(range(k)) + [n + i - 1 for i in range(k + 1, m + 1)]
    T[:, basic] = 0.0
    T[np.arange(1, m + 1), basic] = 1.0
    T[1:, -1] = rng.uniform(-3.0, 10.0, size=m)
    T[0, -1] = 100.0
    x = np.zeros(n)
    x[:k] = T[1:k + 1, -1]
    return T, x, 100.0, basic


def count_divisions(T, m, basic):
    """One per entry beyond EPS of a column outside basicVars (its row's fold) and one per entry
    beyond EPS of the slack block (its column's fold)."""
    n = T.shape[1] - m - 1
    big = np.abs(T[1:, :n + m]) > EPS
    free = np.ones(n + m, dtype=bool)
    free[basic] = False
    return int(big[:, free].sum() + big[:, n:].sum())


def time_calls(fn, window: float, min_calls: int = 3):
    """(seconds per call, calls, per-call extras) over at least `window` seconds."""
    extras = []
    t0 = time.perf_counter()
    calls = 0
    while calls < min_calls or time.perf_counter() - t0 < window:
        extras.append(fn())
        calls += 1
    return (time.perf_counter() - t0) / calls, calls, extras


def host_loop(an, basic_cols, constraints):
    t0 = time.perf_counter()
    for j in basic_cols:
        an.BasicRange(j)
    for k in constraints:
        an.RHSRange(k)
    return time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--max-m", type=int, default=4096)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()

    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd.engine import SensState
    from lpr_381_group_v22_amd.sensitivity_analyzer import SensitivityAnalyzer
    import ref_py_ranging as ref
    import special_values as sv

    bad = 0
    records = []
    with pkg.Engine(0) as eng:
        for m, n, density in SHAPES:
            if m > args.max_m:
                continue
            T, x, z, basic = gen_state(m, n, density, args.seed + m)
            R, Cc = T.shape
            ld = (Cc + 15) // 16 * 16
            st = SensState.create(eng, T, x, z)
            for _ in range(2):                              # warm-up: code objects, buffers
                rep = st.ranging()

            def one():
                st.ranging()
                return st.ranging_times()

            per_call, calls, times = time_calls(one, args.window)
            sweep_ms = statistics.median(t[0] for t in times)
            finish_ms = statistics.median(t[1] for t in times)
            sweep_bytes = m * ld * 8
            share = sweep_bytes / (sweep_ms * 1e-3) / HBM_PEAK
            rec = dict(rows=R, cols=Cc, density=density, calls=calls, e2e_ms=per_call * 1e3,
                       sweep_ms=sweep_ms, finish_ms=finish_ms, sweep_bytes=sweep_bytes,
                       divisions=count_divisions(T, m, basic), hbm_share=share,
                       sweep_gbps=sweep_bytes / (sweep_ms * 1e-3) / 1e9,
                       bound="HBM" if share >= 0.5 else "ALU/latency")
            if not args.no_check:
                want = ref.report_numpy(T, basic)
                ok = all(np.array_equal(getattr(rep, f), want[f]) if f in ref.INT_FIELDS
                         else sv.same(getattr(rep, f), want[f]) for f in ref.FIELDS)
                rec["matches_restatement"] = bool(ok)
                bad += not ok
            if not args.no_loop:
                an = SensitivityAnalyzer(None, (), 0.0, None, _state=st)
                if m <= LOOP_ALL_UP_TO:
                    cols, cons, scale = list(basic), list(range(1, m + 1)), 1.0
                else:
                    pick = np.linspace(0, m - 1, LOOP_SAMPLE).astype(int)
                    cols, cons = [basic[q] for q in pick], (pick + 1).tolist()
                    scale = m / LOOP_SAMPLE
                host_loop(an, cols[:2], cons[:2])           # warm-up
                loop_s = host_loop(an, cols, cons) * scale
                rec.update(loop_ms=loop_s * 1e3, loop_extrapolated=scale != 1.0,
                           loop_indices_run=len(cols) + len(cons),
                           speedup=loop_s / per_call)
            st.destroy()
            records.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/ranging_bench.py", seed=args.seed, window_s=args.window,
                           hbm_peak_bytes_per_s=HBM_PEAK, shapes=records), f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
