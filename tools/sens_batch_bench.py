"""Measures the sensitivity scenario batch and prints one JSON line per
workload:

  S   a solved 8 x 14 LP (m = 7, n = 6), 65536 one-edit scenarios: the RHS of every row and the
      cost of every column (change_nonbasic_cbar or change_basic, by what the column is) at a
      spread of values
  G   a solved 33 x 97 LP (m = 32, n = 64), 4096 three-edit scripts (RHS, cost, RHS)
  H   a solved 257 x 769 LP (m = 256, n = 512), 256 two-edit scripts (RHS, cost): form H

With --grow the scripts hold the two edits that grow the tableau and run through
SensitivityGrowBatch (lpr_sens_batch_create_grow); the committed record of that is
profiles/sens_grow_bench.json:

  S   the 8 x 14 base, 65536 candidate products: one add_activity per scenario
  G   the 33 x 97 base, 4096 scripts: add_constraint (a cap on one variable), then change_rhs
  H   the 257 x 769 base, 256 scripts: add_activity, then add_constraint

With --models the scenarios start from different solved models (SensitivityModelBatch,
lpr_sens_batch_from_batch); the committed record of that is
profiles/sens_model_batch_bench.json.  The LP workloads are those of tools/batch_bench.py (W: 65536
textbook LPs, G: 4096 of 32 x 64, H: 256 of 256 x 512), solved with PrimalSimplexBatch; the optimal
ones are kept.  Two runs are timed separately: from_batch + ranging_arrays() (a report per model),
and from_batch with one change_rhs per model + Run + ranging_arrays().  The baseline is the loop
this replaces: per model GetFinalTableau(k), SensState.create, the edit, ranging(), destroy, over a
time-bounded prefix and scaled (marked extrapolated).  256 evenly spaced scenarios per workload
are compared with that per-handle path in every output.

Per workload: scenarios/s end to end (lpr_sens_batch_create, lpr_sens_batch_run, the bulk reads of
outcomes / pivots / z / basicVars, closed by an engine sync) and for lpr_sens_batch_run alone
(best of --repeat, after one warm-up pass); launches; pivots; the same scenarios one at a time
through SensState.create + the edit calls + shape() + destroy in a Python loop (a time-bounded
prefix); the CPU oracle on one core (a prefix).  256 scenarios per workload (evenly spaced) are
checked against the oracle bit for bit (outcomes, pivots, log, tableau, basicVars, z, solution);
any mismatch makes the exit status non-zero.  Inputs are seeded.

The single-handle loop and the oracle loop cover a time-bounded prefix of the scenarios
(`scenarios` in their records); `speedup_e2e_vs_single` compares the batch's rate over all
scenarios with the loop's rate over that prefix, and `speedup_prefix_scenarios` says how many it
covered.  In S the edit kind cycles with period 20, so any prefix of 20 or more has the full mix.

Run it under a time limit:  timeout -k 10 900 python tools/sens_batch_bench.py --out
profiles/sens_batch_bench.json
Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python
tools/sens_batch_bench.py --no-check --repeat 1   (no --out: profiled times stay out of the record)
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
SHAPES = {"S": (7, 6, 65536), "G": (32, 64, 4096), "H": (256, 512, 256)}


def gen_workload(orc, name: str, seed: int):
    """(base, scripts): a solved random_dense LP and `count` scripts over it."""
    import sens_cases
    m, n, count = SHAPES[name]
    base = sens_cases.solved_lp(orc, m, n, seed % 1000)
    T, _, _, basis = base
    R, C = T.shape
    rng = np.random.RandomState(seed)
    bset = set(int(b) for b in basis)

    def rhs_edit(q):
        k = 1 + q % (R - 1)
        return ("change_rhs", (k, float(T[k, -1]) * float(rng.uniform(0.25, 2.0))))

    def cost_edit(q):
        j = q % (C - 1)
        if j in bset:
            return ("change_basic", (j, float(rng.uniform(-0.5, 0.5))))
        return ("change_nonbasic_cbar", (j, float(T[0, j]) + float(rng.uniform(-0.6, 0.4))))

    scripts = []
    for q in range(count):
        if name == "S":
            t = q % (R - 1 + C - 1)
            scripts.append([rhs_edit(t) if t < R - 1 else cost_edit(t - (R - 1))])
        elif name == "G":
            scripts.append([rhs_edit(q), cost_edit(q), rhs_edit(q + 7)])
        else:
            scripts.append([rhs_edit(q), cost_edit(3 * q)])
    return base, scripts


def gen_grow_workload(orc, name: str, seed: int):
    """(base, scripts): the base of gen_workload and `count` scripts that grow it."""
    base, keep = gen_workload(orc, name, seed)
    T, x, _, _ = base
    R, C = T.shape
    n = C - R
    rng = np.random.RandomState(seed + 1)
    made = [j for j in range(n) if x[j] > 1e-6] or list(range(n))  # the products in the plan

    def activity(rows):
        """A candidate product: a sparse-ish column and a cost near its shadow value, so that
        some candidates enter the basis and some do not."""
        a = rng.uniform(0.0, 1.0, size=rows - 1) * (rng.uniform(size=rows - 1) < 0.5)
        y = T[0, n:n + R - 1]
        worth = float(y @ a[:R - 1])
        return ("add_activity", (worth * float(rng.uniform(0.6, 1.4)), a.tolist()))

    def cap(q, cols):
        """x_j <= 0.3 .. 1.3 of its value: most caps bite, some do not."""
        tech = np.zeros(cols - 1)
        j = made[q % len(made)]
        tech[j] = 1.0
        return ("add_constraint", (tech.tolist(), float(x[j]) * float(rng.uniform(0.3, 1.3))))

    scripts = []
    for q in range(len(keep)):
        if name == "S":
            scripts.append([activity(R)])
        elif name == "G":
            scripts.append([cap(q, C), keep[q][0]])
        else:
            scripts.append([activity(R), cap(q, C + 1)])
    return base, scripts


def run_batch(pkg, eng, base_handle, scripts, grow=False):
    """One end-to-end pass: (seconds end to end, seconds of the run, result, batch)."""
    eng.sync()
    t0 = time.perf_counter()
    b = (pkg.SensitivityGrowBatch if grow else pkg.SensitivityBatch)(base_handle, scripts)
    t1 = time.perf_counter()
    res = b.Run()
    t2 = time.perf_counter()
    b.outcome_arrays()
    b.state_arrays()
    eng.sync()
    t3 = time.perf_counter()
    return t3 - t0, t2 - t1, res, b


def single_loop(SensState, eng, base, scripts, budget_s: float):
    T, x, z, _ = base
    done = 0
    t0 = time.perf_counter()
    while done < len(scripts) and time.perf_counter() - t0 < budget_s:
        d = SensState.create(eng, T, x, z)
        for op, args in scripts[done]:
            getattr(d, op)(*args)
        d.shape()
        d.destroy()
        done += 1
    dt = time.perf_counter() - t0
    return dict(scenarios=done, seconds=dt, scenarios_per_s=done / dt)


def oracle_loop(orc, base, scripts, budget_s: float):
    T, x, z, basis = base
    done = 0
    t0 = time.perf_counter()
    while done < len(scripts) and time.perf_counter() - t0 < budget_s:
        o = orc.sens(T, x, z, basis)
        for op, args in scripts[done]:
            getattr(o, op)(*args)
        done += 1
    dt = time.perf_counter() - t0
    return dict(scenarios=done, seconds=dt, scenarios_per_s=done / dt)


def bit_check(orc, base, scripts, batch) -> int:
    """Scenarios among CHECK evenly spaced ones that differ from the oracle in any output."""
    import sens_batch_cases
    bad = 0
    step = max(1, len(scripts) // CHECK)
    for k in list(range(0, len(scripts), step))[:CHECK]:
        ref = sens_batch_cases.oracle_run(orc, base, scripts[k])
        try:
            sens_batch_cases.same_scenario(batch, k, ref, k)
        except AssertionError:
            bad += 1
    return bad


# ---- --models: scenarios that start from different solved models ---------------------------------
def solved_lp_batch(pkg, N, eng, w):
    """A solved PrimalSimplexBatch over the packed workload w of tools/batch_bench.py."""
    import ctypes as C
    import batch_bench as bb
    h = C.c_void_p()
    count = len(w["n"])
    N.check(N.lib.lpr_batch_from_lps(
        eng._h, count, bb.ptr(w["n"], C.c_int32), bb.ptr(w["m"], C.c_int32),
        bb.ptr(w["obj"], C.c_double), bb.ptr(w["A"], C.c_double), bb.ptr(w["ncoef"], C.c_int32),
        bb.ptr(w["rel"], C.c_int8), bb.ptr(w["rhs"], C.c_double), bb.ptr(w["is_max"], C.c_int8),
        0, C.byref(h)), "lpr_batch_from_lps")
    lps = pkg.PrimalSimplexBatch.__new__(pkg.PrimalSimplexBatch)
    lps._init(eng)
    lps._attach(h, [(int(m) + 1, int(n) + int(m) + 1, int(n)) for n, m in zip(w["n"], w["m"])], 0)
    opts, res = N.BatchOpts(max_pivots=0, chunk=0, variant=0), N.BatchResult()
    N.check(N.lib.lpr_batch_solve(h, C.byref(opts), C.byref(res)), "lpr_batch_solve")
    return lps


def run_models(pkg, eng, lps, items, scripts, run: bool):
    """One pass: (seconds end to end, constructor kernel ms, ranging kernel ms, batch, report)."""
    eng.sync()
    t0 = time.perf_counter()
    b = pkg.SensitivityModelBatch(lps, scripts, items=items)
    if run:
        b.Run()
    rep = b.ranging_arrays()
    eng.sync()
    t1 = time.perf_counter()
    return t1 - t0, b.ConstructTime(), b.RangingTime(), b, rep


def models_handle(SensState, eng, lps, x_at, x, z, k, script):
    """The per-handle path for LP k: (handle after the script, outcomes)."""
    T = lps.GetFinalTableau(k)
    n = lps.Shape(k)[2]
    d = SensState.create(eng, T, x[x_at[k]:x_at[k] + n], float(z[k]))
    return d, [getattr(d, op)(*args) for op, args in script]


def models_loop(SensState, eng, lps, x_at, x, z, items, scripts, budget_s: float):
    done = 0
    t0 = time.perf_counter()
    while done < len(items) and time.perf_counter() - t0 < budget_s:
        d, _ = models_handle(SensState, eng, lps, x_at, x, z, items[done], scripts[done])
        d.ranging()
        d.destroy()
        done += 1
    dt = time.perf_counter() - t0
    return dict(scenarios=done, seconds=dt, scenarios_per_s=done / dt,
                extrapolated=done < len(items))


def models_check(SensState, eng, lps, x_at, x, z, items, scripts, batch, rep) -> int:
    """Scenarios among CHECK evenly spaced ones that differ from the per-handle path in any output:
    outcomes, tableau, basicVars, solution, z and the nine ranging arrays."""
    from lpr_381_group_v22_amd.sens_batch import (RANGING_COLUMN_FIELDS, RANGING_ROW_FIELDS,
                                                  trim_ranging)
    import special_values as sv
    bad = 0
    step = max(1, len(items) // CHECK)
    rows, cols, _, _ = batch.shape_arrays()
    for q in list(range(0, len(items), step))[:CHECK]:
        d, outs = models_handle(SensState, eng, lps, x_at, x, z, items[q], scripts[q])
        T, basic, sol = d.read()
        want = d.ranging()
        st = batch.State(q)
        got = trim_ranging(rep, q, int(rows[q]), int(cols[q]))
        ok = (batch.Outcomes(q) == outs and st["T"].shape == T.shape
              and st["T"].tobytes() == T.tobytes() and st["basic"] == basic.tolist()
              and st["sol"].tobytes() == sol.tobytes() and sv.same(st["z"], d.shape()[4])
              and all(sv.same(getattr(got, f), getattr(want, f)) for f in RANGING_COLUMN_FIELDS + RANGING_ROW_FIELDS))
        bad += not ok
        d.destroy()
    return bad


def main_models(args) -> int:
    import batch_bench as bb
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.engine import SensState
    failures, lines = 0, []
    names = {"S": "W", "G": "G", "H": "H"}
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            w = bb.gen_workload(names[name], args.seed + i)
            offs = bb.offsets(w)
            lps = solved_lp_batch(pkg, N, eng, w)
            items = pkg.optimal_items(lps)
            _, _, z = lps.status_arrays()
            x = lps.solution_packed()
            x_at = offs[0]
            shapes = [lps.Shape(k) for k in items]
            edit = [[("change_rhs", (1, float(w["rhs"][offs[2][k]]) * 1.25))] for k in items]
            none = [[] for _ in items]
            rec = dict(workload=name + "_models", lps=int(lps.Count), scenarios=len(items),
                       max_rows=max(s[0] for s in shapes), max_cols=max(s[1] for s in shapes))
            # what the constructor kernel has to move at the least: every tableau read and written
            rec["ctor_bytes_min"] = int(sum(2 * 8 * s[0] * s[1] for s in shapes))
            for tag, scripts, run in (("report", none, False), ("edit_report", edit, True)):
                run_models(pkg, eng, lps, items, scripts, run)[3].destroy()  # warm-up
                runs = [run_models(pkg, eng, lps, items, scripts, run)
                        for _ in range(max(1, args.repeat))]
                best = min(runs, key=lambda r: r[0])
                r = dict(e2e_seconds=best[0], e2e_scenarios_per_s=len(items) / best[0],
                         e2e_seconds_all=[q[0] for q in runs],
                         ctor_kernel_ms=min(q[1] for q in runs),
                         ranging_kernel_ms=min(q[2] for q in runs))
                r["ctor_gbytes_per_s"] = rec["ctor_bytes_min"] / (r["ctor_kernel_ms"] * 1e-3) / 1e9
                batch, rep = runs[-1][3], runs[-1][4]
                if run:
                    oc, pv = batch.outcome_arrays()
                    r["form"] = {1: "G", 2: "H"}[batch.LastResult.form]
                    r["pivots"] = int(pv.sum())
                    r["outcomes"] = {str(int(c)): int((oc == c).sum()) for c in np.unique(oc)}
                if not args.no_check:
                    if run:
                        bad = models_check(SensState, eng, lps, x_at, x, z, items, scripts, batch,
                                           rep)
                        rec["checked"] = min(CHECK, len(items))
                        rec["mismatches"] = bad
                        failures += bad
                    r["per_handle_loop"] = models_loop(SensState, eng, lps, x_at, x, z, items,
                                                       scripts, args.single_seconds)
                    r["ratio_to_loop"] = r["e2e_scenarios_per_s"] / \
                        r["per_handle_loop"]["scenarios_per_s"]
                for q in runs:
                    q[3].destroy()
                rec[tag] = r
            lps.destroy()
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"check: {failures} scenario(s) differ from the per-handle path", file=sys.stderr)
        return 1
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S,G,H")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261017)
    ap.add_argument("--single-seconds", type=float, default=5.0)
    ap.add_argument("--oracle-seconds", type=float, default=5.0)
    ap.add_argument("--no-check", action="store_true", help="skip the bit check and the loops")
    ap.add_argument("--grow", action="store_true",
                    help="the growth workloads (add_activity / add_constraint) through "
                         "SensitivityGrowBatch")
    ap.add_argument("--models", action="store_true",
                    help="scenarios that start from different solved models, through "
                         "SensitivityModelBatch (record: profiles/sens_model_batch_bench.json)")
    ap.add_argument("--out", default=None,
                    help="also append the JSON lines to this file (the committed record is "
                         "profiles/sens_batch_bench.json; never pass it to a profiled run)")
    args = ap.parse_args()
    if args.models:
        return main_models(args)

    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd.engine import SensState
    from oracle_lib import Oracle
    orc = Oracle()  # the bases are solved on the CPU, outside every timed region
    failures = 0
    lines = []
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            gen = gen_grow_workload if args.grow else gen_workload
            base, scripts = gen(orc, name, args.seed + i)
            T, x, z, _ = base
            d = SensState.create(eng, T, x, z)
            run_batch(pkg, eng, d, scripts, args.grow)[3].destroy()  # warm-up
            runs = [run_batch(pkg, eng, d, scripts, args.grow)
                    for _ in range(max(1, args.repeat))]
            best_e2e = min(r[0] for r in runs)
            best_run = min(r[1] for r in runs)
            res, batch = runs[-1][2], runs[-1][3]
            oc, pv = batch.outcome_arrays()
            count = len(scripts)
            rec = dict(workload=name + ("_grow" if args.grow else ""), scenarios=count, rows=int(T.shape[0]), cols=int(T.shape[1]),
                       edits=int(len(oc)), form={1: "G", 2: "H"}[res.form],
                       pivots=int(pv.sum()), launches=res.launches,
                       outcomes={str(int(c)): int((oc == c).sum()) for c in np.unique(oc)},
                       e2e_seconds=best_e2e, e2e_scenarios_per_s=count / best_e2e,
                       run_seconds=best_run, run_scenarios_per_s=count / best_run,
                       e2e_seconds_all=[r[0] for r in runs],
                       run_seconds_all=[r[1] for r in runs])
            if not args.no_check:
                bad = bit_check(orc, base, scripts, batch)
                rec["bit_checked"] = min(CHECK, count)
                rec["bit_mismatches"] = bad
                failures += bad
                rec["single_handle"] = single_loop(SensState, eng, base, scripts,
                                                   args.single_seconds)
                rec["cpu_oracle_1core"] = oracle_loop(orc, base, scripts, args.oracle_seconds)
                rec["speedup_e2e_vs_single"] = rec["e2e_scenarios_per_s"] / \
                    rec["single_handle"]["scenarios_per_s"]
                rec["speedup_prefix_scenarios"] = rec["single_handle"]["scenarios"]
            for r in runs:
                r[3].destroy()
            d.destroy()
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"bit check: {failures} scenario(s) differ from the oracle", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
