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

--narrate measures the narrated batch instead, on the same workloads cut to
NARR_COUNTS items so that the data slab stays within a few GB, all values kept:
  (a) narrated end to end: a counting handle (caps 0) and a keeping handle, two runs,
      lpr_cut_batch_narrate_read_all; also the keeping handle's run alone
  (b) the un-narrated batch in the same process (create, run, bulk reads)
  (c) CPU: the restatement loop tests/ref_py_cut_text.py producing the same numbers, one core of
      the same host, a time-bounded prefix.  The only ratio given is (c) / (a), per item.
256 evenly spaced items per workload (every item where the cut workload has fewer: H has 64) are
compared block by block with the restatement.

--parent-lib PATH measures what moving the kernel body into a shared text cost the un-narrated
batch: lpr_cut_batch_run of this library and of the parent commit's library (PATH) on the full
workloads, fresh child processes alternated (parent, this) --parent-rounds times, a pass = the
median of --repeat runs in its process; margin = the parent's own max - min over its passes.  One
JSON line per workload with both sets of passes is appended to --out.
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
NARR_COUNTS = {"S": 16384, "G": 1024, "H": 64}
NARR_CHECK = 256   # evenly spaced items per workload (H is cut to 64 items: every one of them)


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


def narrated_pass(pkg, eng, tabs, max_cuts):
    """(seconds end to end, seconds of the keeping run, the keeping batch, info, events, data)"""
    eng.sync()
    t0 = time.perf_counter()
    count = pkg.CuttingPlaneBatch.from_arrays(eng, tabs, max_cuts=max_cuts, log_cap=64)
    count.narrate_reserve(0, 1)
    count.Run(hard_cap=HARD_CAP)
    need = count.narration_info()
    count.destroy()
    keep = pkg.CuttingPlaneBatch.from_arrays(eng, tabs, max_cuts=max_cuts, log_cap=64)
    keep.narrate_reserve(need.doubles_made, int(need.events_made.max()))
    t1 = time.perf_counter()
    keep.Run(hard_cap=HARD_CAP)
    eng.sync()
    t2 = time.perf_counter()
    info = keep.narration_info()
    ev, data = keep.narration_packed()
    keep.result_arrays()
    eng.sync()
    t3 = time.perf_counter()
    return t3 - t0, t2 - t1, keep, info, ev, data


def narrate_main(args, pkg, orc, eng) -> int:
    import ref_py_cut_text as rt
    failures = 0
    lines = []
    repeat = max(1, args.repeat)
    for i, name in enumerate(args.workloads.split(",")):
        tabs = gen_workload(orc, name, args.seed + 1000 * i)[:NARR_COUNTS[name]]
        mc, count = MAX_CUTS[name], len(tabs)
        narrated_pass(pkg, eng, tabs, mc)[2].destroy()  # warm-up
        a_e2e, a_run = [], []
        for p in range(repeat):
            e2e, run, keep, info, ev, data = narrated_pass(pkg, eng, tabs, mc)
            a_e2e.append(e2e)
            a_run.append(run)
            if p < repeat - 1:
                keep.destroy()
        plain = []
        for _ in range(repeat):
            r = run_batch(pkg, eng, tabs, mc)
            plain.append((r[0], r[1]))
            r[3].destroy()
        # (c) the CPU restatement, one core, a time-bounded prefix
        done, t0 = 0, time.perf_counter()
        while done < count and time.perf_counter() - t0 < args.oracle_seconds:
            rt.narrate_cutting_plane(tabs[done], mc, hard_cap=HARD_CAP, text=False)
            done += 1
        cpu_s = time.perf_counter() - t0
        # block by block against the restatement
        bad, checked = 0, 0
        step = max(1, count // NARR_CHECK)
        for k in list(range(0, count, step))[:NARR_CHECK]:
            n = rt.narrate_cutting_plane(tabs[k], mc, hard_cap=HARD_CAP, text=False)[0]
            want = np.concatenate([np.asarray(n.record0).reshape(-1)] +
                                  [np.asarray(b, dtype=np.float64).reshape(-1) for b in n.blocks])
            at = int(info.data_off[k])
            ok = int(info.doubles_made[k]) == int(info.doubles_kept[k]) == want.size and \
                data[at:at + want.size].tobytes() == want.tobytes() and \
                [tuple(t) for t in ev[k, :int(info.events_made[k])].tolist()] == n.events
            bad += not ok
            checked += 1
        keep.destroy()
        failures += bad
        rec = dict(workload=name, narrate=True, items=count, of_section_15_items=COUNTS[name],
                   rows=int(tabs[0].shape[0]), cols=int(tabs[0].shape[1]), max_cuts=mc,
                   hard_cap=HARD_CAP, data_doubles=int(info.doubles_made.sum()),
                   data_bytes=int(info.doubles_made.sum()) * 8,
                   events=int(info.events_made.sum()),
                   a_narrated_e2e_seconds_all=a_e2e, a_narrated_run_seconds_all=a_run,
                   a_narrated_e2e_items_per_s=count / min(a_e2e),
                   a_narrated_run_items_per_s=count / min(a_run),
                   b_unnarrated_e2e_seconds_all=[p[0] for p in plain],
                   b_unnarrated_run_seconds_all=[p[1] for p in plain],
                   c_cpu_restatement_1core=dict(items=done, seconds=cpu_s,
                                                items_per_s=done / cpu_s),
                   c_over_a_per_item=(cpu_s / done) / (min(a_e2e) / count),
                   blocks_checked_items=checked, block_mismatches=bad)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"narration check: {failures} item(s) differ from the restatement", file=sys.stderr)
        return 1
    return 0


def run_child(path: str, names, seed: int, repeat: int) -> int:
    """--run-child: lpr_cut_batch_run alone through the library at `path` (raw ctypes: the
    parent's library has no narrate calls), `repeat` runs per workload, one JSON line."""
    import ctypes as C
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.cut_batch import pack_tableaux
    from oracle_lib import Oracle
    lib = C.CDLL(path)
    P = C.c_void_p
    lib.lpr_engine_open.argtypes = [C.c_int, C.POINTER(P)]
    lib.lpr_engine_sync.argtypes = [P]
    lib.lpr_engine_close.argtypes = [P]
    lib.lpr_cut_batch_create.argtypes = [P, C.c_int32, P, P, P, C.c_int32, C.c_int32, C.POINTER(P)]
    lib.lpr_cut_batch_run.argtypes = [P, C.POINTER(N.CutBatchOpts), C.POINTER(N.CutBatchResult)]
    lib.lpr_cut_batch_destroy.argtypes = [P]
    orc = Oracle()
    eng = P()
    if lib.lpr_engine_open(0, C.byref(eng)) != 0:
        return 1
    out = {}
    for name in names:
        tabs = gen_workload(orc, name, seed + 1000 * "SGH".index(name))
        p = pack_tableaux(tabs, MAX_CUTS[name])
        times = []
        for _ in range(repeat + 1):   # the first run is the warm-up
            h = P()
            if lib.lpr_cut_batch_create(eng, len(p.rows), p.rows.ctypes.data, p.cols.ctypes.data,
                                        p.tableaux.ctypes.data, MAX_CUTS[name], 64,
                                        C.byref(h)) != 0:
                return 1
            opts = N.CutBatchOpts(hard_cap=HARD_CAP)
            res = N.CutBatchResult()
            lib.lpr_engine_sync(eng)
            t0 = time.perf_counter()
            if lib.lpr_cut_batch_run(h, C.byref(opts), C.byref(res)) != 0:
                return 1
            times.append(time.perf_counter() - t0)
            lib.lpr_cut_batch_destroy(h)
        out[name] = times[1:]
    lib.lpr_engine_close(eng)
    print(json.dumps(out), flush=True)
    return 0


def against_parent(args) -> int:
    import statistics
    import subprocess
    from lpr_381_group_v22_amd import _native as N
    names = args.workloads.split(",")
    runs = {"parent": [], "this": []}
    for _ in range(max(1, args.parent_rounds)):
        for tag, path in (("parent", args.parent_lib), ("this", N.LIB_PATH)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--run-child",
                                os.path.abspath(path), "--workloads", ",".join(names),
                                "--seed", str(args.seed), "--repeat", str(args.repeat)],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"run child on {path} failed: {p.stderr[-400:]}")
            runs[tag].append(json.loads(p.stdout.strip().splitlines()[-1]))
    lines = []
    for name in names:
        par = [statistics.median(r[name]) for r in runs["parent"]]
        this = [statistics.median(r[name]) for r in runs["this"]]
        margin = max(par) - min(par)
        diff = statistics.mean(this) - statistics.mean(par)
        lines.append(json.dumps(dict(
            workload=name, unnarrated_ab=True, items=COUNTS[name], rounds=len(par),
            runs_per_pass=args.repeat, parent_run_seconds_passes=par,
            this_run_seconds_passes=this,
            parent_run_seconds_all=[r[name] for r in runs["parent"]],
            this_run_seconds_all=[r[name] for r in runs["this"]],
            margin_seconds=margin, this_mean_minus_parent_mean_seconds=diff,
            within_parent_margin=bool(diff <= margin))))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="S,G,H")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--single-seconds", type=float, default=4.0)
    ap.add_argument("--oracle-seconds", type=float, default=4.0)
    ap.add_argument("--no-check", action="store_true", help="skip the bit check and the loops")
    ap.add_argument("--narrate", action="store_true",
                    help="measure the narrated batch (DESIGN.md section 24); the committed record "
                         "is profiles/cut_batch_narr_bench.json")
    ap.add_argument("--out", default=None,
                    help="also append the JSON lines to this file (the committed record is "
                         "profiles/cut_batch_bench.json; never pass it to a profiled run)")
    ap.add_argument("--parent-lib", default=None,
                    help="the parent commit's liblpr_engine.so: the un-narrated run of this "
                         "library against it, fresh processes alternated")
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--run-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.run_child:
        return run_child(args.run_child, args.workloads.split(","), args.seed,
                         max(1, args.repeat))
    if args.parent_lib:
        return against_parent(args)

    import lpr_381_group_v22_amd as pkg
    from oracle_lib import Oracle
    orc = Oracle()  # the LPs behind S are solved on the CPU, outside every timed region
    failures = 0
    lines = []
    repeat = max(1, args.repeat)
    if args.narrate:
        with pkg.Engine(0) as eng:
            return narrate_main(args, pkg, orc, eng)
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
