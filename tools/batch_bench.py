"""Measures the batched primal simplex and prints one JSON line per workload:

  W   65536 textbook LPs, m ~ U{3..8}, n ~ U{3..12}; even k random_dense style (A, c ~ U(0,1),
      b = 1 + U(0,1) n / 4, all "<="), odd k tie_heavy style (small integers, "<=", "=", ">=")
  G   4096 LPs, m = 32, n = 64, the same two styles alternating
  H   256 LPs, m = 256, n = 512, random_dense style

Per workload: LPs/s and pivots/s end to end (lpr_batch_from_lps, lpr_batch_solve, the bulk reads
of status / Z / x / basis, closed by an engine sync) and for lpr_batch_solve alone (best of
--repeat); launches; the same LPs one at a time through Tableau.from_lp + solve + reads in a
Python loop (a time-bounded prefix); the CPU oracle on one core (a prefix).  Every solve is
capped at 5000 pivots per LP (tie-heavy LPs can cycle), the oracle too.  256 LPs per workload are
checked against the oracle bit for bit (tableau, status, pivots, log, basis, Z, x); any mismatch
makes the exit status non-zero.  Inputs are seeded (numpy RandomState(seed + workload)).

With --trace it measures the traced batch instead, on the same three
workloads, and appends one JSON line per workload to profiles/batch_trace_bench.json: (a) traced
end to end (create + lpr_batch_trace_reserve + solve + lpr_batch_trace_read_all) and the traced
solve alone, (b) the untraced batch in the same process, (c) what the trace replaces -- per model
the stepwise loop of PrimalSimplexSolver(..., snapshots="all"): select_entering, select_leaving,
pivot and a full tableau read per pivot for the first trace_cap records, one solve call for the
rest, a time-bounded prefix, the rate scaled to the workload -- and, with --parent-lib, (d) the
untraced solve of this library against the parent commit's, fresh processes alternated
(--parent-rounds rounds of --repeat passes; --parent-only measures (d) alone).  256 LPs
per workload are compared record by record with the stepped oracle.  Every pass's value is kept.

Run it under a time limit:  timeout -k 10 900 python tools/batch_bench.py [--out FILE]
Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -d DIR -- python
tools/batch_bench.py --no-check --repeat 1
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

CAP = 5000
CHECK = 256


def gen_workload(name: str, seed: int):
    """Packed arrays (n, m, obj, A, ncoef, rel, rhs, is_max) of one workload."""
    rng = np.random.RandomState(seed)
    count, fixed = {"W": (65536, None), "G": (4096, (32, 64)), "H": (256, (256, 512))}[name]
    ns, ms, obj, A, rel, rhs = [], [], [], [], [], []
    for k in range(count):
        if fixed:
            m, n = fixed
        else:
            m, n = int(rng.randint(3, 9)), int(rng.randint(3, 13))
        if name == "H" or k % 2 == 0:  # random_dense
            a = rng.rand(m, n)
            b = 1.0 + rng.rand(m) * n / 4.0
            c = rng.rand(n)
            r = np.zeros(m, dtype=np.int8)
        else:  # tie_heavy: "<=" x3, "=", ">="
            a = rng.randint(0, 4, size=(m, n)).astype(float)
            b = rng.randint(0, 6, size=m).astype(float)
            c = rng.randint(1, 4, size=n).astype(float)
            r = np.array([0, 0, 0, 2, 1], dtype=np.int8)[rng.randint(0, 5, size=m)]
        ns.append(n)
        ms.append(m)
        obj.append(c)
        A.append(a.reshape(-1))
        rel.append(r)
        rhs.append(b)
    n_a = np.asarray(ns, dtype=np.int32)
    m_a = np.asarray(ms, dtype=np.int32)
    return dict(n=n_a, m=m_a, obj=np.concatenate(obj), A=np.concatenate(A),
                ncoef=np.concatenate([np.full(m, n, dtype=np.int32) for n, m in zip(ns, ms)]),
                rel=np.concatenate(rel), rhs=np.concatenate(rhs),
                is_max=np.ones(count, dtype=np.int8))


def offsets(w):
    n, m = w["n"].astype(np.int64), w["m"].astype(np.int64)
    return (np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(m * n)]),
            np.concatenate([[0], np.cumsum(m)]))


def lp_of(w, offs, k):
    on, oa, om = offs
    n, m = int(w["n"][k]), int(w["m"][k])
    return (w["obj"][on[k]:on[k] + n], w["A"][oa[k]:oa[k] + m * n].reshape(m, n),
            w["ncoef"][om[k]:om[k] + m], w["rel"][om[k]:om[k] + m], w["rhs"][om[k]:om[k] + m],
            bool(w["is_max"][k]))


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a.size else None


def run_batch(N, eng, w, check: bool):
    """One end-to-end pass: (seconds end to end, seconds of the solve, result, outputs)."""
    count = len(w["n"])
    st = np.zeros(count, dtype=np.int32)
    piv = np.zeros(count, dtype=np.int64)
    z = np.zeros(count)
    x = np.zeros(max(int(w["n"].sum()), 1))
    basis = np.zeros(max(int(w["m"].sum()), 1), dtype=np.int32)
    h = C.c_void_p()
    opts = N.BatchOpts(max_pivots=CAP, chunk=0, variant=0)
    res = N.BatchResult()
    eng.sync()
    t0 = time.perf_counter()
    N.check(N.lib.lpr_batch_from_lps(
        eng._h, count, ptr(w["n"], C.c_int32), ptr(w["m"], C.c_int32), ptr(w["obj"], C.c_double),
        ptr(w["A"], C.c_double), ptr(w["ncoef"], C.c_int32), ptr(w["rel"], C.c_int8),
        ptr(w["rhs"], C.c_double), ptr(w["is_max"], C.c_int8), 0, C.byref(h)),
        "lpr_batch_from_lps")
    t1 = time.perf_counter()
    N.check(N.lib.lpr_batch_solve(h, C.byref(opts), C.byref(res)), "lpr_batch_solve")
    t2 = time.perf_counter()
    N.check(N.lib.lpr_batch_status_read(h, ptr(st, C.c_int32), ptr(piv, C.c_int64),
                                        ptr(z, C.c_double)), "lpr_batch_status_read")
    N.check(N.lib.lpr_batch_solution_read(h, ptr(x, C.c_double)), "lpr_batch_solution_read")
    N.check(N.lib.lpr_batch_basis_read(h, ptr(basis, C.c_int32)), "lpr_batch_basis_read")
    eng.sync()
    t3 = time.perf_counter()
    out = dict(st=st, piv=piv, z=z, x=x, basis=basis, h=h)
    return t3 - t0, t2 - t1, res, out


def single_loop(pkg, eng, w, offs, budget_s: float, limit: int):
    done = pivots = 0
    t0 = time.perf_counter()
    while done < limit and time.perf_counter() - t0 < budget_s:
        o, A, nc, rel, rhs, mx = lp_of(w, offs, done)
        t = pkg.Tableau.from_lp(eng, o, A, rel, rhs, is_max=mx, ncoef=nc)
        r = t.solve(max_pivots=CAP)
        t.extract_solution(len(o))
        t.basis()
        t.destroy()
        pivots += int(r.pivots)
        done += 1
    dt = time.perf_counter() - t0
    return dict(lps=done, seconds=dt, lps_per_s=done / dt, pivots_per_s=pivots / dt)


def oracle_loop(orc, w, offs, budget_s: float, limit: int):
    done = pivots = 0
    t0 = time.perf_counter()
    while done < limit and time.perf_counter() - t0 < budget_s:
        o, A, nc, rel, rhs, mx = lp_of(w, offs, done)
        T, basis = orc.primal_build(o, A, rel, rhs, mx, nc)
        _, piv, _ = orc.primal_solve(T, basis, CAP)
        orc.extract_solution(T, len(o))
        pivots += piv
        done += 1
    dt = time.perf_counter() - t0
    return dict(lps=done, seconds=dt, lps_per_s=done / dt, pivots_per_s=pivots / dt)


def bit_check(N, orc, w, offs, out) -> int:
    """LPs among the first CHECK that differ from the oracle in any output."""
    h = out["h"]
    on, _, om = offs
    bad = 0
    for k in range(min(CHECK, len(w["n"]))):
        o, A, nc, rel, rhs, mx = lp_of(w, offs, k)
        n, m = len(o), len(rhs)
        T, basis = orc.primal_build(o, A, rel, rhs, mx, nc)
        st, piv, log = orc.primal_solve(T, basis, CAP)
        x, z = orc.extract_solution(T, n)
        got = np.empty_like(T)
        N.check(N.lib.lpr_batch_tableau_read(h, k, ptr(got, C.c_double)), "lpr_batch_tableau_read")
        lr = np.zeros(log.shape[0] + 1, dtype=np.int32)
        lc = np.zeros_like(lr)
        cnt = C.c_int64()
        N.check(N.lib.lpr_batch_log_read(h, k, ptr(lr, C.c_int32), ptr(lc, C.c_int32), len(lr),
                                         C.byref(cnt)), "lpr_batch_log_read")
        kept = cnt.value
        ok = (got.tobytes() == T.tobytes() and out["st"][k] == st and out["piv"][k] == piv
              and np.float64(out["z"][k]).tobytes() == np.float64(z).tobytes()
              and out["basis"][om[k]:om[k] + m].tobytes() == basis.tobytes()
              and np.array_equal(np.stack([lr[:kept], lc[:kept]], axis=1), log[:kept])
              and kept == min(piv, min(4096, 4 * ((m + 1) + (n + m + 1)))))
        if st == 0:
            ok = ok and out["x"][on[k]:on[k] + n].tobytes() == x.tobytes()
        bad += 0 if ok else 1
    return bad


# ------------------------------------------------------------------ --trace
# Records kept per LP: W keeps every record its LPs make; G and H keep a prefix (a record of H is
# about 1.6 MB).
TRACE_CAP = {"W": 0, "G": 16, "H": 2}  # 0: the most records any LP of the workload makes


def create(lib, eng_h, w, h):
    return lib.lpr_batch_from_lps(
        eng_h, len(w["n"]), ptr(w["n"], C.c_int32), ptr(w["m"], C.c_int32),
        ptr(w["obj"], C.c_double), ptr(w["A"], C.c_double), ptr(w["ncoef"], C.c_int32),
        ptr(w["rel"], C.c_int8), ptr(w["rhs"], C.c_double), ptr(w["is_max"], C.c_int8), 0,
        C.byref(h))


def run_traced(N, eng, w, trace_cap: int):
    """create + reserve + solve + trace_read_all: (seconds end to end, seconds of the solve,
    outputs)."""
    count = len(w["n"])
    rows, cols = w["m"].astype(np.int64) + 1, (w["n"] + w["m"]).astype(np.int64) + 1
    slab = np.empty(int(trace_cap * (2 + rows * cols).sum()))
    recs, off, st = (np.zeros(count, dtype=np.int64) for _ in range(3))
    h = C.c_void_p()
    opts = N.BatchOpts(max_pivots=CAP, chunk=0, variant=0)
    res = N.BatchResult()
    eng.sync()
    t0 = time.perf_counter()
    N.check(create(N.lib, eng._h, w, h), "lpr_batch_from_lps")
    N.check(N.lib.lpr_batch_trace_reserve(h, trace_cap), "lpr_batch_trace_reserve")
    t1 = time.perf_counter()
    N.check(N.lib.lpr_batch_solve(h, C.byref(opts), C.byref(res)), "lpr_batch_solve")
    t2 = time.perf_counter()
    N.check(N.lib.lpr_batch_trace_info(h, ptr(recs, C.c_int64), ptr(off, C.c_int64),
                                       ptr(st, C.c_int64)), "lpr_batch_trace_info")
    N.check(N.lib.lpr_batch_trace_read_all(h, ptr(slab, C.c_double), slab.size),
            "lpr_batch_trace_read_all")
    eng.sync()
    t3 = time.perf_counter()
    return t3 - t0, t2 - t1, dict(h=h, slab=slab, recs=recs, off=off, stride=st, res=res)


def step_loop(pkg, eng, w, offs, trace_cap: int, budget_s: float, limit: int):
    """What the traced batch replaces: per model the stepwise loop of the single mirror, with a
    full tableau read per record for the first trace_cap records, then one solve call for the
    rest and the read of the final tableau."""
    done = kept_all = 0
    t0 = time.perf_counter()
    while done < limit and time.perf_counter() - t0 < budget_s:
        o, A, nc, rel, rhs, mx = lp_of(w, offs, done)
        t = pkg.Tableau.from_lp(eng, o, A, rel, rhs, is_max=mx, ncoef=nc)
        t.read()
        kept = 1
        while kept < trace_cap:
            e = t.select_entering()
            if e == -1:
                break
            r = t.select_leaving(e)
            if r == -1:
                break
            t.pivot(r, e)
            t.read()
            kept += 1
        else:
            t.solve(max_pivots=CAP)
        t.read()
        t.destroy()
        kept_all += kept
        done += 1
    dt = time.perf_counter() - t0
    return dict(lps=done, seconds=dt, lps_per_s=done / dt, records_per_s=kept_all / dt)


def trace_check(orc, w, offs, out, trace_cap: int) -> int:
    """LPs among the first CHECK whose count or any kept record differs from the stepped oracle."""
    from batch_trace_cases import record_bytes, step_records
    bad = 0
    for k in range(min(CHECK, len(w["n"]))):
        o, A, nc, rel, rhs, mx = lp_of(w, offs, k)
        T, basis = orc.primal_build(o, A, rel, rhs, mx, nc)
        ref = step_records(orc, T, max_pivots=trace_cap - 1, keep=trace_cap)  # the kept prefix
        _, piv, _ = orc.primal_solve(T, basis, CAP)                           # the exact count
        ok = int(out["recs"][k]) == 1 + piv and len(ref["records"]) == min(1 + piv, trace_cap)
        stride = int(out["stride"][k])
        for i, want in enumerate(ref["records"]):
            at = int(out["off"][k]) + i * stride
            ok = ok and out["slab"][at:at + stride].tobytes() == record_bytes(want)
        bad += 0 if ok else 1
    return bad


def solve_child(lib_path: str, names, seed: int, repeat: int) -> int:
    """--solve-child: the untraced solve alone on the library at lib_path (it may predate the
    trace calls), `repeat` passes per workload, one JSON line."""
    from lpr_381_group_v22_amd import _native as N
    lib = C.CDLL(lib_path)
    for name in ("lpr_engine_open", "lpr_engine_close", "lpr_engine_sync", "lpr_batch_from_lps",
                 "lpr_batch_solve", "lpr_batch_destroy"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = N.SIGNATURES[name]
    eng = C.c_void_p()
    if lib.lpr_engine_open(0, C.byref(eng)) != 0:
        return 1
    out = {}
    for i, name in enumerate(names):
        w = gen_workload(name, seed + i)
        times = []
        for _ in range(repeat):
            h = C.c_void_p()
            opts = N.BatchOpts(max_pivots=CAP, chunk=0, variant=0)
            res = N.BatchResult()
            if create(lib, eng, w, h) != 0:
                return 1
            lib.lpr_engine_sync(eng)
            t0 = time.perf_counter()
            if lib.lpr_batch_solve(h, C.byref(opts), C.byref(res)) != 0:
                return 1
            times.append(time.perf_counter() - t0)
            lib.lpr_batch_destroy(h)
        out[name] = times
    lib.lpr_engine_close(eng)
    print(json.dumps(out), flush=True)
    return 0


def against_parent(args, names):
    """(d): the untraced solve of this library and of --parent-lib, alternating fresh child
    processes (this, parent) --parent-rounds times, --repeat passes each, all values kept, per
    process too."""
    import subprocess
    from lpr_381_group_v22_amd import _native as N
    runs = {"this": [], "parent": []}
    for _ in range(max(1, args.parent_rounds)):
        for tag, path in (("this", N.LIB_PATH), ("parent", args.parent_lib)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--solve-child", path,
                                "--workloads", ",".join(names), "--seed", str(args.seed),
                                "--repeat", str(args.repeat)],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"solve child on {path} failed: {p.stderr[-400:]}")
            runs[tag].append(json.loads(p.stdout.strip().splitlines()[-1]))
    out = {}
    for name in names:
        this = [t for r in runs["this"] for t in r[name]]
        parent = [t for r in runs["parent"] for t in r[name]]
        margin = max(max(r[name]) - min(r[name]) for r in runs["parent"])
        out[name] = dict(this_solve_seconds_all=this, parent_solve_seconds_all=parent,
                         this_by_process=[r[name] for r in runs["this"]],
                         parent_by_process=[r[name] for r in runs["parent"]],
                         this_best=min(this), parent_best=min(parent),
                         parent_margin_max_minus_min=margin,
                         within_margin=min(this) <= min(parent) + margin)
    return out


def main_parent_only(args) -> int:
    """--parent-only: (d) alone, one JSON line appended to the profile."""
    rec = dict(mode="untraced_solve_vs_parent", rounds=max(1, args.parent_rounds),
               passes_per_process=args.repeat,
               workloads=against_parent(args, args.workloads.split(",")))
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "batch_trace_bench.json"), "a") as f:
        f.write(line + "\n")
    return 0


def main_trace(args) -> int:
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    from oracle_lib import Oracle
    orc = Oracle()
    names = args.workloads.split(",")
    failures = 0
    lines = []
    with pkg.Engine(0) as eng:
        for i, name in enumerate(names):
            w = gen_workload(name, args.seed + i)
            offs = offsets(w)
            count = len(w["n"])
            plain = [run_batch(N, eng, w, check=False) for _ in range(3)]         # (b)
            most = 1 + int(plain[-1][3]["piv"].max())
            trace_cap = TRACE_CAP[name] or most
            for r in plain:
                N.lib.lpr_batch_destroy(r[3]["h"])
            traced = []
            for _ in range(3):                                                    # (a)
                traced.append(run_traced(N, eng, w, trace_cap))
                if len(traced) > 1:
                    N.lib.lpr_batch_destroy(traced[-2][2]["h"])
                    traced[-2][2]["slab"] = None
            out = traced[-1][2]
            print(f"{name}: traced and untraced passes done, trace_cap {trace_cap}",
                  file=sys.stderr, flush=True)
            bad = trace_check(orc, w, offs, out, trace_cap)
            failures += bad
            kept = int(np.minimum(out["recs"], trace_cap).sum())
            print(f"{name}: {bad} of {min(CHECK, count)} checked LPs differ from the oracle",
                  file=sys.stderr, flush=True)
            base = step_loop(pkg, eng, w, offs, trace_cap, args.single_seconds, count)  # (c)
            a_best = min(r[0] for r in traced)
            rec = dict(workload=name, mode="trace", lps=count, trace_cap=trace_cap,
                       most_records_of_an_lp=most, records=int(out["recs"].sum()),
                       records_kept=kept, trace_slab_bytes=int(out["slab"].nbytes),
                       traced_e2e_seconds_all=[r[0] for r in traced],
                       traced_solve_seconds_all=[r[1] for r in traced],
                       untraced_e2e_seconds_all=[r[0] for r in plain],
                       untraced_solve_seconds_all=[r[1] for r in plain],
                       traced_e2e_lps_per_s=count / a_best,
                       trace_price_e2e_seconds=a_best - min(r[0] for r in plain),
                       trace_price_solve_seconds=min(r[1] for r in traced)
                       - min(r[1] for r in plain),
                       step_loop=base, step_loop_seconds_scaled=count / base["lps_per_s"],
                       step_loop_is_extrapolated=base["lps"] < count,
                       speedup_traced_e2e_vs_step_loop=(count / a_best) / base["lps_per_s"],
                       trace_checked=min(CHECK, count), trace_mismatches=bad)
            N.lib.lpr_batch_destroy(out["h"])
            out["slab"] = None
            lines.append(rec)
    if args.parent_lib:
        d = against_parent(args, names)
        for rec in lines:
            rec["untraced_solve_vs_parent"] = d[rec["workload"]]
    text = [json.dumps(rec) for rec in lines]
    for line in text:
        print(line, flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "batch_trace_bench.json"), "a") as f:
        f.write("\n".join(text) + "\n")
    if failures:
        print(f"trace check: {failures} LP(s) differ from the oracle", file=sys.stderr)
        return 1
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true",
                    help="measure the traced batch (section 22) instead; appends to --out, by "
                         "default profiles/batch_trace_bench.json")
    ap.add_argument("--parent-lib", default=None,
                    help="--trace: a liblpr_engine.so built from the parent commit, for the "
                         "untraced solve against it")
    ap.add_argument("--parent-rounds", type=int, default=2,
                    help="--parent-lib: alternated rounds (this, parent), --repeat passes each")
    ap.add_argument("--parent-only", action="store_true",
                    help="with --parent-lib: only the untraced solve against the parent's, one "
                         "line appended to the profile")
    ap.add_argument("--solve-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workloads", default="W,G,H")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--single-seconds", type=float, default=5.0)
    ap.add_argument("--oracle-seconds", type=float, default=5.0)
    ap.add_argument("--no-check", action="store_true", help="skip the bit check and the loops")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.solve_child:
        return solve_child(args.solve_child, args.workloads.split(","), args.seed, args.repeat)
    if args.parent_only:
        if not args.parent_lib:
            ap.error("--parent-only needs --parent-lib")
        return main_parent_only(args)
    if args.trace:
        return main_trace(args)

    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    orc = None
    if not args.no_check:
        from oracle_lib import Oracle
        orc = Oracle()
    failures = 0
    lines = []
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            w = gen_workload(name, args.seed + i)
            offs = offsets(w)
            count = len(w["n"])
            runs = []
            for _ in range(max(1, args.repeat)):
                e2e, solve, res, out = run_batch(N, eng, w, check=False)
                runs.append((e2e, solve, res, out))
            best_e2e = min(r[0] for r in runs)
            best_solve = min(r[1] for r in runs)
            res, out = runs[-1][2], runs[-1][3]
            pivots = int(out["piv"].sum())
            rec = dict(workload=name, lps=count,
                       m=[int(w["m"].min()), int(w["m"].max())],
                       n=[int(w["n"].min()), int(w["n"].max())],
                       pivots=pivots, optimal=res.optimal, unbounded=res.unbounded,
                       limit=res.limit, launches=res.launches,
                       e2e_seconds=best_e2e, e2e_lps_per_s=count / best_e2e,
                       e2e_pivots_per_s=pivots / best_e2e,
                       solve_seconds=best_solve, solve_lps_per_s=count / best_solve,
                       solve_pivots_per_s=pivots / best_solve,
                       e2e_seconds_all=[r[0] for r in runs],
                       solve_seconds_all=[r[1] for r in runs])
            if not args.no_check:
                bad = bit_check(N, orc, w, offs, out)
                rec["bit_checked"] = min(CHECK, count)
                rec["bit_mismatches"] = bad
                failures += bad
                rec["single_model"] = single_loop(pkg, eng, w, offs, args.single_seconds, count)
                rec["cpu_oracle_1core"] = oracle_loop(orc, w, offs, args.oracle_seconds, count)
                rec["speedup_e2e_vs_single"] = rec["e2e_lps_per_s"] / \
                    rec["single_model"]["lps_per_s"]
            for r in runs:
                N.lib.lpr_batch_destroy(r[3]["h"])
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if failures:
        print(f"bit check: {failures} LP(s) differ from the oracle", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
