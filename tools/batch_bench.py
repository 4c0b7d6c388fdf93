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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="W,G,H")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--single-seconds", type=float, default=5.0)
    ap.add_argument("--oracle-seconds", type=float, default=5.0)
    ap.add_argument("--no-check", action="store_true", help="skip the bit check and the loops")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

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
