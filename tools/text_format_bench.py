"""Device text formatter on the three workloads of tools/batch_bench.py --trace (DESIGN.md section
25): W (the issue's S: 65 536 textbook LPs, every record), G (4 096 x 32 x 64, 16 records) and H
(256 x 256 x 512, 2 records).  Per workload one traced batch is solved once; then one warm-up
pass and --passes timed passes, all recorded, of
  (a) lpr_batch_trace_text alone: its kernel_ms (lpr_text_info) and the call's wall-clock;
  (b) end to end: FormatTrace() + the read-back of bytes and offsets + block(i) for every block.
The comparison is the parent's path on the same handle in the same process: IterationSnapshots(k)
(trace read + host Format) over an evenly spaced, time-bounded set of LPs, per block, labelled an
extrapolation when scaled to the batch.  --check LPs per workload, evenly spaced, are compared
string for string (IterationSnapshotsDevice(k) == IterationSnapshots(k)); the mismatch count is
recorded.  clears_bar: the slowest device pass per block is below the fastest host pass per block
on every workload.  With --parent-lib the untraced lpr_batch_solve of W is also timed against the
parent commit's library in alternating fresh processes (batch_bench.against_parent), and so is (a)
-- the kernel_ms of lpr_batch_trace_text on every workload, --parent-rounds fresh processes per
library, alternated; within_margin: this library's best is within the parent's best plus the
parent's own spread (its largest max - min over the passes of one process).  Appends one
JSON line per workload and a summary line to profiles/text_format_bench.json.

    python tools/text_format_bench.py [--workloads W,G,H] [--check 256] [--check-h 256]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import batch_bench as bb  # noqa: E402


def traced_batch(pkg, N, eng, w, name):
    """A solved traced PrimalSimplexBatch over the packed workload (created through the ABI as
    batch_bench does, then adopted by the Python class)."""
    count = len(w["n"])
    if bb.TRACE_CAP[name]:
        cap = bb.TRACE_CAP[name]
    else:  # every record: one untraced solve tells the most pivots
        _, _, _, out = bb.run_batch(N, eng, w, check=False)
        cap = 1 + int(out["piv"].max())
        N.lib.lpr_batch_destroy(out["h"])
    h = C.c_void_p()
    N.check(bb.create(N.lib, eng._h, w, h), "lpr_batch_from_lps")
    b = pkg.PrimalSimplexBatch.__new__(pkg.PrimalSimplexBatch)
    b._init(eng)
    b._attach(h, [(int(m) + 1, int(n) + int(m) + 1, int(n)) for n, m in zip(w["n"], w["m"])], 0)
    b.trace_reserve(cap)
    b.Solve(max_pivots=bb.CAP)
    return b, cap


def device_pass(b, eng):
    """One pass: (kernel_ms, seconds of the call, seconds end to end, blocks, bytes)."""
    b._text = None
    eng.sync()
    t0 = time.perf_counter()
    text = b.FormatTrace()
    t1 = time.perf_counter()
    n = 0
    for i in range(text.Count):
        n += len(text.block(i))
    t2 = time.perf_counter()
    assert n == text.Bytes
    out = (text.KernelMs, t1 - t0, t2 - t0, text.Count, text.Bytes)
    text.destroy()
    b._text = None
    return out


def host_passes(b, picks, passes, budget_s):
    """IterationSnapshots(k) over `picks`, `passes` times, each pass cut at budget_s: per pass
    (LPs done, blocks, seconds)."""
    out = []
    for _ in range(passes):
        done = blocks = 0
        t0 = time.perf_counter()
        for k in picks:
            blocks += len(b.IterationSnapshots(int(k)))
            done += 1
            if time.perf_counter() - t0 > budget_s:
                break
        out.append((done, blocks, time.perf_counter() - t0))
    return out


def trace_text_child(lib_path: str, names, seed: int, passes: int) -> int:
    """--trace-text-child: (a) alone with the engine library at lib_path (it may predate calls this
    package declares: what it lacks is not bound), one JSON line {workload: [kernel_ms, ...]}."""
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    if os.path.abspath(lib_path) != os.path.abspath(N.LIB_PATH):
        lib = C.CDLL(lib_path)
        for name, (res, argtypes) in N.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        N.lib = lib  # every call of the package goes through N.lib
    out = {}
    with pkg.Engine(0) as eng:
        for i, name in enumerate(names):
            b, _ = traced_batch(pkg, N, eng, bb.gen_workload(name, seed + i), name)
            ms = []
            for p in range(passes + 1):  # the first one warms up
                b._text = None
                eng.sync()
                text = b.FormatTrace()
                if p:
                    ms.append(text.KernelMs)
                text.destroy()
            b._text = None
            out[name] = ms
            b.destroy()
    print(json.dumps(out), flush=True)
    return 0


def trace_text_against_parent(args, names):
    import subprocess
    from lpr_381_group_v22_amd import _native as N
    runs = {"this": [], "parent": []}
    for _ in range(max(1, args.parent_rounds)):
        for tag, path in (("this", N.LIB_PATH), ("parent", args.parent_lib)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-text-child",
                                path, "--workloads", ",".join(names), "--seed", str(args.seed),
                                "--passes", str(args.passes)], capture_output=True, text=True,
                               timeout=900)
            if p.returncode != 0:
                raise RuntimeError(f"trace-text child on {path} failed: {p.stderr[-600:]}")
            runs[tag].append(json.loads(p.stdout.strip().splitlines()[-1]))
    out = {}
    for name in names:
        this = [t for r in runs["this"] for t in r[name]]
        parent = [t for r in runs["parent"] for t in r[name]]
        margin = max(max(r[name]) - min(r[name]) for r in runs["parent"])
        out[name] = dict(this_kernel_ms_by_process=[r[name] for r in runs["this"]],
                         parent_kernel_ms_by_process=[r[name] for r in runs["parent"]],
                         this_best=min(this), parent_best=min(parent),
                         parent_margin_max_minus_min=margin,
                         within_margin=min(this) <= min(parent) + margin)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="W,G,H")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--check", type=int, default=256, help="LPs compared per workload")
    ap.add_argument("--check-h", type=int, default=256, help="LPs compared of workload H")
    ap.add_argument("--host-seconds", type=float, default=4.0, help="budget of one host pass")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--trace-text-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_format_bench.json"))
    args = ap.parse_args()
    if args.trace_text_child:
        return trace_text_child(args.trace_text_child, args.workloads.split(","), args.seed,
                                args.passes)
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import _native as N
    lines, clears, mismatches = [], True, 0
    with pkg.Engine(0) as eng:
        for i, name in enumerate(args.workloads.split(",")):
            w = bb.gen_workload(name, args.seed + i)
            b, cap = traced_batch(pkg, N, eng, w, name)
            device_pass(b, eng)  # warm-up
            dev = [device_pass(b, eng) for _ in range(args.passes)]
            blocks, nbytes = dev[0][3], dev[0][4]
            n_check = min(args.check_h if name == "H" else args.check, b.Count)
            picks = np.linspace(0, b.Count - 1, n_check).astype(np.int64)
            host = host_passes(b, picks, args.passes, args.host_seconds)
            bad = sum(b.IterationSnapshotsDevice(int(k)) != b.IterationSnapshots(int(k))
                      for k in picks)
            mismatches += bad
            recs = b.trace_info()[0]
            cells = int(sum((min(int(recs[k]), cap) + (1 if b._ended(k) else 0)) * s[0] * s[1]
                            for k, s in enumerate(b._shapes)))
            b._text[1].destroy()
            b._text = None
            dev_per_block = max(d[2] for d in dev) / blocks
            host_per_block = min(h[2] / h[1] for h in host)
            clears = clears and dev_per_block < host_per_block
            rec = dict(workload=name, lps=b.Count, trace_cap=cap, blocks=blocks, text_bytes=nbytes,
                       cells=cells,
                       kernel_ms_all=[d[0] for d in dev],
                       call_seconds_all=[d[1] for d in dev],
                       e2e_seconds_all=[d[2] for d in dev],
                       text_bytes_per_s_kernel=nbytes / (min(d[0] for d in dev) / 1e3),
                       text_bytes_per_s_e2e=nbytes / min(d[2] for d in dev),
                       device_seconds_per_block_slowest=dev_per_block,
                       host_lps_blocks_seconds_all=host,
                       host_seconds_per_block_fastest=host_per_block,
                       host_seconds_whole_batch_extrapolated=host_per_block * blocks,
                       speedup_e2e_per_block=host_per_block / dev_per_block,
                       lps_compared=int(n_check), mismatches=int(bad))
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            b.destroy()
    summary = dict(mode="summary", clears_bar=bool(clears), mismatches=int(mismatches),
                   lps_compared=int(sum(r["lps_compared"] for r in lines)))
    if args.parent_lib:
        summary["untraced_solve_vs_parent"] = bb.against_parent(args, ["W"])["W"]
        summary["trace_text_kernel_ms_vs_parent"] = trace_text_against_parent(
            args, args.workloads.split(","))
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    with open(args.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    return 0 if mismatches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
