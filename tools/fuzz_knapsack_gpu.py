#!/usr/bin/env python3
"""Time-bounded randomised comparison of the knapsack engine (menu option 5) on the device with the
restatement tests/ref_py_knapsack.py: status, Z*, selected ids, counters, rank and every kept node
record (bounds by bits), i.e. all that tests/test_knapsack_gpu.py compares; on draws with n <= 64
also lpr_knap_dp (both variants) against numpy at a capacity of at most 20 000:

    python tools/fuzz_knapsack_gpu.py [--seconds 120] [--seed 1]

Instance i is drawn from random.Random(seed + i) alone.  The first mismatch prints that seed and the
case as a Python literal and exits non-zero.  One engine, no child processes."""
import argparse
import math
import random
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ref_py_knapsack as K  # noqa: E402
from test_knapsack_gpu import compare_with_ref, np_dp  # noqa: E402
import lpr_381_group_v22_amd as pkg  # noqa: E402
from lpr_381_group_v22_amd.knapsack import KnapsackBranchBoundSimplex, knapsack_dp  # noqa: E402

TOP = (1 << 31) - 1


def draw(seed):
    """The case of one seed: dict(C, w, v, node_cap, narrate)."""
    rng = random.Random(seed)
    huge = rng.randrange(50) == 0
    if huge:
        n = rng.randint(1000, 8192)
    else:
        n = min(300, int(math.exp(rng.uniform(0.0, math.log(301.0)))))
    top = rng.choice([10, 1000, 1 << 16, TOP])
    rule = rng.choice(["independent", "offset", "multiple", "some_zero"])
    if rule == "multiple":
        c = rng.choice([1, 2, 3])
        w = [rng.randint(1, max(1, top // c)) for _ in range(n)]
        v = [c * x for x in w]
    else:
        w = [rng.randint(1, top) for _ in range(n)]
        if rule == "offset":
            c = rng.randint(0, max(1, top // 8))
            v = [min(TOP, x + c) for x in w]
        else:
            v = [rng.randint(0, top) for _ in range(n)]
            if rule == "some_zero":
                v = [0 if rng.randrange(3) == 0 else x for x in v]
    total = sum(w)
    C = rng.choice([0, rng.randint(0, total), total, total + 1])
    node_cap = 300 if huge else rng.choice([rng.randint(1, 600), 20000])
    narrate = rng.choice([0, rng.randint(1, 64), node_cap])
    return dict(C=C, w=w, v=v, node_cap=node_cap, narrate=narrate)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    eng = pkg.Engine(0)
    t_end = time.time() + args.seconds
    seed = args.seed
    instances = nodes = records = dps = multiword = capped = 0
    while time.time() < t_end:
        case = draw(seed)
        C, w, v = case["C"], case["w"], case["v"]
        try:
            r = K.branch_and_bound(C, w, v, node_cap=case["node_cap"])
            s = KnapsackBranchBoundSimplex(C, [float(x) for x in w], [float(x) for x in v],
                                           engine=eng, node_cap=case["node_cap"],
                                           narrate=case["narrate"])
            s.Solve()
            compare_with_ref(s, r, case["narrate"])
            records += len(s.Nodes())
            s.destroy()
            if len(w) <= 64:
                Cd = min(C, 20000)
                want = np_dp(Cd, w, v)
                for variant in (0, 1):
                    got = knapsack_dp(Cd, w, v, engine=eng, variant=variant)
                    assert got == want, f"DP variant {variant} at C = {Cd}: {got}, numpy {want}"
                dps += 1
        except AssertionError as exc:
            print(f"MISMATCH at seed {seed}: {exc}")
            print(f"case = {case!r}")
            eng.close()
            return 1
        instances += 1
        nodes += r["evaluated"]
        multiword += len(w) > 64
        capped += r["status"] == K.NODE_CAP
        seed += 1
        if instances % 200 == 0:
            print(f"{instances} instances, seed {seed}, {nodes} nodes", flush=True)
    print(f"OK: {instances} instances (seeds {args.seed}..{seed - 1}; {multiword} with n > 64, "
          f"{capped} stopped by the node cap), {nodes} nodes evaluated, {records} node records and "
          f"{dps} DP pairs compared, 0 mismatches")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
