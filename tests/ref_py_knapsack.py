"""Independent pure-Python restatement of the knapsack menu option (TEST ONLY): the 0/1 DP of
KnapsackBranchBoundSolver.Solve and the level-synchronous branch-and-bound of
KnapsackBranchBoundSimplex, written from the rules of DESIGN.md section 11 (the reference has no
C# lines for either class).  Does not import the product.

Node records are tuples (parent, branch, status, bound, k, V): parent is the record index of the
parent (-1 for the root), branch 0 for child ".1" (x_k = 0) and 1 for child ".2" (x_k = 1), k the
critical item's RANK position (-1 when there is none to report), V the candidate value.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

FRACTIONAL, PRUNED, INTEGRAL, INFEASIBLE = 0, 1, 2, 3
STATUS_TEXT = {FRACTIONAL: "fractional", PRUNED: "fractional, pruned", INTEGRAL: "integral",
               INFEASIBLE: "infeasible"}
DEFAULT_NODE_CAP = 1 << 22
OK, NODE_CAP = 0, 6


def dp(capacity: int, weights: Sequence[int], values: Sequence[int]) -> int:
    """max sum v over subsets with sum w <= capacity; row initialised to 0 (the empty set)."""
    if capacity < 0 or any(w < 0 for w in weights):
        raise ValueError("negative capacity or weight")
    row = [0] * (capacity + 1)
    for w, v in zip(weights, values):
        if w > capacity:
            continue
        for c in range(capacity, w - 1, -1):
            t = row[c - w] + v
            if t > row[c]:
                row[c] = t
    return row[capacity]


def rank_items(weights: Sequence[int], values: Sequence[int]) -> List[int]:
    """rank[p] = original index of rank position p: v/w descending, compared as v_i*w_j against
    v_j*w_i, ties to the lower original index."""
    def cmp(i, j):
        a, b = values[i] * weights[j], values[j] * weights[i]
        if a != b:
            return -1 if a > b else 1
        return -1 if i < j else (1 if i > j else 0)
    return sorted(range(len(weights)), key=functools.cmp_to_key(cmp))


def relax(C: int, w: Sequence[int], v: Sequence[int], f1: set, f0: set):
    """Relaxation of one node over rank-ordered w, v.  Returns (status, bound, k, V, stop):
    stop is the rank position where the greedy walk stopped (n when it took every free item)."""
    n = len(w)
    R = C - sum(w[p] for p in f1)
    V = sum(v[p] for p in f1)
    if R < 0:
        return INFEASIBLE, 0.0, -1, 0, n
    k = -1
    for p in range(n):
        if p in f1 or p in f0:
            continue
        if w[p] <= R:
            R -= w[p]
            V += v[p]
        else:
            k = p
            break
    stop = n if k < 0 else k
    if k < 0 or R == 0:
        return INTEGRAL, float(V), -1, V, stop
    q = float(R) / float(w[k])
    t = float(v[k]) * q
    return FRACTIONAL, float(V) + t, k, V, stop


def branch_and_bound(capacity: int, weights: Sequence[int], values: Sequence[int],
                     node_cap: int = DEFAULT_NODE_CAP, records: bool = True):
    """The level-synchronous search.  Returns a dict: status, z (None when no incumbent),
    selected (ascending original indices), rank, records, evaluated, levels, widest."""
    n = len(weights)
    rank = rank_items(weights, values)
    w = [weights[i] for i in rank]
    v = [values[i] for i in rank]
    frontier = [(-1, 0, frozenset(), frozenset())]  # (parent record, branch, F1, F0)
    recs: List[Tuple[int, int, int, float, int, int]] = []
    z: Optional[int] = None
    inc = None
    evaluated = levels = widest = 0
    status = OK
    while frontier:
        if evaluated + len(frontier) > node_cap:
            status = NODE_CAP
            break
        base = evaluated
        evals = [relax(capacity, w, v, f1, f0) for (_, _, f1, f0) in frontier]
        evaluated += len(frontier)
        levels += 1
        widest = max(widest, len(frontier))
        best = -1
        for i, e in enumerate(evals):
            if e[0] != INFEASIBLE and (best < 0 or e[3] > evals[best][3]):
                best = i
        if best >= 0 and (z is None or evals[best][3] > z):
            z = evals[best][3]
            inc = (frontier[best][2], frontier[best][3], evals[best][4])
        nxt = []
        for i, ((par, br, f1, f0), e) in enumerate(zip(frontier, evals)):
            st = e[0]
            if st == FRACTIONAL:
                if e[1] > z:
                    k = e[2]
                    nxt.append((base + i, 0, f1, f0 | {k}))
                    nxt.append((base + i, 1, f1 | {k}, f0))
                else:
                    st = PRUNED
            if records:
                recs.append((par, br, st, e[1], e[2], e[3]))
        frontier = nxt
    selected: List[int] = []
    if inc is not None:
        f1, f0, stop = inc
        selected = sorted(rank[p] for p in range(n) if p in f1 or (p < stop and p not in f0))
    return {"status": status, "z": z, "selected": selected, "rank": rank, "records": recs,
            "evaluated": evaluated, "levels": levels, "widest": widest}


def labels(records) -> List[str]:
    """Node labels: root "0", its children "1" / "2", the children of "1" "1.1" / "1.2"."""
    out: List[str] = []
    for par, br, *_ in records:
        if par < 0:
            out.append("0")
        else:
            out.append(("" if par == 0 else out[par] + ".") + str(br + 1))
    return out


def brute_force(capacity: int, weights: Sequence[int], values: Sequence[int]) -> int:
    n = len(weights)
    best = 0
    for m in range(1 << n):
        sw = sv = 0
        for i in range(n):
            if m >> i & 1:
                sw += weights[i]
                sv += values[i]
        if sw <= capacity and sv > best:
            best = sv
    return best
