"""Knapsack branch-and-bound instances for the CPU and GPU tests of menu option 5 (TEST ONLY).
Every instance is drawn by a seeded random.Random and is a dict with name, family, C, w, v,
node_cap, plus the properties it is meant to have; tests/test_knapsack_cpu.py asserts those on the
restatement (tests/ref_py_knapsack.py), tests/test_knapsack_gpu.py compares the device with the
restatement record by record on the same instances.  Does not import the product.

What the families reach that w, v <= 1000 and n <= 200 do not:
  big               sums over 2^32: the high halves of the 64-bit wave shuffles
  big_multiword     n > 64: the scan's carry of R across 64-item chunks, k in a word >= 1
  sc_multiword      the same with small numbers and deep searches (strongly correlated)
  max_items(_late)  n = 8192 and 8129 (a partial last word), k in a late or the last word
  wide_mixed        levels over 1024 and 2048 wide with branched and pruned nodes mixed: the
                    stable compaction inside and across the 1024-node steps of the level kernel
  all_branch_wide   every ratio ties, every node of a wide level branches
  degenerate        the rules' corner cases
"""
from __future__ import annotations

import functools
import random
from typing import Dict, List, Tuple

import ref_py_knapsack as K

BIG_LO, BIG_HI = 1 << 30, (1 << 31) - 1
TWO32 = 1 << 32


def _big(rng: random.Random, n: int) -> List[int]:
    return [rng.randint(BIG_LO, BIG_HI) for _ in range(n)]


def _small(rng: random.Random, n: int) -> List[int]:
    return [rng.randint(1, 1000) for _ in range(n)]


def _case(family: str, tag: str, C: int, w, v, node_cap: int, **props) -> Dict:
    return dict(name=f"{family}_{tag}", family=family, C=C, w=list(w), v=list(v),
                node_cap=node_cap, **props)


# seeds of the two wide_mixed instances, found by scanning seeds 0.. on the CPU for the first at
# which the family's property holds and the search also finishes inside the node cap, so that the
# default cap runs the same search (test_knapsack_cpu.py asserts both still hold)
WIDE_MIXED_SEED_SMALL = 2
WIDE_MIXED_SEED_BIG = 4


def big_cases() -> List[Dict]:
    out = []
    for n in (1, 6, 12, 20):
        rng = random.Random(1000 + n)
        w, v = _big(rng, n), _big(rng, n)
        out.append(_case("big", f"n{n}", sum(w) // 2, w, v, 20000, status=K.OK))
    return out


def big_multiword_cases() -> List[Dict]:
    out = []
    for n in (64, 65, 128, 129, 200):
        rng = random.Random(2000 + n)
        w, v = _big(rng, n), _big(rng, n)
        out.append(_case("big_multiword", f"n{n}", sum(w) // 2, w, v, 20000, status=K.OK,
                         k_min=64 if n > 64 else None))
    return out


def sc_multiword_cases() -> List[Dict]:
    out = []
    for n in (65, 129, 200):
        rng = random.Random(3000 + n)
        w = _small(rng, n)
        v = [x + 100 for x in w]
        out.append(_case("sc_multiword", f"n{n}", sum(w) // 2, w, v, 20000,
                         status=K.NODE_CAP if n > 65 else None, k_min=64))
    return out


def max_items_cases() -> List[Dict]:
    out = []
    for n in (8192, 8129):
        rng = random.Random(4000 + n)
        w, v = _big(rng, n), _big(rng, n)
        out.append(_case("max_items", f"n{n}", sum(w) // 2, w, v, 600, status=K.NODE_CAP,
                         k_min=64 * 64))
        out.append(_case("max_items_late", f"n{n}", sum(w) - (1 << 31), w, v, 600,
                         k_min=n - 64))
    return out


def wide_mixed_cases() -> List[Dict]:
    rng = random.Random(WIDE_MIXED_SEED_SMALL)
    w = _small(rng, 40)
    small = _case("wide_mixed", "small", sum(w) // 2, w, [x + 100 for x in w], 40000,
                  status=K.OK)
    rng = random.Random(WIDE_MIXED_SEED_BIG)
    w = [rng.randint(BIG_LO, BIG_HI - (1 << 27)) for _ in range(40)]  # v = w + 2^27 <= 2^31 - 1
    big = _case("wide_mixed", "big", sum(w) // 2, w, [x + (1 << 27) for x in w], 40000,
                status=K.OK)
    return [small, big]


def all_branch_wide_cases() -> List[Dict]:
    rng = random.Random(6000)
    w = _big(rng, 30)
    out = [_case("all_branch_wide", "n30", sum(w) // 2, w, w, 32767, status=K.NODE_CAP)]
    # the same with only six distinct weights: many nodes of a level share the largest V, and
    # the first of them must become the incumbent
    rng = random.Random(8)
    kinds = _big(rng, 6)
    w = [rng.choice(kinds) for _ in range(30)]
    out.append(_case("all_branch_wide", "ties", sum(w) // 2, w, w, 32767, status=K.NODE_CAP,
                     tied_incumbent=True))
    return out


def degenerate_cases() -> List[Dict]:
    """z and selected are worked out here from the rules, not taken from the restatement."""
    rng = random.Random(7000)
    out = []
    # every value 0: all ratios tie, the rank is the identity, the root's bound V + 0 * q = 0 does
    # not exceed Z* = 0, so the root is pruned and the candidate is its greedy prefix
    w = _small(rng, 10)
    C = sum(w) // 2
    taken, R = [], C
    for i, x in enumerate(w):
        if x > R:
            break
        R -= x
        taken.append(i)
    out.append(_case("degenerate", "all_values_zero", C, w, [0] * 10, 20000, status=K.OK, z=0,
                     selected=taken, evaluated=1))
    # C = 0: the first item does not fit and R == 0: integral root with nothing taken
    w, v = _big(rng, 7), _big(rng, 7)
    out.append(_case("degenerate", "zero_capacity", 0, w, v, 20000, status=K.OK, z=0, selected=[],
                     evaluated=1))
    # C >= sum w: the walk takes every item; integral root, stop = n
    for tag, n in (("capacity_is_sum", 70), ("capacity_2_60", 130)):
        w, v = _big(rng, n), _big(rng, n)
        C = sum(w) if tag == "capacity_is_sum" else 1 << 60
        out.append(_case("degenerate", tag, C, w, v, 20000, status=K.OK, z=sum(v),
                         selected=list(range(n)), evaluated=1))
    # one item heavier than the capacity, with the best ratio: it is k at the root and can only
    # ever be left out (the z comes from brute force in the CPU test)
    w, v = _small(rng, 8), _small(rng, 8)
    C = sum(w) // 2
    w[3], v[3] = C + 1, BIG_HI
    out.append(_case("degenerate", "one_item_over_capacity", C, w, v, 20000, status=K.OK,
                     never_selected=3))
    out.append(_case("degenerate", "n1_fits", BIG_HI, [BIG_HI], [BIG_HI - 1], 20000, status=K.OK,
                     z=BIG_HI - 1, selected=[0], evaluated=1))
    out.append(_case("degenerate", "n1_does_not_fit", BIG_HI - 1, [BIG_HI], [BIG_HI], 20000,
                     status=K.OK, z=0, selected=[]))
    return out


@functools.lru_cache(maxsize=None)
def _all() -> Tuple[Dict, ...]:
    cases = (big_cases() + big_multiword_cases() + sc_multiword_cases() + max_items_cases() +
             wide_mixed_cases() + all_branch_wide_cases() + degenerate_cases())
    assert len({c["name"] for c in cases}) == len(cases)
    return tuple(cases)


def all_cases() -> Tuple[Dict, ...]:
    return _all()


def case_names() -> List[str]:
    return [c["name"] for c in _all()]


def by_name(name: str) -> Dict:
    return next(c for c in _all() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def reference(name: str, node_cap: int = -1) -> Dict:
    """The restatement's run of a case (at the case's own node_cap unless one is given), computed
    once per process and shared; callers must not change it."""
    c = by_name(name)
    return K.branch_and_bound(c["C"], c["w"], c["v"],
                              node_cap=c["node_cap"] if node_cap < 0 else node_cap)


def level_split(records) -> List[Tuple[int, int, int]]:
    """(first record, width, branched) of every level, walking the records by W -> 2 * branched.
    The last level may be cut short by a log that kept fewer records than were evaluated."""
    out = []
    base, W = 0, 1
    while W > 0 and base < len(records):
        level = records[base:base + W]
        branched = sum(1 for rec in level if rec[2] == K.FRACTIONAL)
        out.append((base, W, branched))
        base += W
        W = 2 * branched
    return out


def level_of(records, index: int) -> Tuple[int, int, int]:
    """(level number, first record of the level, width) of record `index`."""
    for lv, (base, W, _) in enumerate(level_split(records)):
        if index < base + W:
            return lv, base, W
    raise IndexError(index)


def mixed_wide_levels(records, width: int = 1024, share: float = 0.25) -> List[Tuple[int, int, int]]:
    """The levels wider than `width` in which the branched and the not-branched nodes are each
    more than `share` of the level."""
    return [(base, W, b) for (base, W, b) in level_split(records)
            if W > width and b > share * W and (W - b) > share * W]
