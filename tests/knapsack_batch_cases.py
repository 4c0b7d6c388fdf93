"""Instances for the CPU and GPU tests of the knapsack batch (TEST ONLY).
An instance is a dict with name, C, w, v, node_cap, like those of tests/knapsack_cases.py, whose
cases are all part of the main batch here.  tests/test_knapsack_batch_cpu.py asserts on the
restatement (tests/ref_py_knapsack.py) that the instances have the properties the GPU tests rely
on; tests/test_knapsack_batch_gpu.py compares the device with the restatement.  The footprint
formula is restated here from DESIGN.md section 16.  Does not import the product.
"""
from __future__ import annotations

import functools
import random
from typing import Dict, List, Sequence, Tuple

import knapsack_cases as KC
import ref_py_knapsack as K

SAMPLE = (40, [11, 8, 6, 14, 10, 10], [2, 3, 3, 5, 2, 4])   # section 11: 3 levels, 5 nodes
SAMPLE_EVALUATED = 5

FORM_W, FORM_G, FORM_H = 0, 1, 2
DEFAULT_CAP = 1024
# DESIGN.md section 16 (the LDS limits are section 12's)
MAX_LDS_W = (64 * 1024 - 1024) // 4   # 16 128 bytes: a quarter of 64 KiB less the scratch
MAX_LDS_G = 160 * 1024 - 1024         # 162 816 bytes
DP_CELLS_W = MAX_LDS_W // 8           # 2 016 int64 cells
DP_CELLS_G = MAX_LDS_G // 8           # 20 352
DP_CHUNK_W, DP_CHUNK_G = 64 * 4, 256 * 4
DP_MAX_CELLS = 1 << 22


def footprint(n: int, node_cap: int) -> int:
    """Bytes of one instance: per node two frontier entries (F1 and F0 of ceil(n / 64) words, a
    parent index) and the level's results (V, bound, stop, status); the ranked w, v as 32-bit."""
    nw = (n + 63) // 64
    return node_cap * (2 * (2 * nw * 8 + 4) + (8 + 8 + 4 + 4)) + n * 2 * 4


def form_of(n: int, node_cap: int, variant: int = 0) -> int:
    fp = footprint(n, node_cap)
    fit_w, fit_g = fp <= MAX_LDS_W, fp <= MAX_LDS_G
    if variant == 1 and fit_w:
        return FORM_W
    if variant == 2 and fit_g:
        return FORM_G
    if variant == 3:
        return FORM_H
    return FORM_W if fit_w else (FORM_G if fit_g else FORM_H)


def _case(name: str, C: int, w: Sequence[int], v: Sequence[int], node_cap: int, **props) -> Dict:
    return dict(name=name, C=C, w=list(w), v=list(v), node_cap=node_cap, **props)


def sample(node_cap: int, tag: str = "") -> Dict:
    return _case(f"sample_cap{node_cap}{tag}", SAMPLE[0], SAMPLE[1], SAMPLE[2], node_cap)


def strongly_correlated(seed: int, n: int, node_cap: int, hi: int = 1000) -> Dict:
    rng = random.Random(seed)
    w = [rng.randint(1, hi) for _ in range(n)]
    return _case(f"sc_s{seed}_n{n}_cap{node_cap}", sum(w) // 2, w, [x + 100 for x in w], node_cap)


def small_random(seed: int, n: int, node_cap: int, hi: int = 20) -> Dict:
    rng = random.Random(seed)
    w = [rng.randint(1, hi) for _ in range(n)]
    v = [rng.randint(0, hi) for _ in range(n)]
    return _case(f"small_s{seed}_n{n}_cap{node_cap}", max(1, sum(w) // 2), w, v, node_cap)


def lds_cases() -> List[Dict]:
    """Instances that fit LDS, to stand next to knapsack_cases' (whose node caps of 600 and more
    put every one of them in form H): W and G, finishing and stopped, one and two bitmap words."""
    return [
        sample(SAMPLE_EVALUATED, "_exact"),          # evaluated + width == cap at the last level: W
        sample(64),                                  # W, finishes
        strongly_correlated(11, 30, 200),            # W (64 * 200 + 240 bytes), stopped by the cap
        strongly_correlated(12, 40, 2000),           # G, wide levels, stopped
        strongly_correlated(13, 64, 150),            # W, n = 64: the full word
        strongly_correlated(13, 65, 150),            # W, n = 65: two words, a wave per node
        strongly_correlated(14, 130, 1200),          # G, three words
        small_random(15, 10, DEFAULT_CAP),           # G at the default cap (65 616 bytes)
    ]


@functools.lru_cache(maxsize=None)
def main_batch() -> Tuple[Dict, ...]:
    """The whole of knapsack_cases.all_cases() at their own caps, interleaved with lds_cases()."""
    big = list(KC.all_cases())
    small = lds_cases()
    out: List[Dict] = []
    step = max(1, len(big) // len(small))
    for i, c in enumerate(big):
        if i % step == 0 and small:
            out.append(small.pop(0))
        out.append(c)
    out.extend(small)
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _ref(C: int, w: Tuple[int, ...], v: Tuple[int, ...], node_cap: int) -> Dict:
    return K.branch_and_bound(C, list(w), list(v), node_cap=node_cap)


def reference(case: Dict, node_cap: int = -1) -> Dict:
    """The restatement's run of an instance at its own cap (or the one given), computed once per
    process and shared; callers must not change it.  knapsack_cases' instances share that
    module's cache."""
    cap = case["node_cap"] if node_cap < 0 else node_cap
    if case["name"] in KC.case_names():
        return KC.reference(case["name"], -1 if cap == case["node_cap"] else cap)
    return _ref(case["C"], tuple(case["w"]), tuple(case["v"]), cap)


def limit_cases() -> List[Tuple[Dict, int]]:
    """(instance, form): n = 8 and the node caps whose footprint is one node below, at and one
    node past the W limit (64 cap + 64 = 16 128 at cap 251) and the G limit (162 816 at 2 543)."""
    out = []
    for cap, form in ((250, FORM_W), (251, FORM_W), (252, FORM_G),
                      (2542, FORM_G), (2543, FORM_G), (2544, FORM_H)):
        c = strongly_correlated(20 + cap % 7, 8, cap, hi=50)
        out.append((c, form))
    return out


def cap_cases() -> List[Dict]:
    """Instances that finish, for the runs at node caps of E, E - 1, E + 1 and after the root: one
    of knapsack_cases (form H at those caps) and one whose caps fit LDS."""
    return [KC.by_name("wide_mixed_small"), small_random(15, 10, DEFAULT_CAP)]


def form_order_cases() -> List[Dict]:
    """One instance per form, in the order H, W, G."""
    return [strongly_correlated(31, 24, 5000), sample(32), strongly_correlated(32, 24, 1000)]


def dp_edge_cases() -> List[Dict]:
    """C = 0; C + 1 at and beside the W and G row limits and the chunk sizes; an item with w = C
    and one with w = C + 1; all values 0."""
    rng = random.Random(40)
    out = [_case("dp_c0", 0, [1, 2, 3], [5, 6, 7], 8)]
    cells = sorted({DP_CHUNK_W - 1, DP_CHUNK_W, DP_CHUNK_W + 1, DP_CHUNK_G - 1, DP_CHUNK_G,
                    DP_CHUNK_G + 1, DP_CELLS_W - 1, DP_CELLS_W, DP_CELLS_W + 1, DP_CELLS_G - 1,
                    DP_CELLS_G, DP_CELLS_G + 1})
    for m in cells:
        C = m - 1
        w = [rng.randint(1, max(2, C // 3)) for _ in range(12)]
        v = [rng.randint(0, 1000) for _ in range(12)]
        out.append(_case(f"dp_cells{m}", C, w, v, 8))
    C = 700
    out.append(_case("dp_w_is_c", C, [C, 3, 5, 691], [1000, 2, 3, 990], 8))
    out.append(_case("dp_w_is_c_plus_1", C, [C + 1, 300, 400, 2], [10 ** 6, 7, 8, 1], 8))
    out.append(_case("dp_values_zero", 500, [rng.randint(1, 90) for _ in range(9)], [0] * 9, 8))
    return out


def pack(cases: Sequence[Dict]):
    """(capacities, weights, values, node_caps) for KnapsackBatch."""
    return ([c["C"] for c in cases], [c["w"] for c in cases], [c["v"] for c in cases],
            [c["node_cap"] for c in cases])
