"""Many knapsack instances in one call (``lpr_knap_batch_*``): option 5
(``Program.cs:430-470``) for a whole batch.  One ``Solve()`` runs the level-synchronous
branch-and-bound of section 11 for every instance on the device, one ``DP()`` the 0/1 DP of every
instance.  Instance k gets what ``KnapsackBranchBoundSimplex`` gives for it alone at the same
``node_cap``.  All numbers come from the device; this file is packing and text.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from ._native import _ptr
from .engine import Engine, default_engine
from .knapsack import KnapsackNode, narration_lines

VARIANT_AUTO, VARIANT_W, VARIANT_G, VARIANT_H = 0, 1, 2, 3   # lpr_knap_batch_opts.variant
FORM_W, FORM_G, FORM_H = 0, 1, 2

DEFAULT_NODE_CAP = 1024          # kKnapBatchDefaultCap
MAX_NODE_CAP = 1 << 22           # kKnapBatchMaxCap
MAX_ITEMS = 8192                 # kKnapMaxItems
DP_MAX_CELLS = 1 << 22           # kKnapBatchDpMaxCells
MAX_LDS_W = ((64 << 10) - (1 << 10)) // 4   # kBatchMaxLdsW
MAX_LDS_G = (160 << 10) - (1 << 10)         # kBatchMaxLdsG


def footprint(n: int, node_cap: int) -> int:
    """Bytes an instance needs (knap_batch_footprint): per node two frontier buffers of two
    bitmaps and a parent each, plus V, bound, stop and status; the ranked items as 32-bit words."""
    nw = (n + 63) // 64
    return node_cap * (2 * (2 * nw * 8 + 4) + 24) + 8 * n


def form_of(n: int, node_cap: int, variant: int = VARIANT_AUTO) -> int:
    """The form batch_pick_form gives an instance."""
    fp = footprint(n, node_cap)
    fit_w, fit_g = fp <= MAX_LDS_W, fp <= MAX_LDS_G
    if variant == VARIANT_W and fit_w:
        return FORM_W
    if variant == VARIANT_G and fit_g:
        return FORM_G
    if variant == VARIANT_H:
        return FORM_H
    return FORM_W if fit_w else (FORM_G if fit_g else FORM_H)


class PackedKnapsacks(NamedTuple):
    """The packed arrays of lpr_knap_batch_create."""
    capacity: np.ndarray   # int64[count]
    n: np.ndarray          # int32[count]
    weights: np.ndarray    # float64, packed by n
    values: np.ndarray
    node_cap: np.ndarray   # int64[count]
    offsets: np.ndarray    # int64[count + 1]: instance k's items are [offsets[k], offsets[k + 1])


def pack_knapsacks(capacities: Sequence[int], weights: Sequence[Sequence[float]],
                   values: Sequence[Sequence[float]],
                   node_cap=None) -> PackedKnapsacks:
    """Instances -> the packed ABI arrays, with the shape checks of lpr_knap_batch_create (raises
    ValueError naming the instance).  node_cap: None, one int for all, or one per instance."""
    count = len(capacities)
    if count < 1 or len(weights) != count or len(values) != count:
        raise ValueError("capacities, weights and values must list the same instances (>= 1)")
    if node_cap is None:
        caps = [0] * count
    elif np.isscalar(node_cap):
        caps = [int(node_cap)] * count
    else:
        caps = [int(c) for c in node_cap]
        if len(caps) != count:
            raise ValueError("node_cap must have one entry per instance")
    ns = []
    for k in range(count):
        if len(weights[k]) != len(values[k]):
            raise ValueError(f"instance {k}: weights and values differ in length")
        if not 1 <= len(weights[k]) <= MAX_ITEMS:
            raise ValueError(f"instance {k}: n = {len(weights[k])} is outside 1..{MAX_ITEMS}")
        if int(capacities[k]) < 0:
            raise ValueError(f"instance {k}: capacity {capacities[k]} < 0")
        if caps[k] > MAX_NODE_CAP:
            raise ValueError(f"instance {k}: node_cap {caps[k]} is over 2^22")
        ns.append(len(weights[k]))
    off = np.zeros(count + 1, dtype=np.int64)
    np.cumsum(ns, out=off[1:])
    w = np.concatenate([np.asarray(x, dtype=np.float64) for x in weights])
    v = np.concatenate([np.asarray(x, dtype=np.float64) for x in values])
    return PackedKnapsacks(np.asarray([int(c) for c in capacities], dtype=np.int64),
                           np.asarray(ns, dtype=np.int32), np.ascontiguousarray(w),
                           np.ascontiguousarray(v), np.asarray(caps, dtype=np.int64), off)


class KnapsackBatch:
    """``count`` knapsack instances in one device handle (lpr_knap_batch_*).

    node_cap: evaluated nodes per instance (None / 0: 1024; the single engine's default is 2^22,
    so pass the same cap to both when comparing).  narrate: node records kept per instance."""

    def __init__(self, capacities: Sequence[int], weights: Sequence[Sequence[float]],
                 values: Sequence[Sequence[float]], node_cap=None, narrate: int = 0,
                 engine: Optional[Engine] = None):
        self.engine = engine or default_engine()
        self._p = p = pack_knapsacks(capacities, weights, values, node_cap)
        self.count = len(p.n)
        self.narrate = int(narrate)
        self.node_caps = [int(c) if c > 0 else DEFAULT_NODE_CAP for c in p.node_cap]
        self.result: Optional[N.KnapBatchResult] = None
        self._res: Optional[Dict[str, np.ndarray]] = None
        h = C.c_void_p()
        N.check(N.lib.lpr_knap_batch_create(
            self.engine._h, self.count, _ptr(p.capacity, C.c_int64), _ptr(p.n, C.c_int32),
            _ptr(p.weights, C.c_double), _ptr(p.values, C.c_double), _ptr(p.node_cap, C.c_int64),
            self.narrate, C.byref(h)), "lpr_knap_batch_create")
        self._h = h

    def destroy(self) -> None:
        if getattr(self, "_h", None):
            N.lib.lpr_knap_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def Solve(self, chunk: int = 0, variant: int = VARIANT_AUTO) -> N.KnapBatchResult:
        """The search of every instance from its root; returns the call's counts."""
        opts = N.KnapBatchOpts(chunk=int(chunk), variant=int(variant))
        res = N.KnapBatchResult()
        N.check(N.lib.lpr_knap_batch_solve(self._h, C.byref(opts), C.byref(res)),
                "lpr_knap_batch_solve")
        self.result = res
        self._res = None
        return res

    def Stats(self) -> Dict[str, np.ndarray]:
        """status, found, z, evaluated, widest, levels: one array of ``count`` entries each."""
        if self._res is None:
            out = {"status": np.zeros(self.count, np.int32), "found": np.zeros(self.count, np.int32),
                   "z": np.zeros(self.count, np.float64),
                   "evaluated": np.zeros(self.count, np.int64),
                   "widest": np.zeros(self.count, np.int64),
                   "levels": np.zeros(self.count, np.int32)}
            N.check(N.lib.lpr_knap_batch_result_read(
                self._h, _ptr(out["status"], C.c_int32), _ptr(out["found"], C.c_int32),
                _ptr(out["z"], C.c_double), _ptr(out["evaluated"], C.c_int64),
                _ptr(out["widest"], C.c_int64), _ptr(out["levels"], C.c_int32)),
                "lpr_knap_batch_result_read")
            self._res = out
        return self._res

    def Status(self) -> List[int]:
        return self.Stats()["status"].tolist()

    def Z(self) -> List[Optional[float]]:
        """Z* per instance, None where no incumbent was found."""
        s = self.Stats()
        return [float(z) if f else None for z, f in zip(s["z"], s["found"])]

    def Rank(self) -> List[List[int]]:
        r = np.zeros(int(self._p.offsets[-1]), dtype=np.int32)
        N.check(N.lib.lpr_knap_batch_rank_read(self._h, _ptr(r, C.c_int32)),
                "lpr_knap_batch_rank_read")
        o = self._p.offsets
        return [r[o[k]:o[k + 1]].tolist() for k in range(self.count)]

    def SelectedIds(self) -> List[List[int]]:
        ids = np.zeros(int(self._p.offsets[-1]), dtype=np.int32)
        cnt = np.zeros(self.count, dtype=np.int32)
        N.check(N.lib.lpr_knap_batch_selected_read(self._h, _ptr(ids, C.c_int32),
                                                    _ptr(cnt, C.c_int32)),
                "lpr_knap_batch_selected_read")
        o = self._p.offsets
        return [ids[o[k]:o[k] + cnt[k]].tolist() for k in range(self.count)]

    def Nodes(self, k: int) -> List[KnapsackNode]:
        cnt = C.c_int64()
        N.check(N.lib.lpr_knap_batch_nodes_read(self._h, int(k), None, None, None, None, None,
                                                 None, 0, C.byref(cnt)),
                "lpr_knap_batch_nodes_read")
        m = cnt.value
        par, br, st, kk = (np.zeros(max(m, 1), dtype=np.int32) for _ in range(4))
        bd = np.zeros(max(m, 1), dtype=np.float64)
        V = np.zeros(max(m, 1), dtype=np.int64)
        N.check(N.lib.lpr_knap_batch_nodes_read(
            self._h, int(k), _ptr(par, C.c_int32), _ptr(br, C.c_int32), _ptr(st, C.c_int32),
            _ptr(bd, C.c_double), _ptr(kk, C.c_int32), _ptr(V, C.c_int64), m, C.byref(cnt)),
            "lpr_knap_batch_nodes_read")
        return [KnapsackNode(p, b, s, d, q, x) for p, b, s, d, q, x in
                zip(par[:m].tolist(), br[:m].tolist(), st[:m].tolist(), bd[:m].tolist(),
                    kk[:m].tolist(), V[:m].tolist())]

    def IterationLines(self, k: int) -> List[str]:
        s = self.Stats()
        return narration_lines(self.Nodes(k), int(s["evaluated"][k]), int(s["levels"][k]))

    def DP(self, which: Optional[Sequence[bool]] = None) -> List[int]:
        """dp[capacity] of every instance (-1 where ``which`` is false)."""
        best = np.zeros(self.count, dtype=np.int64)
        w = None
        if which is not None:
            w = np.ascontiguousarray([1 if x else 0 for x in which], dtype=np.uint8)
            if len(w) != self.count:
                raise ValueError("which must have one entry per instance")
        N.check(N.lib.lpr_knap_batch_dp(self._h, _ptr(w, C.c_uint8), _ptr(best, C.c_int64)),
                "lpr_knap_batch_dp")
        return best.tolist()


class KnapsackOutcome(NamedTuple):
    """Option 5's report for one instance."""
    Z: float                # Branch & Bound Best Value Z*
    Chosen: List[int]       # original indices, ascending
    DP: float               # Dynamic Programming Result
    ResultsMatch: bool      # Program.cs:470: Math.Abs(dp - branchBoundResult) < 1e-6
    Status: int


def solve_knapsacks(instances: Sequence[Tuple[int, Sequence[float], Sequence[float]]],
                    node_cap=None, engine: Optional[Engine] = None) -> List[KnapsackOutcome]:
    """Option 5 for many (capacity, weights, values) instances: B&B and DP, one device call
    each."""
    b = KnapsackBatch([c for c, _, _ in instances], [w for _, w, _ in instances],
                      [v for _, _, v in instances], node_cap=node_cap, engine=engine)
    try:
        b.Solve()
        s = b.Stats()
        sel = b.SelectedIds()
        dp = b.DP()
        return [KnapsackOutcome(float(s["z"][k]), sel[k], float(dp[k]),
                                abs(float(dp[k]) - float(s["z"][k])) < 1e-6, int(s["status"][k]))
                for k in range(b.count)]
    finally:
        b.destroy()
