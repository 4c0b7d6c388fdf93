"""Host mirror of menu option 5 (``Program.cs:430-470``): ``KnapsackBranchBoundSimplex`` (the
level-synchronous branch-and-bound) and ``KnapsackBranchBoundSolver.Solve`` (the 0/1 DP cross-check).
The reference calls both classes without defining them; the rules are DESIGN.md section 11.  All
numbers come from the device (``lpr_knap_*``); this file is plumbing and text.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _native as N
from .engine import Engine, default_engine
from .table_iteration_formater import dotnet_double_to_string

FRACTIONAL, PRUNED, INTEGRAL, INFEASIBLE = 0, 1, 2, 3
STATUS_TEXT = {FRACTIONAL: "fractional", PRUNED: "fractional, pruned", INTEGRAL: "integral",
               INFEASIBLE: "infeasible"}


class KnapsackItem(NamedTuple):
    """An item of GetSelectedItemsOriginal(): original 0-based index, value, weight."""
    Id: int
    Value: float
    Weight: float


class KnapsackNode(NamedTuple):
    """One node record of the device log, in evaluation order."""
    parent: int   # record index of the parent, -1 for the root
    branch: int   # 0: child ".1" (x_k = 0), 1: child ".2" (x_k = 1)
    status: int   # FRACTIONAL / PRUNED / INTEGRAL / INFEASIBLE
    bound: float
    k: int        # original index of the critical item, -1 when there is none to report
    V: int


def node_labels(nodes: Sequence[KnapsackNode]) -> List[str]:
    """"0" for the root, "1" / "2" for its children, "1.1" / "1.2" for the children of "1"."""
    out: List[str] = []
    for nd in nodes:
        if nd.parent < 0:
            out.append("0")
        else:
            out.append(("" if nd.parent == 0 else out[nd.parent] + ".") + str(nd.branch + 1))
    return out


def narration_lines(nodes: Sequence[KnapsackNode], evaluated: int, levels: int) -> List[str]:
    """PrintIterations(): one line per node (the same text as GpuSolvers.cs), then a count of the
    nodes the log did not keep."""
    labels = node_labels(nodes)
    fixed: List[str] = []
    lines: List[str] = []
    for r, nd in enumerate(nodes):
        if nd.parent < 0:
            fixed.append("")
        else:
            p = nodes[nd.parent]
            f = f"x{p.k + 1}={nd.branch}"
            fixed.append((fixed[nd.parent] + " " + f) if fixed[nd.parent] else f)
        if nd.status == INFEASIBLE:
            tail = "bound = -; k = -; V = -"
        else:
            k = f"x{nd.k + 1}" if nd.k >= 0 else "-"
            tail = f"bound = {dotnet_double_to_string(nd.bound)}; k = {k}; V = {nd.V}"
        lines.append(f"Node {labels[r]}: fixed {fixed[r] or 'none'}; {STATUS_TEXT[nd.status]}; "
                     f"{tail}")
    if evaluated > len(nodes):
        lines.append(f"({evaluated - len(nodes)} of {evaluated} nodes in {levels} levels not "
                     f"recorded)")
    return lines


class KnapsackBranchBoundSimplex:
    """``new KnapsackBranchBoundSimplex(capacity, weights, values)`` (Program.cs:443-447).

    node_cap: evaluated nodes (0: 2^22).  narrate: node records kept for PrintIterations (-1: auto,
    4096 when n <= 64; 0: none; > 0: that many)."""

    def __init__(self, capacity: int, weights: Sequence[float], values: Sequence[float],
                 engine: Optional[Engine] = None, node_cap: int = 0, narrate: int = -1):
        self.engine = engine or default_engine()
        self.capacity = capacity
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.n = len(self.weights)
        self.node_cap = node_cap
        self.narrate = narrate
        self.Status: Optional[int] = None
        self.Found = False
        self.Z: Optional[float] = None
        self.Evaluated = self.Levels = self.Widest = 0
        if len(self.values) != self.n:
            raise ValueError("weights and values differ in length")
        h = C.c_void_p()
        N.check(N.lib.lpr_knap_bb_create(
            self.engine._h, int(capacity),
            self.weights.ctypes.data_as(C.POINTER(C.c_double)),
            self.values.ctypes.data_as(C.POINTER(C.c_double)), self.n, C.byref(h)),
            "lpr_knap_bb_create")
        self._h = h

    def Solve(self) -> float:
        """Z* of the level-synchronous search (LPR_BB_NODE_CAP keeps the incumbent so far)."""
        opts = N.KnapBBOpts(node_cap=int(self.node_cap), narrate=int(self.narrate))
        res = N.KnapBBResult()
        self.Status = N.check(N.lib.lpr_knap_bb_solve(self._h, C.byref(opts), C.byref(res)),
                              "lpr_knap_bb_solve")
        self.Found = bool(res.found)
        self.Z = res.z
        self.Evaluated, self.Levels, self.Widest = res.evaluated, res.levels, res.widest
        return res.z

    def Rank(self) -> List[int]:
        r = np.zeros(self.n, dtype=np.int32)
        N.check(N.lib.lpr_knap_bb_rank_read(self._h, r.ctypes.data_as(C.POINTER(C.c_int32))),
                "lpr_knap_bb_rank_read")
        return r.tolist()

    def SelectedIds(self) -> List[int]:
        ids = np.zeros(self.n, dtype=np.int32)
        cnt = C.c_int32()
        N.check(N.lib.lpr_knap_bb_selected_read(self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 C.byref(cnt)), "lpr_knap_bb_selected_read")
        return ids[:cnt.value].tolist()

    def GetSelectedItemsOriginal(self) -> List[KnapsackItem]:
        """The incumbent's items in ascending original index (Program.cs:455-461)."""
        return [KnapsackItem(i, float(self.values[i]), float(self.weights[i]))
                for i in self.SelectedIds()]

    def Nodes(self) -> List[KnapsackNode]:
        cnt = C.c_int64()
        N.check(N.lib.lpr_knap_bb_nodes_read(self._h, None, None, None, None, None, None, 0,
                                              C.byref(cnt)), "lpr_knap_bb_nodes_read")
        m = cnt.value
        par, br, st, kk = (np.zeros(max(m, 1), dtype=np.int32) for _ in range(4))
        bd = np.zeros(max(m, 1), dtype=np.float64)
        V = np.zeros(max(m, 1), dtype=np.int64)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        N.check(N.lib.lpr_knap_bb_nodes_read(
            self._h, i32(par), i32(br), i32(st), bd.ctypes.data_as(C.POINTER(C.c_double)),
            i32(kk), V.ctypes.data_as(C.POINTER(C.c_int64)), m, C.byref(cnt)),
            "lpr_knap_bb_nodes_read")
        return [KnapsackNode(int(par[r]), int(br[r]), int(st[r]), float(bd[r]), int(kk[r]),
                             int(V[r])) for r in range(m)]

    def IterationLines(self) -> List[str]:
        return narration_lines(self.Nodes(), self.Evaluated, self.Levels)

    def PrintIterations(self) -> None:
        for line in self.IterationLines():
            print(line)

    def destroy(self) -> None:
        if getattr(self, "_h", None):
            N.lib.lpr_knap_bb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def knapsack_dp(capacity: int, weights: Sequence[int], values: Sequence[int],
                engine: Optional[Engine] = None, variant: int = 0) -> int:
    """The 0/1 DP on the device, as the exact int64 dp[capacity].  variant 1 forces one
    streaming pass per item (same result)."""
    eng = engine or default_engine()
    w = np.ascontiguousarray(weights, dtype=np.int32)
    v = np.ascontiguousarray(values, dtype=np.int32)
    if len(w) != len(v):
        raise ValueError("weights and values differ in length")
    best = C.c_int64()
    opts = N.KnapDpOpts(variant=variant)
    N.check(N.lib.lpr_knap_dp(eng._h, int(capacity), w.ctypes.data_as(C.POINTER(C.c_int32)),
                              v.ctypes.data_as(C.POINTER(C.c_int32)), len(w), C.byref(opts),
                              C.byref(best)), "lpr_knap_dp")
    return best.value


class KnapsackBranchBoundSolver:
    """``KnapsackBranchBoundSolver.Solve(capacity, int[] weights, int[] values)`` (Program.cs:465)."""

    @staticmethod
    def Solve(capacity: int, weights: Sequence[int], values: Sequence[int],
              engine: Optional[Engine] = None) -> float:
        return float(knapsack_dp(capacity, weights, values, engine))
