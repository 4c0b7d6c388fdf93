"""Many independent Branch & Bound searches in one call (lpr_bb_batch_*).

Every IP of a batch runs the whole ``ExecuteBranchAndBound`` of
IntegerProgramming/BranchBoundSimplexSolver.cs on the MI355X, with no host step per node, and gives
the bits ``BranchBoundTree.run`` (lpr_bb_run) gives for that root alone.  The reference has no
batch mode: the per-IP accessors below are named after the single-tree surface
(branch_and_bound.py), and ``solve_integer_programs`` is menu option 3 (Program.cs:356-416) for
many models at once.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .engine import Engine, default_engine
from .input_file_parser import Constraint
from .primal_batch import PrimalSimplexBatch

DEFAULT_NODE_CAP = 20   # :1038
MAX_NODE_CAP = 64       # kBBBatchMaxNodeCap
MAX_ROWS_H = 1024       # at full depth: rows + node_cap
MAX_COLS_H = 2048       # ... and cols + node_cap
DEFAULT_TRACE_CAP = 256


class PackedRoots(NamedTuple):
    """The packed arrays of lpr_bb_batch_create."""
    rows: np.ndarray      # int32, per IP
    cols: np.ndarray      # int32, per IP
    tableaux: np.ndarray  # float64, rows x cols row-major blocks
    nvars: np.ndarray     # int32, per IP


def node_cap_of(node_cap: int) -> int:
    """The node cap a batch runs with: <= 0 is the reference's 20; above 64 is refused."""
    cap = int(node_cap) if int(node_cap) > 0 else DEFAULT_NODE_CAP
    if cap > MAX_NODE_CAP:
        raise ValueError(f"node_cap {node_cap} is above the batch maximum of {MAX_NODE_CAP}")
    return cap


def pack_roots(tableaux: Sequence[np.ndarray], nvars: Sequence[int],
               node_cap: int = 0) -> PackedRoots:
    """Root tableaux and SetNumVars per IP -> the packed ABI arrays, with the checks of
    lpr_bb_batch_create (raises ValueError where the call would refuse the batch)."""
    cap = node_cap_of(node_cap)
    try:
        T = [np.ascontiguousarray(t, dtype=np.float64) for t in tableaux]
        nv = [int(v) for v in nvars]
    except (TypeError, ValueError):
        raise ValueError("tableaux must be 2-D numeric arrays and nvars integers")
    if not T:
        raise ValueError("no tableaux")
    if len(nv) != len(T):
        raise ValueError(f"{len(T)} tableaux but {len(nv)} nvars")
    for k, (t, n) in enumerate(zip(T, nv)):
        if t.ndim != 2:
            raise ValueError(f"IP {k}: the root is not a 2-D array")
        r, c = t.shape
        if r < 1 or c < 2 or not 0 <= n <= c - 1:
            raise ValueError(f"IP {k}: a {r} x {c} root with nvars={n}; it needs rows >= 1, "
                             f"cols >= 2 and 0 <= nvars <= cols - 1")
        if r + cap > MAX_ROWS_H or c + cap > MAX_COLS_H:
            raise ValueError(f"IP {k}: a {r} x {c} root is {r + cap} x {c + cap} at full depth, "
                             f"beyond {MAX_ROWS_H} x {MAX_COLS_H}; run it with BranchBoundTree")
    return PackedRoots(np.asarray([t.shape[0] for t in T], dtype=np.int32),
                       np.asarray([t.shape[1] for t in T], dtype=np.int32),
                       np.concatenate([t.reshape(-1) for t in T]),
                       np.asarray(nv, dtype=np.int32))


def option3_models(parsers) -> List[tuple]:
    """Option 3's models, one per InputFileParser: the objective, the constraints and the n rows
    "x_i <= 1" that program._append_unit_bound_rows appends (Program.cs:372-382), on copies --
    the caller's parsers are left as they are -- and isMaximization = true, as Program.cs:384
    constructs its PrimalSimplexSolver."""
    models = []
    for p in parsers:
        obj = list(p.ObjectiveCoefficients)
        cons = [Constraint(list(c.Coefficients), c.Relation, c.RHS) for c in p.Constraints]
        n = len(obj)
        for i in range(n):
            co = [0.0] * (n + 3)
            co[i] = 1.0
            co[n + 1] = 1.0
            cons.append(Constraint(co, "<=", 1.0))
        models.append((obj, cons, True))
    return models


def _ptr(a: Optional[np.ndarray], ctype):
    return None if a is None or not a.size else a.ctypes.data_as(C.POINTER(ctype))


class BranchAndBoundBatch:
    """``count`` BranchAndBound searches in one device handle (lpr_bb_batch_*)."""

    def __init__(self, handle: C.c_void_p, engine: Engine, shapes, nvars, node_cap: int,
                 trace_cap: int):
        self._h = handle
        self._engine = engine
        self._shapes = list(shapes)
        self.nvars = [int(v) for v in nvars]
        self.node_cap = node_cap
        self.trace_cap = trace_cap
        self.Count = len(self._shapes)
        self.LastResult: Optional[N.BBBatchResult] = None

    @classmethod
    def from_tableaux(cls, tableaux: Sequence[np.ndarray], nvars: Sequence[int], node_cap: int = 0,
                      trace_cap: int = 0, engine: Optional[Engine] = None) -> "BranchAndBoundBatch":
        """Roots (each a primal FinalTableau) and SetNumVars per IP (BranchAndBoundAdapter.cs:
        9-24)."""
        p = pack_roots(tableaux, nvars, node_cap)
        eng = engine or default_engine()
        h = C.c_void_p()
        N.check(N.lib.lpr_bb_batch_create(eng._h, len(p.rows), _ptr(p.rows, C.c_int32),
                                          _ptr(p.cols, C.c_int32), _ptr(p.tableaux, C.c_double),
                                          _ptr(p.nvars, C.c_int32), int(node_cap), int(trace_cap),
                                          C.byref(h)), "lpr_bb_batch_create")
        return cls(h, eng, zip(p.rows.tolist(), p.cols.tolist()), p.nvars, node_cap_of(node_cap),
                   int(trace_cap) if trace_cap > 0 else DEFAULT_TRACE_CAP)

    @classmethod
    def from_primal_batch(cls, primal: PrimalSimplexBatch, node_cap: int = 0,
                          trace_cap: int = 0) -> "BranchAndBoundBatch":
        """SolveFromPrimal (:9-24) for every LP of a solved PrimalSimplexBatch, device to device:
        nvars = SolutionVector.Count, or InferNumVariables (cols - 1, at least 1) for an
        unbounded LP.  The new handle does not depend on ``primal`` staying alive."""
        h = C.c_void_p()
        N.check(N.lib.lpr_bb_batch_from_batch(primal._h, int(node_cap), int(trace_cap),
                                              C.byref(h)), "lpr_bb_batch_from_batch")
        shapes, nv = [], []
        for k in range(primal.Count):
            r, c, n = primal.Shape(k)
            shapes.append((r, c))
            nv.append(n if primal.Status[k] == N.LPR_OK_OPTIMAL else max(1, c - 1))
        return cls(h, primal._engine, shapes, nv, node_cap_of(node_cap),
                   int(trace_cap) if trace_cap > 0 else DEFAULT_TRACE_CAP)

    def destroy(self) -> None:
        if self._h:
            N.lib.lpr_bb_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- ExecuteBranchAndBound :1006-1233, per IP ----------------------------------------------
    def Run(self, enable_pruning: bool = False, chunk: int = 0, variant: int = 0,
            max_child_pivots: int = 0) -> N.BBBatchResult:
        opts = N.BBBatchOpts(enable_pruning=1 if enable_pruning else 0, chunk=int(chunk),
                             variant=int(variant), max_child_pivots=int(max_child_pivots))
        res = N.BBBatchResult()
        N.check(N.lib.lpr_bb_batch_run(self._h, C.byref(opts), C.byref(res)), "lpr_bb_batch_run")
        self.LastResult = res
        return res

    # -- bulk reads -----------------------------------------------------------------------------
    def result_arrays(self) -> dict:
        """lpr_bb_result's fields per IP, as arrays."""
        n = self.Count
        out = dict(status=np.zeros(n, dtype=np.int32), found=np.zeros(n, dtype=np.int32),
                   processed=np.zeros(n, dtype=np.int64), best_node=np.zeros(n, dtype=np.int32),
                   z=np.zeros(n, dtype=np.float64), pivots=np.zeros(n, dtype=np.int64),
                   nodes_created=np.zeros(n, dtype=np.int64))
        N.check(N.lib.lpr_bb_batch_result_read(
            self._h, _ptr(out["status"], C.c_int32), _ptr(out["found"], C.c_int32),
            _ptr(out["processed"], C.c_int64), _ptr(out["best_node"], C.c_int32),
            _ptr(out["z"], C.c_double), _ptr(out["pivots"], C.c_int64),
            _ptr(out["nodes_created"], C.c_int64)), "lpr_bb_batch_result_read")
        return out

    def solution_packed(self) -> np.ndarray:
        total = sum(self.nvars)
        x = np.zeros(max(total, 1), dtype=np.float64)
        N.check(N.lib.lpr_bb_batch_solution_read(self._h, _ptr(x, C.c_double)),
                "lpr_bb_batch_solution_read")
        return x[:total]

    # -- per-IP reads ---------------------------------------------------------------------------
    def Result(self, k: int) -> dict:
        a = self.result_arrays()
        return {key: (float(v[k]) if key == "z" else int(v[k])) for key, v in a.items()}

    def Solution(self, k: int) -> Optional[np.ndarray]:
        """The incumbent x of IP k, or None where no integer solution was found."""
        if not self.Result(k)["found"]:
            return None
        at = sum(self.nvars[:k])
        return self.solution_packed()[at:at + self.nvars[k]]

    def Records(self, k: int) -> List[dict]:
        cap = 1 + 2 * self.node_cap
        p, kd, d, v, s = (np.zeros(cap, dtype=np.int32) for _ in range(5))
        b, z = np.zeros(cap), np.zeros(cap)
        n = C.c_int64()
        N.check(N.lib.lpr_bb_batch_records_read(
            self._h, int(k), _ptr(p, C.c_int32), _ptr(kd, C.c_int32), _ptr(d, C.c_int32),
            _ptr(v, C.c_int32), _ptr(b, C.c_double), _ptr(s, C.c_int32), _ptr(z, C.c_double),
            cap, C.byref(n)), "lpr_bb_batch_records_read")
        return [dict(parent=int(p[i]), kind=int(kd[i]), depth=int(d[i]), var=int(v[i]),
                     bound=float(b[i]), status=int(s[i]), z=float(z[i])) for i in range(n.value)]

    def PopOrder(self, k: int) -> List[int]:
        ids = np.zeros(max(self.node_cap, 1), dtype=np.int32)
        n = C.c_int64()
        N.check(N.lib.lpr_bb_batch_pop_order_read(self._h, int(k), _ptr(ids, C.c_int32),
                                                  self.node_cap, C.byref(n)),
                "lpr_bb_batch_pop_order_read")
        return ids[:n.value].tolist()

    def Trace(self, k: int) -> List[Tuple[int, int, int, int]]:
        q = np.zeros(4 * max(self.trace_cap, 1), dtype=np.int32)
        n = C.c_int64()
        N.check(N.lib.lpr_bb_batch_trace_read(self._h, int(k), _ptr(q, C.c_int32),
                                              self.trace_cap, C.byref(n)),
                "lpr_bb_batch_trace_read")
        return [tuple(t) for t in q[:4 * n.value].reshape(-1, 4).tolist()]


def solve_integer_programs(parsers, node_cap: int = 0, enable_pruning: bool = False,
                           engine: Optional[Engine] = None) -> List[Tuple[List[float], float]]:
    """Menu option 3 (Program.cs:356-416) for many models at once: the unit bound rows on copies,
    PrimalSimplexSolver.Solve per model (one PrimalSimplexBatch), then SolveFromPrimal per model
    (one BranchAndBoundBatch).  Returns ``(x, z)`` per model as
    ``BranchAndBoundAdapter.SolveFromPrimal`` does: ``([], -inf)`` where no integer solution was
    found (BranchAndBoundAdapter.cs:23)."""
    primal = PrimalSimplexBatch(option3_models(parsers), engine=engine)
    try:
        primal.Solve()
        bb = BranchAndBoundBatch.from_primal_batch(primal, node_cap=node_cap)
    finally:
        primal.destroy()
    try:
        bb.Run(enable_pruning=enable_pruning)
        res = bb.result_arrays()
        x = bb.solution_packed()
    finally:
        bb.destroy()
    out, at = [], 0
    for k, n in enumerate(bb.nvars):
        if res["found"][k]:
            out.append(([float(v) for v in x[at:at + n]], float(res["z"][k])))
        else:
            out.append(([], -math.inf))
        at += n
    return out
