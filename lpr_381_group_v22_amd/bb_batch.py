"""Many independent Branch & Bound searches in one call (lpr_bb_batch_*).

Every IP of a batch runs the whole ``ExecuteBranchAndBound`` of
IntegerProgramming/BranchBoundSimplexSolver.cs on the MI355X, with no host step per node, and gives
the bits ``BranchBoundTree.run`` (lpr_bb_run) gives for that root alone.  The reference has no
batch mode: the per-IP accessors below are named after the single-tree surface
(branch_and_bound.py), and ``solve_integer_programs`` is menu option 3 (Program.cs:356-416) for
many models at once.

A batch made NARRATED (``narrate_reserve`` / ``Narrate``) also keeps what the
console text of ExecuteBranchAndBound is made of, written by the search kernel; ``NarrationText(k)``
formats it with branch_and_bound.format_branch_and_bound, the formatter of the single-tree path.
The record layout (csrc/bb_narr_layout.hpp), per IP:

* child tableaux: for record ``rid`` the list DoDualSimplex returns (:292, :341, :388) -- the
  tableau AddConstraint hands it, then one per pivot -- each (R0 + depth) x (C0 + depth) doubles,
  row-major, unrounded, back to back in the IP's slice of one slab; ``tab_off[rid]`` (doubles from
  the slice start) and ``ntab[rid]`` (tableaux made, after the drop of :392-400) go with the
  record; the root has ntab 0;
* per pop: objVal, nvars decision values, flags (1 scored, 2 all integer, 4 became the incumbent);
* the incumbent's tableau at its node's own shape.

A tableau that does not fit whole in the IP's reserved doubles is counted and not written, nor is
any later one: what is kept is a prefix and the totals are exact (csrc/kept_prefix.hpp).
"""
from __future__ import annotations

import ctypes as C
import io
import math
from contextlib import redirect_stdout
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from ._native import _ptr
from . import branch_and_bound as bnb
from .engine import Engine, default_engine
from .input_file_parser import Constraint
from .primal_batch import PrimalSimplexBatch

DEFAULT_NODE_CAP = 20   # :1038
MAX_NODE_CAP = 64       # kBBBatchMaxNodeCap
MAX_ROWS_H = 1024       # at full depth: rows + node_cap
MAX_COLS_H = 2048       # ... and cols + node_cap
DEFAULT_TRACE_CAP = 256
NARR_SCORED, NARR_INTEGER, NARR_INCUMBENT = 1, 2, 4  # pop flags (bb_narr_layout.hpp)


class NarrationInfo(NamedTuple):
    """lpr_bb_batch_narrate_info, one entry per IP."""
    tableaux: np.ndarray      # child tableaux made (exact)
    doubles_made: np.ndarray  # ... and their doubles
    doubles_kept: np.ndarray  # doubles kept: a prefix of those made
    offset: np.ndarray        # start of the IP's slice in the slab


class PackedRoots(NamedTuple):
    """The packed arrays of lpr_bb_batch_create."""
    rows: np.ndarray      # int32, per IP
    cols: np.ndarray      # int32, per IP
    tableaux: np.ndarray  # float64, rows x cols row-major blocks
    nvars: np.ndarray     # int32, per IP


def kept_tableaux(rows: int, cols: int, tab_off: int, ntab: int, doubles_kept: int) -> int:
    """How many whole tableaux of a record's list the IP's kept prefix holds: the rule of
    csrc/bb_narr_text_layout.hpp, min(ntab, (kept - tab_off) / (rows * cols)), never below 0."""
    return max(0, min(int(ntab), (int(doubles_kept) - int(tab_off)) // (rows * cols)))


def narration_block_index(root_shape, records, tab_off, ntab, doubles_kept: int) -> List[int]:
    """Where each record's tableaux are among the blocks of its IP in ``FormatNarration``'s text:
    entry rid is the block of the record's first kept tableau, counted from the IP's first block
    (tableau i of the record is block ``index[rid] + i``); the last entry is the number of child
    blocks, which is where the incumbent's block is when the IP has one.  ``records`` as
    ``Records(k)`` gives them, ``tab_off`` / ``ntab`` as ``Children(k)``, ``doubles_kept`` the
    IP's entry of ``narration_info()``."""
    index, at = [], 0
    for rid, rec in enumerate(records):
        index.append(at)
        at += kept_tableaux(root_shape[0] + rec["depth"], root_shape[1] + rec["depth"],
                            tab_off[rid], ntab[rid], doubles_kept)
    index.append(at)
    return index


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
        self.Narrated = False
        self._pruning = False      # of the last Run
        self._narr_info = None     # read once per run
        self._narr_text = None     # (DeviceText, first_block) of FormatNarration, per run

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
        self._drop_narration_text()
        if self._h:
            N.lib.lpr_bb_batch_destroy(self._h)
            self._h = None

    def _drop_narration_text(self) -> None:
        if getattr(self, "_narr_text", None) is not None:
            self._narr_text[0].destroy()
            self._narr_text = None

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
        self._pruning = bool(enable_pruning)
        self._narr_info = None
        self._drop_narration_text()
        return res

    # -- narration (section 23) ------------------------------------------------------------------
    def narrate_reserve(self, cap) -> None:
        """Make the batch narrated (lpr_bb_batch_narrate_reserve): ``cap`` doubles of child
        tableaux per IP (one int for all, or one per IP).  May be called again between runs."""
        caps = np.full(self.Count, int(cap), dtype=np.int64) if np.isscalar(cap) else \
            np.ascontiguousarray([int(c) for c in cap], dtype=np.int64)
        if caps.shape != (self.Count,):
            raise ValueError(f"{caps.size} caps for {self.Count} IPs")
        self.Narrated = False
        self._narr_info = None
        self._drop_narration_text()
        self._caps = caps
        N.check(N.lib.lpr_bb_batch_narrate_reserve(self._h, caps.ctypes.data_as(
            C.POINTER(C.c_int64))), "lpr_bb_batch_narrate_reserve")
        self.Narrated = True

    def narration_info(self) -> NarrationInfo:
        if self._narr_info is None:
            a = [np.zeros(self.Count, dtype=np.int64) for _ in range(4)]
            N.check(N.lib.lpr_bb_batch_narrate_info(self._h, *[_ptr(x, C.c_int64) for x in a]),
                    "lpr_bb_batch_narrate_info")
            self._narr_info = NarrationInfo(*a)
        return self._narr_info

    def Narrate(self, enable_pruning: bool = False, **run_opts) -> N.BBBatchResult:
        """The two-pass flow: reserve nothing, run, read the exact needs, reserve them, run
        again.  A run is deterministic and starts from the roots, so the second keeps all."""
        self.narrate_reserve(0)
        self.Run(enable_pruning=enable_pruning, **run_opts)
        self.narrate_reserve(self.narration_info().doubles_made)
        return self.Run(enable_pruning=enable_pruning, **run_opts)

    def narration_packed(self) -> np.ndarray:
        """The whole slab in one copy (lpr_bb_batch_narrate_read_all)."""
        total = int(self._caps.sum())
        out = np.zeros(max(total, 1), dtype=np.float64)
        N.check(N.lib.lpr_bb_batch_narrate_read_all(self._h, _ptr(out, C.c_double), out.size),
                "lpr_bb_batch_narrate_read_all")
        return out[:total]

    def PopInfo(self, k: int) -> List[dict]:
        """The pops of IP k in order: dict(id, z, vals (None for a pruned pop), flags)."""
        cap, nv = self.node_cap, self.nvars[k]
        fl, z = np.zeros(cap, dtype=np.int32), np.zeros(cap)
        vals = np.zeros(max(cap * nv, 1))
        n = C.c_int64()
        N.check(N.lib.lpr_bb_batch_narrate_pops_read(
            self._h, int(k), _ptr(fl, C.c_int32), _ptr(z, C.c_double), _ptr(vals, C.c_double), cap,
            C.byref(n)), "lpr_bb_batch_narrate_pops_read")
        ids = self.PopOrder(k)
        return [dict(id=ids[i], z=float(z[i]), flags=int(fl[i]),
                     vals=[float(v) for v in vals[i * nv:(i + 1) * nv]]
                     if fl[i] & NARR_SCORED else None) for i in range(n.value)]

    def Children(self, k: int):
        """(tab_off, ntab) per record of IP k (lpr_bb_batch_narrate_children_read)."""
        cap = 1 + 2 * self.node_cap
        off, nt = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int32)
        n = C.c_int64()
        N.check(N.lib.lpr_bb_batch_narrate_children_read(
            self._h, int(k), _ptr(off, C.c_int64), _ptr(nt, C.c_int32), cap, C.byref(n)),
            "lpr_bb_batch_narrate_children_read")
        return off[:n.value], nt[:n.value]

    def _child_tableaux(self, k: int, rid: int, depth: int, off, nt, kept: int):
        """The kept tableaux of record rid, and how many its list holds."""
        r, c = self._shapes[k][0] + depth, self._shapes[k][1] + depth
        have = kept_tableaux(r, c, off[rid], nt[rid], kept)
        out = np.zeros((max(have, 1), r, c))
        if have:
            N.check(N.lib.lpr_bb_batch_narrate_tableaux_read(
                self._h, int(k), int(off[rid]), have * r * c, _ptr(out, C.c_double)),
                "lpr_bb_batch_narrate_tableaux_read")
        return [out[i] for i in range(have)], int(nt[rid])

    def ChildTableaux(self, k: int, rid: int) -> List[np.ndarray]:
        """The kept tableaux of the child LP of record ``rid`` of IP k: DoDualSimplex's list
        (:292, :341, :388), unrounded.  Fewer than the record's ntab where the IP's cap cut it."""
        off, nt = self.Children(k)
        if not 0 <= rid < len(nt):
            raise IndexError(f"IP {k} has {len(nt)} records")
        depth = self.Records(k)[rid]["depth"]
        return self._child_tableaux(k, rid, depth, off, nt,
                                    int(self.narration_info().doubles_kept[k]))[0]

    def IncumbentTableau(self, k: int) -> Optional[np.ndarray]:
        """bestTableau of IP k (:935-983), or None where no integer solution was found."""
        if not self.Result(k)["found"]:
            return None
        r, c = C.c_int32(), C.c_int32()
        N.check(N.lib.lpr_bb_batch_narrate_best_read(self._h, int(k), None, C.byref(r),
                                                     C.byref(c)), "lpr_bb_batch_narrate_best_read")
        out = np.zeros((r.value, c.value))
        N.check(N.lib.lpr_bb_batch_narrate_best_read(self._h, int(k), _ptr(out, C.c_double),
                                                     C.byref(r), C.byref(c)),
                "lpr_bb_batch_narrate_best_read")
        return out

    def NarrationNumbers(self, k: int, device_text: bool = False):
        """(pops, incumbent tableau, capped) of IP k for format_branch_and_bound.  The text of a
        search has no gaps: raises ValueError where IP k kept fewer tableaux or trace quads than
        it made, or ended with LPR_PIVOT_LIMIT.  With ``device_text`` every tableau is its body
        from ``FormatNarration``'s text (a str) and no tableau is read back."""
        res = self.Result(k)
        if res["status"] == N.LPR_PIVOT_LIMIT:
            raise ValueError(f"IP {k} ended with LPR_PIVOT_LIMIT: its search is incomplete")
        info = self.narration_info()
        if info.doubles_kept[k] < info.doubles_made[k]:
            raise ValueError(f"IP {k} made {int(info.doubles_made[k])} doubles of child tableaux "
                             f"and keeps {int(info.doubles_kept[k])}: its text would miss tableaux")
        if res["pivots"] > self.trace_cap:
            raise ValueError(f"IP {k} made {res['pivots']} trace quads and trace_cap keeps "
                             f"{self.trace_cap}: its text would miss pivots")
        recs = self.Records(k)
        off, nt = self.Children(k)
        kept = int(info.doubles_kept[k])
        if device_text and (info.tableaux[k] > 0 or res["found"]):
            text, first = self.FormatNarration()
            index = narration_block_index(self._shapes[k], recs, off, nt, kept)

            def tableaux_of(rid):
                at = int(first[k]) + index[rid]
                return [text.block(at + i) for i in range(index[rid + 1] - index[rid])]

            incumbent = text.block(int(first[k + 1]) - 1) if res["found"] else None
        else:
            def tableaux_of(rid):
                return self._child_tableaux(k, rid, recs[rid]["depth"], off, nt, kept)[0]

            incumbent = None if device_text else self.IncumbentTableau(k)
        pivots = {}
        for rid, ph, r, c in self.Trace(k):
            pivots.setdefault(rid, []).append((ph, r, c))
        kids = {}
        for rid, rec in enumerate(recs):
            if rec["parent"] >= 0:
                kids.setdefault(rec["parent"], []).append(rid)
        status = {0: bnb.BB_SOLVED, 1: bnb.BB_INFEASIBLE, 2: bnb.BB_FAILED}
        pops = []
        for pop in self.PopInfo(k):
            children = None
            if pop["id"] in kids:
                children = [bnb.ChildNumbers(status[recs[rid]["status"]], pivots.get(rid, []),
                                             tableaux_of(rid)) for rid in kids[pop["id"]]]
            pops.append(bnb.PopNumbers(pop["z"], pop["vals"], children))
        return pops, incumbent, res["status"] == N.LPR_BB_NODE_CAP

    def NarrationText(self, k: int, newline: str = "\n") -> str:
        """What ExecuteBranchAndBound of IP k alone writes to the console (:1006-1233), with
        "Potential infinite loop detected" (:1040) for LPR_BB_NODE_CAP.  ``newline`` ends every
        Console.WriteLine (format_branch_and_bound)."""
        pops, tab, capped = self.NarrationNumbers(k)
        return bnb.format_branch_and_bound(self.nvars[k], pops, tab, capped, self._pruning,
                                           newline)[0]

    # -- device text (section 26) ---------------------------------------------------------------
    def FormatNarration(self):
        """(DeviceText, first_block) of lpr_bb_batch_narrate_text: DisplayTableau's body (:623-640)
        of every kept child tableau of every IP, in record-id order, then the incumbent's where
        the IP has one; IP k's blocks are first_block[k] .. first_block[k + 1] - 1
        (``narration_block_index`` places a record's).  One call per run: kept until the next
        ``Run`` / ``narrate_reserve``."""
        if self._narr_text is None:
            first = np.zeros(self.Count + 1, dtype=np.int64)
            h = C.c_void_p()
            N.check(N.lib.lpr_bb_batch_narrate_text(self._h, _ptr(first, C.c_int64), C.byref(h)),
                    "lpr_bb_batch_narrate_text")
            from .table_iteration_formater import DeviceText
            self._narr_text = (DeviceText(h), first)
        return self._narr_text

    def NarrationTextDevice(self, k: int, newline: str = "\n") -> str:
        """``NarrationText(k)`` with every tableau rounded and formatted on the device
        (``FormatNarration``): the same text, the same ValueErrors."""
        pops, body, capped = self.NarrationNumbers(k, device_text=True)
        return bnb.format_branch_and_bound(self.nvars[k], pops, body, capped, self._pruning,
                                           newline)[0]

    def all_narration_texts(self, newline: str = "\n") -> List[str]:
        """``NarrationTextDevice(k)`` for every IP, from one ``FormatNarration``."""
        return [self.NarrationTextDevice(k, newline) for k in range(self.Count)]

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


def option3_texts(parsers, node_cap: int = 0, enable_pruning: bool = False,
                  engine: Optional[Engine] = None, primal_trace_cap: int = 256,
                  trace_cap: int = 1 << 14,
                  device_text: bool = False) -> List[Tuple[str, List[float], float]]:
    """Menu option 3 (Program.cs:356-415) for many models at once, with its text: one traced
    PrimalSimplexBatch and one narrated BranchAndBoundBatch.  Per model ``(text, x, z)``: the
    console text Program.cs captures into the result file -- the banner (:358), the canonical
    form (:360-361), the primal solve's tables (``ConsoleText(k)``), everything
    ExecuteBranchAndBound writes (``NarrationText(k)``) and the result block (:401-407) -- and
    SolveFromPrimal's ``(x, z)``.  The caller's parsers are left as they are.  With
    ``device_text`` the tables of both halves are formatted on the device (``ConsoleTextDevice``,
    ``NarrationTextDevice``): the same text."""
    from . import program as prog
    from . import table_iteration_formater as fmt
    nl = fmt.NEWLINE
    primal = PrimalSimplexBatch(option3_models(parsers), engine=engine,
                                trace_cap=primal_trace_cap)
    try:
        primal.Solve()
        console = primal.ConsoleTextDevice if device_text else primal.ConsoleText
        consoles = [console(k) for k in range(primal.Count)]
        bb = BranchAndBoundBatch.from_primal_batch(primal, node_cap=node_cap, trace_cap=trace_cap)
    finally:
        primal.destroy()
    try:
        bb.Narrate(enable_pruning=enable_pruning)
        res = bb.result_arrays()
        xs = bb.solution_packed()
        out, at = [], 0
        for k, p in enumerate(parsers):
            n = bb.nvars[k]
            found = bool(res["found"][k])
            x = [float(v) for v in xs[at:at + n]] if found else []
            z = float(res["z"][k]) if found else -math.inf
            at += n
            buf = io.StringIO()

            class _Console(io.TextIOBase):  # print()'s own terminator is Console.WriteLine's
                def write(self, t):
                    buf.write(nl if t == "\n" else t)
                    return len(t)

            with redirect_stdout(_Console()):
                print("Solving with Branch and Bound Simplex Algorithm...")
                prog.display_canonical_form(p.ProblemType, p.ObjectiveCoefficients, p.Constraints,
                                            p.SignRestrictions)
            tail = ["\n=== Branch & Bound Result ===" + nl,
                    f"Z* = {fmt._custom_0_hashes(z) if math.isfinite(z) else z}" + nl]
            tail += [f"x{i + 1} = {fmt._custom_0_hashes(v)}" + nl for i, v in enumerate(x)]
            narration = bb.NarrationTextDevice if device_text else bb.NarrationText
            out.append((buf.getvalue() + consoles[k] + narration(k, newline=nl) +
                        "".join(tail), x, z))
    finally:
        bb.destroy()
    return out


def write_option3_files(parsers, paths: Sequence[str], **kw) -> List[Tuple[List[float], float]]:
    """option3_texts, each text written as Program.cs:409-410 writes it (WriteSnapshotsOnly,
    OutputFileWrite.cs:83-119) to its own path.  Returns ``(x, z)`` per model."""
    from . import program as prog
    if len(paths) != len(parsers):
        raise ValueError(f"{len(paths)} paths for {len(parsers)} models")
    out = []
    for path, (text, x, z) in zip(paths, option3_texts(parsers, **kw)):
        prog.write_snapshots_only(path, "Branch and Bound Simplex Algorithm", [text], z, x,
                                  append=False)
        out.append((x, z))
    return out
