"""Many independent ``PrimalSimplexSolver`` runs in one call (lpr_batch_*).

Every LP of a batch is built and solved on the MI355X with the rules of
Simplex/PrimalSimplexSolver.cs, the same bits ``PrimalSimplexSolver`` gives for that LP alone.
The reference has no batch mode: the members below are per-LP lists / accessors named after the
single-model mirror (primal_simplex_solver.py).  A batch made with ``trace_cap > 0`` is traced
(DESIGN.md section 22): its solve also stores the tableau after every pivot of every LP on the
device, and ``IterationSnapshots(k)`` / ``ConsoleText(k)`` format them with the single mirror's
formatter; an untraced batch keeps none.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _native as N
from ._native import _ptr
from .engine import Engine, default_engine
from . import table_iteration_formater as fmt
from .primal_simplex_solver import (col_label, format_console, format_snapshots,
                                    solution_summary)


class PackedModels(NamedTuple):
    """The packed arrays of lpr_batch_from_lps."""
    n: np.ndarray          # int32, per LP
    m: np.ndarray          # int32, per LP
    objective: np.ndarray  # float64, packed by n
    A: np.ndarray          # float64, m x n row-major blocks
    ncoef: np.ndarray      # int32, packed by m
    relation: np.ndarray   # int8, packed by m
    rhs: np.ndarray        # float64, packed by m
    is_max: np.ndarray     # int8, per LP


def _number(v, what: str) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.floating,
                                                                np.integer)):
        raise ValueError(f"{what} is not a number: {v!r}")
    return float(v)


def _numbers(vals, what: str) -> np.ndarray:
    a = np.asarray(list(vals))
    if a.size and a.dtype.kind not in "fiu":  # bools, strings and objects are refused
        raise ValueError(f"{what} holds entries that are not numbers")
    return a.astype(np.float64).reshape(-1)


def pack_models(models) -> PackedModels:
    """``(objective, constraints, isMaximization)`` triples -> the packed ABI arrays.

    The same flattening ``PrimalSimplexSolver`` does per model: a row keeps its first
    ``min(n, len(Coefficients))`` coefficients (PrimalSimplexSolver.cs:68-72); ">=" and "=" map to
    their relation codes, anything else is "<=" (:36-50).  Raises ValueError on malformed input."""
    try:
        models = list(models)
    except TypeError:
        raise ValueError("models must be a sequence of (objective, constraints, isMaximization)")
    if not models:
        raise ValueError("no models")
    ns, ms, obj, A, nc, rel, rhs, mx = [], [], [], [], [], [], [], []
    for k, model in enumerate(models):
        try:
            objective, constraints, is_max = model
        except (TypeError, ValueError):
            raise ValueError(f"model {k} is not an (objective, constraints, isMaximization) triple")
        if isinstance(objective, (str, bytes)) or isinstance(constraints, (str, bytes)):
            raise ValueError(f"model {k}: objective and constraints must be sequences")
        try:
            c = _numbers(objective, f"model {k} objective")
            cons = list(constraints)
        except TypeError:
            raise ValueError(f"model {k}: objective and constraints must be sequences")
        if not isinstance(is_max, (bool, np.bool_, numbers.Integral)):
            raise ValueError(f"model {k}: isMaximization must be a bool")
        n, m = len(c), len(cons)
        if n + m == 0:
            raise ValueError(f"model {k} has neither variables nor constraints")
        block = np.zeros((m, n))
        for i, con in enumerate(cons):
            try:
                coeffs, relation, b = con.Coefficients, con.Relation, con.RHS
            except AttributeError:
                raise ValueError(f"model {k} constraint {i} has no Coefficients / Relation / RHS")
            if not isinstance(relation, str):
                raise ValueError(f"model {k} constraint {i}: Relation must be a string")
            try:
                coeffs = list(coeffs)
            except TypeError:
                raise ValueError(f"model {k} constraint {i}: Coefficients must be a sequence")
            cnt = min(n, len(coeffs))
            block[i, :cnt] = _numbers(coeffs[:cnt], f"model {k} constraint {i} coefficients")
            nc.append(cnt)
            rel.append(N.LPR_REL_GE if relation == ">=" else
                       (N.LPR_REL_EQ if relation == "=" else N.LPR_REL_LE))
            rhs.append(_number(b, f"model {k} constraint {i} RHS"))
        ns.append(n)
        ms.append(m)
        obj.append(c)
        A.append(block.reshape(-1))
        mx.append(1 if is_max else 0)
    return PackedModels(
        np.asarray(ns, dtype=np.int32), np.asarray(ms, dtype=np.int32),
        np.concatenate(obj).astype(np.float64),
        np.concatenate(A).astype(np.float64) if A else np.zeros(0),
        np.asarray(nc, dtype=np.int32), np.asarray(rel, dtype=np.int8),
        np.asarray(rhs, dtype=np.float64), np.asarray(mx, dtype=np.int8))


# One record of a traced batch (batch_trace_* of batch_common.hpp), in doubles: the header
# [0] leavingRow (1-based) [1] enteringCol of the pivot that made it (-1, -1 for record 0), then
# the tableau after that pivot, rows x cols row-major.
TRACE_ROW, TRACE_COL, TRACE_TAB = 0, 1, 2


def trace_stride(rows: int, cols: int) -> int:
    """batch_trace_stride: doubles of one record."""
    return TRACE_TAB + rows * cols


def trace_record(r: np.ndarray, rows: int, cols: int):
    """One record as (leaving_row, entering_col, tableau)."""
    return (int(r[TRACE_ROW]), int(r[TRACE_COL]),
            r[TRACE_TAB:TRACE_TAB + rows * cols].reshape(rows, cols).copy())


class PrimalSimplexBatch:
    """``count`` PrimalSimplexSolver models in one device handle.

    ``Status[k]``, ``FinalZ[k]`` (0.0 unless optimal, as the C# leaves it on the unbounded exit),
    ``SolutionVector[k]`` (None unless optimal) and ``Iterations[k]`` are set by ``Solve``;
    ``BasicVariables(k)``, ``PivotLog(k)`` and ``GetFinalTableau(k)`` read LP k."""

    def __init__(self, models, engine: Optional[Engine] = None, log_cap: int = 0,
                 trace_cap: int = 0):
        p = pack_models(models)
        self._init(engine)
        h = C.c_void_p()
        N.check(N.lib.lpr_batch_from_lps(
            self._engine._h, len(p.n), _ptr(p.n, C.c_int32), _ptr(p.m, C.c_int32),
            _ptr(p.objective, C.c_double), _ptr(p.A, C.c_double), _ptr(p.ncoef, C.c_int32),
            _ptr(p.relation, C.c_int8), _ptr(p.rhs, C.c_double), _ptr(p.is_max, C.c_int8),
            int(log_cap), C.byref(h)), "lpr_batch_from_lps")
        self._attach(h, [(int(m) + 1, int(n) + int(m) + 1, int(n)) for n, m in zip(p.n, p.m)],
                     log_cap)
        if trace_cap:
            self.trace_reserve(trace_cap)

    @classmethod
    def from_parsers(cls, parsers, engine: Optional[Engine] = None, log_cap: int = 0,
                     trace_cap: int = 0) -> "PrimalSimplexBatch":
        """One LP per InputFileParser, maximising unless ProblemType is "min" (program.py)."""
        models = [(p.ObjectiveCoefficients, p.Constraints,
                   (p.ProblemType or "").lower() != "min") for p in parsers]
        return cls(models, engine=engine, log_cap=log_cap, trace_cap=trace_cap)

    @classmethod
    def from_tableaux(cls, tableaux: Sequence[np.ndarray], bases=None,
                      engine: Optional[Engine] = None, log_cap: int = 0,
                      trace_cap: int = 0) -> "PrimalSimplexBatch":
        """Ready (rows x cols) tableaux, with their bases (rows - 1 entries each) or None."""
        self = cls.__new__(cls)
        self._init(engine)
        T = [np.ascontiguousarray(t, dtype=np.float64) for t in tableaux]
        if not T or any(t.ndim != 2 for t in T):
            raise ValueError("tableaux must be a non-empty list of 2-D arrays")
        rows = np.asarray([t.shape[0] for t in T], dtype=np.int32)
        cols = np.asarray([t.shape[1] for t in T], dtype=np.int32)
        flat = np.concatenate([t.reshape(-1) for t in T])
        b = None
        if bases is not None:
            b = np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1) for x in bases] +
                               [np.zeros(0, dtype=np.int32)])
            if b.size != int(np.sum(rows - 1)):
                raise ValueError("bases must hold rows - 1 entries per tableau")
        h = C.c_void_p()
        N.check(N.lib.lpr_batch_create(self._engine._h, len(T), _ptr(rows, C.c_int32),
                                       _ptr(cols, C.c_int32), _ptr(flat, C.c_double),
                                       None if b is None else _ptr(b, C.c_int32), int(log_cap),
                                       C.byref(h)), "lpr_batch_create")
        self._attach(h, [(int(r), int(c), max(0, int(c) - int(r))) for r, c in zip(rows, cols)],
                     log_cap)
        if trace_cap:
            self.trace_reserve(trace_cap)
        return self

    def _init(self, engine: Optional[Engine]) -> None:
        self._engine = engine or default_engine()
        self._h = None

    def _attach(self, h: C.c_void_p, shapes, log_cap: int) -> None:
        """shapes: (rows, cols, n) per LP, as lpr_batch_shape reports them."""
        self._h = h
        self._shapes = shapes
        # pairs kept per LP (include/lpr_engine.h: 0 means 4 * (rows + cols), at most 4096)
        self._log_caps = [int(log_cap) if log_cap > 0 else min(4096, 4 * (r + c))
                          for r, c, _ in shapes]
        self._basis = None
        self.Count = len(shapes)
        self.Status: List[Optional[int]] = [None] * self.Count
        self.FinalZ: List[float] = [0.0] * self.Count
        self.SolutionVector: List[Optional[List[float]]] = [None] * self.Count
        self.Iterations: List[int] = [0] * self.Count
        self.LastResult: Optional[N.BatchResult] = None
        self.TraceCap = 0  # records kept per LP; 0: untraced
        self._trace_info = None  # (records, offset, stride), read once per solve

    def trace_reserve(self, trace_cap: int) -> None:
        """Make the batch traced (lpr_batch_trace_reserve): only before the first Solve."""
        N.check(N.lib.lpr_batch_trace_reserve(self._h, int(trace_cap)), "lpr_batch_trace_reserve")
        self.TraceCap = int(trace_cap)
        self._trace_info = None

    def destroy(self) -> None:
        if self._h:
            N.lib.lpr_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- Solve :102-150, per LP ------------------------------------------------------------
    def Solve(self, max_pivots: int = 0, chunk: int = 0, variant: int = 0) -> N.BatchResult:
        opts = N.BatchOpts(max_pivots=int(max_pivots), chunk=int(chunk), variant=int(variant))
        res = N.BatchResult()
        N.check(N.lib.lpr_batch_solve(self._h, C.byref(opts), C.byref(res)), "lpr_batch_solve")
        self.LastResult = res
        self._basis = None
        self._trace_info = None
        st, piv, z = self.status_arrays()
        x = self.solution_packed()
        at = 0
        for k, (_, _, n) in enumerate(self._shapes):
            self.Status[k] = int(st[k])
            self.Iterations[k] = int(piv[k])
            if st[k] == N.LPR_OK_OPTIMAL:  # :110-126
                self.FinalZ[k] = float(z[k])
                self.SolutionVector[k] = [float(v) for v in x[at:at + n]]
            else:  # :129-135 keeps FinalZ = 0 and SolutionVector null
                self.FinalZ[k] = 0.0
                self.SolutionVector[k] = None
            at += n
        return res

    # -- bulk reads ------------------------------------------------------------------------
    def status_arrays(self):
        """(status int32[count], pivots int64[count], T[0, cols-1] float64[count])."""
        st = np.zeros(self.Count, dtype=np.int32)
        piv = np.zeros(self.Count, dtype=np.int64)
        z = np.zeros(self.Count, dtype=np.float64)
        N.check(N.lib.lpr_batch_status_read(self._h, _ptr(st, C.c_int32), _ptr(piv, C.c_int64),
                                            _ptr(z, C.c_double)), "lpr_batch_status_read")
        return st, piv, z

    def solution_packed(self) -> np.ndarray:
        x = np.zeros(max(sum(s[2] for s in self._shapes), 1), dtype=np.float64)
        N.check(N.lib.lpr_batch_solution_read(self._h, _ptr(x, C.c_double)),
                "lpr_batch_solution_read")
        return x[:sum(s[2] for s in self._shapes)]

    def basis_packed(self) -> np.ndarray:
        total = sum(s[0] - 1 for s in self._shapes)
        b = np.zeros(max(total, 1), dtype=np.int32)
        N.check(N.lib.lpr_batch_basis_read(self._h, _ptr(b, C.c_int32)), "lpr_batch_basis_read")
        return b[:total]

    # -- per-LP reads :18-24, 269-278 --------------------------------------------------------
    def Shape(self, k: int):
        """(rows, cols, n) of LP k."""
        return self._shapes[k]

    def BasicVariables(self, k: int) -> List[int]:
        if self._basis is None:  # one packed read per solve
            self._basis = self.basis_packed()
            self._basis_at = np.concatenate([[0], np.cumsum([s[0] - 1 for s in self._shapes])])
        at = int(self._basis_at[k])
        return [int(v) for v in self._basis[at:at + self._shapes[k][0] - 1]]

    def PivotLog(self, k: int, cap: Optional[int] = None) -> np.ndarray:
        """(row, column) of every pivot kept, row 1-based as in the console line of :138."""
        if cap is None:
            cap = self._log_caps[k]
        rows = np.zeros(max(cap, 1), dtype=np.int32)
        cols = np.zeros(max(cap, 1), dtype=np.int32)
        cnt = C.c_int64()
        N.check(N.lib.lpr_batch_log_read(self._h, int(k), _ptr(rows, C.c_int32),
                                         _ptr(cols, C.c_int32), int(cap), C.byref(cnt)),
                "lpr_batch_log_read")
        n = cnt.value
        return np.stack([rows[:n], cols[:n]], axis=1)

    def GetFinalTableau(self, k: int) -> np.ndarray:
        r, c, _ = self._shapes[k]
        out = np.empty((r, c), dtype=np.float64)
        N.check(N.lib.lpr_batch_tableau_read(self._h, int(k), _ptr(out, C.c_double)),
                "lpr_batch_tableau_read")
        return out

    # -- the trace --------------------------------------------------
    def trace_info(self):
        """(records, offset, stride), int64[count] each: the exact number of records of every LP
        (1 + pivots; min(records, TraceCap) are kept), where its records start in the trace slab
        and the doubles of one record.  Read once per solve: the per-LP accessors below share
        the arrays, so a loop over every LP of a large batch stays linear."""
        if self._trace_info is not None:
            return self._trace_info
        recs = np.zeros(self.Count, dtype=np.int64)
        off = np.zeros(self.Count, dtype=np.int64)
        stride = np.zeros(self.Count, dtype=np.int64)
        N.check(N.lib.lpr_batch_trace_info(self._h, _ptr(recs, C.c_int64), _ptr(off, C.c_int64),
                                           _ptr(stride, C.c_int64)), "lpr_batch_trace_info")
        for a in (recs, off, stride):
            a.setflags(write=False)
        self._trace_info = (recs, off, stride)
        return self._trace_info

    def trace_packed(self):
        """(slab, records, offset, stride): every LP's records in one copy."""
        recs, off, stride = self.trace_info()
        slab = np.zeros(int(self.TraceCap * stride.sum()), dtype=np.float64)
        N.check(N.lib.lpr_batch_trace_read_all(self._h, _ptr(slab, C.c_double), slab.size),
                "lpr_batch_trace_read_all")
        return slab, recs, off, stride

    def trace_read(self, k: int, first: int, n: int) -> np.ndarray:
        """Records [first, first + n) of LP k, one per row."""
        r, c, _ = self._shapes[k]
        out = np.zeros((max(int(n), 0), trace_stride(r, c)), dtype=np.float64)
        N.check(N.lib.lpr_batch_trace_read(self._h, int(k), int(first), int(n),
                                           _ptr(out, C.c_double)), "lpr_batch_trace_read")
        return out

    def _kept(self, k: int):
        """The kept records of LP k as (leaving_row, entering_col, tableau)."""
        r, c, _ = self._shapes[k]
        count = int(self.trace_info()[0][k])
        return [trace_record(rec, r, c) for rec in self.trace_read(k, 0, min(count, self.TraceCap))]

    def _ended(self, k: int) -> bool:
        return self.Status[k] in (N.LPR_OK_OPTIMAL, N.LPR_UNBOUNDED)

    def SnapshotCount(self, k: int) -> int:
        """Entries the C# list of LP k holds: one per record (may exceed TraceCap) and the final
        block of the optimal (:118-122) or unbounded (:133) exit."""
        return int(self.trace_info()[0][k]) + (1 if self._ended(k) else 0)

    def Snapshot(self, k: int, i: int):
        """Record i of LP k: (leaving_row, entering_col, tableau after i pivots)."""
        r, c, _ = self._shapes[k]
        return trace_record(self.trace_read(k, i, 1)[0], r, c)

    def IterationSnapshots(self, k: int) -> List[str]:  # :86, :148, :118-122, :133
        """The C#'s list of text blocks for LP k: "Initial Tableau", "Iteration i - After pivot"
        per kept record, then the final block from the LP's tableau in the batch (an LP stopped
        at the pivot limit has none)."""
        final = self.GetFinalTableau(k) if self._ended(k) else None
        return format_snapshots([T for _, _, T in self._kept(k)], self._shapes[k][2],
                                self.Status[k], final, self.FinalZ[k], self.SolutionVector[k])

    def ConsoleText(self, k: int) -> str:  # :117-148
        """What Solve() of LP k alone writes to the console, from the records' headers and
        tableaux (independent of log_cap).  The text of a solve has no gaps: an LP that made more
        records than TraceCap keeps raises ValueError instead of returning its first pivots
        followed by the exit lines."""
        count = int(self.trace_info()[0][k])
        if count > self.TraceCap:
            raise ValueError(f"LP {k} made {count} records and TraceCap keeps {self.TraceCap}: "
                             "its console text would miss pivots")
        return format_console(self._kept(k), self._shapes[k][2], self.Status[k], self.FinalZ[k],
                              self.SolutionVector[k])

    # -- device text ------------------------------------------------
    def FormatTrace(self) -> fmt.DeviceText:
        """Every kept record of every LP, and the final tableau of every LP that ended, as text
        blocks written on the device (lpr_batch_trace_text): one call, kept until the next
        ``Solve``.  ``first_block[k]`` of the result is where LP k's blocks start."""
        cached = getattr(self, "_text", None)
        if cached is not None and cached[0] is self.LastResult:
            return cached[1]
        if cached is not None:
            cached[1].destroy()
        first = np.zeros(self.Count + 1, dtype=np.int64)
        h = C.c_void_p()
        N.check(N.lib.lpr_batch_trace_text(self._h, _ptr(first, C.c_int64), C.byref(h)),
                "lpr_batch_trace_text")
        text = fmt.DeviceText(h)
        first.setflags(write=False)
        text.first_block = first
        self._text = (self.LastResult, text)
        return text

    def _bodies(self, k: int):
        """(bodies of LP k's kept records, body of its final tableau or None), from the device."""
        text = self.FormatTrace()
        at, end = int(text.first_block[k]), int(text.first_block[k + 1])
        kept = end - at - (1 if self._ended(k) else 0)
        return ([text.block(i) for i in range(at, at + kept)],
                text.block(at + kept) if self._ended(k) else None)

    def _headers(self, k: int, n: int):
        """(leaving_row, entering_col) of pivots 1 .. n - 1 of LP k: the pivot log when it kept
        them all, else the records' headers."""
        log = self.PivotLog(k)
        if len(log) >= n - 1:
            return [(int(r), int(e)) for r, e in log[:n - 1]]
        return [(r, e) for r, e, _ in self._kept(k)[1:n]]

    def IterationSnapshotsDevice(self, k: int) -> List[str]:
        """``IterationSnapshots(k)``, its tableau bodies formatted on the device."""
        bodies, final = self._bodies(k)
        return snapshots_from_bodies(bodies, self._shapes[k][2], self.Status[k], final,
                                     self.FinalZ[k], self.SolutionVector[k])

    def ConsoleTextDevice(self, k: int) -> str:
        """``ConsoleText(k)``, its tableau bodies formatted on the device; the same ValueError
        for an LP with more records than TraceCap keeps."""
        count = int(self.trace_info()[0][k])
        if count > self.TraceCap:
            raise ValueError(f"LP {k} made {count} records and TraceCap keeps {self.TraceCap}: "
                             "its console text would miss pivots")
        bodies, _ = self._bodies(k)
        return console_from_bodies(self._headers(k, len(bodies)), bodies, self._shapes[k][2],
                                   self.Status[k], self.FinalZ[k], self.SolutionVector[k])

    def all_snapshot_texts(self) -> List[List[str]]:
        """``IterationSnapshots`` of every LP, from one device call."""
        return [self.IterationSnapshotsDevice(k) for k in range(self.Count)]


def snapshots_from_bodies(bodies, numVariables: int, status: Optional[int] = None,
                          final_body: Optional[str] = None, final_z: float = 0.0,
                          solution=None) -> List[str]:
    """format_snapshots of primal_simplex_solver.py from Format bodies (Format without its title
    line) in place of tableaux: ``bodies[i]`` belongs to the tableau after i pivots."""
    out = [fmt.title_line("Initial Tableau" if i == 0 else f"Iteration {i} - After pivot") + body
           for i, body in enumerate(bodies)]
    if status == N.LPR_OK_OPTIMAL:  # :118-122
        out.append(fmt.title_line("Final Tableau (Optimal)") + final_body + fmt.NEWLINE +
                   solution_summary(final_z, solution, numVariables) + fmt.NEWLINE)
    elif status == N.LPR_UNBOUNDED:  # :133
        out.append(fmt.title_line("Unbounded Tableau") + final_body)
    return out


def console_from_bodies(headers, bodies, numVariables: int, status: Optional[int] = None,
                        final_z: float = 0.0, solution=None) -> str:
    """format_console of primal_simplex_solver.py from Format bodies: ``headers[i - 1]`` is the
    (leaving_row, entering_col) of pivot i, ``bodies[i]`` the body of the tableau after it."""
    nl = fmt.NEWLINE
    out = []
    for i in range(1, len(bodies)):
        r, e = headers[i - 1]
        label = col_label(int(e), numVariables)
        out.append(f"\nIteration {i}: pivot @ constraint {int(r)}, column {label}" + nl)
        out.append(fmt.title_line("Before pivot") + bodies[i - 1] + nl)
        out.append(f"After pivot (constraint {int(r)}, column {label}):" + nl)
        out.append(fmt.title_line("After pivot") + bodies[i] + nl)
    if status == N.LPR_OK_OPTIMAL:
        out.append("Optimal Solution Found!" + nl)
        out.append(solution_summary(final_z, solution, numVariables) + nl)
        out.append("-" * 100 + nl)
    elif status == N.LPR_UNBOUNDED:
        out.append("Unbounded Solution!" + nl)
    return "".join(out)
