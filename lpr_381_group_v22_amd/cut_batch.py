"""Many cutting-plane runs in one call (lpr_cut_batch_*).

Every item of a batch is one tableau (row 0 = objectiveRow, rows 1.. = constraintRows) taken
through the whole ``CuttingPlaneSolver.CuttingPlaneSolution`` recursion of
IntegerProgramming/CuttingPlaneSolver.cs on the MI355X, with no host step per cut or per pivot,
and ends with the bits ``Tableau.cutting_plane`` (lpr_cutting_plane) gives for it alone.
``Run(mode=MODE_DUAL)`` / ``Run(mode=MODE_PRIMAL2)`` are ``Tableau.dual_solve`` /
``Tableau.primal2_solve`` per item.  The reference has no batch mode: the per-item accessors
below are named after the single-handle surface (engine.py).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from ._native import _ptr
from . import table_iteration_formater as fmt
from .engine import Engine, default_engine
from .primal_batch import PrimalSimplexBatch

MODE_CUTTING_PLANE, MODE_DUAL, MODE_PRIMAL2 = 0, 1, 2   # lpr_cut_batch_opts.mode
FORM_G, FORM_H = 1, 2
VARIANT_G, VARIANT_H = 2, 3      # lpr_cut_batch_opts.variant
DEFAULT_MAX_CUTS = 64            # max_cuts <= 0, as lpr_cutting_plane
MAX_ROWS_H = 1024                # at full row capacity: rows + max_cuts
MAX_COLS_H = 2048
MAX_LDS_G = 160 * 1024 - 1024    # kBatchMaxLdsG
LOG_DEFAULT_MAX = 4096           # kBatchLogDefaultMax
CHUNK = {FORM_G: 128, FORM_H: 16}  # kCutBatchChunk: pivots per item per launch

# ---- narration; csrc/cut_narr_layout.hpp restated --------------------------
# Per item: events of four int32 (kind, a, b, rows_now) -- the count exact, the first ev_cap kept --
# and blocks of doubles back to back in event order: block 0 the rows x cols tableau at reserve
# time, one block per EV_CUT (the appended row, cols doubles) and per pivot event (the whole
# rows_now x cols tableau after it).  A block that does not fit whole is counted and not written,
# and so is every later one (the rule of csrc/kept_prefix.hpp).
EV_CALL, EV_LEVEL, EV_CUT, EV_SOLVE_BEGIN, EV_SOLVE_END, EV_EXIT = 0, 1, 2, 3, 4, 5
EV_PIVOT = 8                     # + the log kind: 8 dual, 9 primal2, 10 cut
KIND_DUAL, KIND_PRIMAL2, KIND_CUT = 0, 1, 2
ST_OK, ST_UNBOUNDED, ST_INFEASIBLE, ST_PIVOT_TOO_SMALL, ST_PIVOT_LIMIT = 0, 1, 2, 3, 5


def event_doubles(kind: int, rows_now: int, cols: int) -> int:
    """cut_narr_event_doubles: the doubles of the block an event adds."""
    if kind == EV_CUT:
        return cols
    return rows_now * cols if kind >= EV_PIVOT else 0


def block_offsets(events, rows0: int, cols: int) -> List[Tuple[int, int]]:
    """(offset, doubles) of every block the events make, block 0 first: the prefix sum of
    event_doubles."""
    out = [(0, rows0 * cols)]
    at = rows0 * cols
    for kind, _a, _b, rows_now in events:
        n = event_doubles(kind, rows_now, cols)
        if n:
            out.append((at, n))
            at += n
    return out


def narr_push(c: dict, n: int) -> int:
    """kept_push (csrc/kept_prefix.hpp) on a dict of cursors (cap, cur, made_d, and made_b /
    kept_b for KeptPrefix's made_n / kept_n): where the block goes, or -1 where it is only
    counted."""
    keep = c["kept_b"] == c["made_b"] and n <= c["cap"] - c["cur"]
    at = c["cur"] if keep else -1
    c["made_b"] += 1
    c["made_d"] += n
    if keep:
        c["kept_b"] += 1
        c["cur"] += n
    return at


class NarrationInfo(NamedTuple):
    """lpr_cut_batch_narrate_info, per item."""
    events_made: np.ndarray
    doubles_made: np.ndarray
    doubles_kept: np.ndarray
    data_off: np.ndarray


class NarrationStopped(ValueError):
    """The item has no complete C# text: it kept less than it made, or it ended where the
    reference cannot (the cut limit, an escaped exception, a hard_cap stop)."""


_DUAL_END = {ST_OK: "Dual phase complete: all RHS >= 0.",                          # :42
             ST_INFEASIBLE: "Infeasible: pivot row has no negative coefficients with non-zero "
                            "ratios.",                                             # :74
             ST_PIVOT_LIMIT: "Max iterations reached."}                            # :110
_PRIMAL2_END = {ST_OK: "Optimal reached.",                                         # :58
                ST_UNBOUNDED: "Unbounded: no valid leaving row.",                  # :65
                ST_PIVOT_LIMIT: "Max iterations reached."}                         # :92


def _h4_row(row) -> str:
    return "\t".join(fmt.H4(float(v)) for v in row)


def format_cutting_plane(events, record0, blocks, newline: str = "\n",
                         partial: bool = False) -> str:
    """WHAT THE C# WRITES to the console in CuttingPlaneSolver.CuttingPlaneSolution
    (IntegerProgramming/CuttingPlaneSolver.cs:47-54, 64-229, the recursion unrolled) and in the
    two clean-up solvers under printSteps (Simplex/DualSimplex.cs:14-114, 193-207, 228-239;
    Simplex/PrimalSimplexSolver2.cs:46-97, 184-189), from numbers alone: ``events`` are the
    (kind, a, b, rows_now) quads of one item, ``record0`` its tableau at reserve time and
    ``blocks`` the data blocks after it in event order (a 1-D row per EV_CUT, a 2-D tableau per
    pivot).  Pure: no device, and no control flow beyond walking the events -- which branch was
    taken is what the events say.  In modes 1 and 2 (EV_CALL's a) the text is that of
    Solve(printSteps) alone.  Raises NarrationStopped where the text cannot go on: a block is
    missing, or the item ended at exit 6, exit 7 or a hard_cap stop, which the reference cannot
    reach; with ``partial`` the text up to there is returned.  ``newline`` ends every
    Console.WriteLine (TableIterationFormater.Format keeps its own Environment.NewLine)."""
    out: List[str] = []
    T = np.array(record0, dtype=np.float64, copy=True)
    nxt = iter(blocks)
    mode, steps, fresh, solver, it = MODE_CUTTING_PLANE, True, True, None, 0

    def emit(s: str = "") -> None:
        out.append(s + newline)

    def print_tableau(title: str) -> None:  # CuttingPlaneSolver.PrintTableau :47-54
        emit(title)
        emit("z:  " + _h4_row(T[0]))
        for i in range(1, T.shape[0]):
            emit(f"r{i}: " + _h4_row(T[i]))
        emit()

    def num_vars() -> int:  # DualSimplex.cs:228-234
        return T.shape[1] - 1 - (T.shape[0] - 1)

    def dual_tableau() -> None:  # DualSimplex.cs:193-207
        emit(fmt.Format(T, num_vars(), "Dual Simplex Tableau"))

    def primal2_tableau() -> None:  # PrimalSimplexSolver2.cs:184-189
        emit("OBJ: " + _h4_row(T[0]))
        for i in range(1, T.shape[0]):
            emit(f"r{i}: " + _h4_row(T[i]))

    class _Stop(Exception):
        pass

    if not partial:  # an ending without C# text is refused before anything is formatted
        m = MODE_CUTTING_PLANE
        for kind, a, b, _r in events:
            if kind == EV_CALL:
                m = a
            elif (kind == EV_SOLVE_END and (b or a == ST_PIVOT_TOO_SMALL)) or \
                    (kind == EV_EXIT and m == MODE_CUTTING_PLANE and a in (6, 7)):
                raise NarrationStopped("the item ended at exit 6, exit 7 or a hard_cap stop: the "
                                       "reference has no text for that (partial=True gives the "
                                       "text up to there)")

    def block(shape):
        b = next(nxt, None)
        if b is None:
            raise _Stop("a data block was not kept")
        return np.asarray(b, dtype=np.float64).reshape(shape)

    try:
        for kind, a, b, rows_now in events:
            if kind == EV_CALL:
                mode, steps, fresh = a, (bool(b) if a != MODE_CUTTING_PLANE else True), True
            elif kind == EV_LEVEL:
                if not fresh:                                                       # :219
                    emit("Objective optimal but RHS has fractional values \u2192 adding another "
                         "Gomory cut...")
                fresh = False
                print_tableau("Initial tableau:")                                   # :74
            elif kind == EV_CUT:
                T = np.vstack([T, block((1, T.shape[1]))])                          # :110
            elif kind == EV_SOLVE_BEGIN:
                solver, it = a, 0
                if mode == MODE_CUTTING_PLANE:
                    emit("Negative RHS detected \u2192 running Dual Simplex..." if a == KIND_DUAL
                         else "Negative reduced cost detected \u2192 running Primal "
                              "Simplex...")                                         # :188 / :198
            elif kind == EV_PIVOT + KIND_CUT:
                where = f"row {a + 1}, col {b + 1}"
                print_tableau("Before pivot on cut: " + where)                      # :141-143
                T = block((rows_now, T.shape[1]))
                print_tableau("After pivot on cut: " + where)                       # :178-180
            elif kind == EV_PIVOT + KIND_DUAL:
                if steps:                                                           # :91-96
                    it += 1
                    n = num_vars()
                    label = f"x{b + 1}" if b < n else f"t{b - n + 1}"               # :236-239
                    emit(f"\nIteration {it}: pivot @ constraint {a + 1}, column {label}")
                    dual_tableau()
                T = block((rows_now, T.shape[1]))
                if steps:                                                           # :100-105
                    emit("After pivot:")
                    dual_tableau()
            elif kind == EV_PIVOT + KIND_PRIMAL2:
                if steps:                                                           # :73-77
                    it += 1
                    emit(f"\nIter {it}: pivot @ row {a}, col {b}")
                    primal2_tableau()
                T = block((rows_now, T.shape[1]))
                if steps:                                                           # :84-88
                    emit("After pivot:")
                    primal2_tableau()
            elif kind == EV_SOLVE_END:
                if b or a == ST_PIVOT_TOO_SMALL:
                    raise _Stop("a hard_cap stop" if b else
                                "InvalidOperationException: Pivot too small/zero")
                if steps:
                    emit((_DUAL_END if solver == KIND_DUAL else _PRIMAL2_END)[a])
                if mode == MODE_CUTTING_PLANE:
                    if solver == KIND_PRIMAL2:
                        print_tableau("After Primal Simplex:")                      # :211
                    elif a == ST_OK:
                        print_tableau("After Dual Simplex:")                        # :192
                    else:
                        emit("Dual Simplex failed (infeasible or max iters).")      # :191
            elif kind == EV_EXIT:
                if mode != MODE_CUTTING_PLANE:
                    continue
                if a == 0:
                    emit("Displayed the Optimal Tableau.")                          # :224
                elif a == 1:
                    emit("All RHS are integers. No Gomory cut needed.")             # :89
                elif a == 2:
                    emit("No valid pivot column on the cut (need a negative cut coeff with "
                         "non-zero obj coeff).")                                    # :136
                elif a == 3:
                    print_tableau(f"Before pivot on cut: row {rows_now - 1}, col {b + 1}")
                    emit("Pivot too small/zero.")                                   # :148
                elif a == 5:
                    emit("Cutting-plane step finished (further steps may be required).")  # :228
                elif a != 4:
                    raise _Stop(f"exit {a}")
            else:
                raise ValueError(f"unknown event kind {kind}")
    except _Stop as e:
        if not partial:
            raise NarrationStopped(f"no C# text beyond this point: {e}") from None
    return "".join(out)


def format_primal2_snapshots(events, record0, blocks) -> List[str]:
    """PrimalSimplexSolver2.IterationSnapshots (PrimalSimplexSolver2.cs:51, :71, :82, :168-182)
    of the LAST mode-2 call among ``events``: "Start of iter {iter}" at the head of every pass,
    "Before pivot (iter {iter + 1}) ..." and "After pivot (iter {iter}) ..." around every pivot,
    each with "Current Tableau:" in 0.###.  `iter` moves only under printSteps (:75), as in the
    C#.  A hard_cap stop has no C# counterpart: the list ends with the pass that met it."""
    T = np.array(record0, dtype=np.float64, copy=True)
    nxt = iter(blocks)
    nl = fmt.NEWLINE
    snaps: List[str] = []
    mode, steps, it, pending = MODE_CUTTING_PLANE, True, 0, False

    def capture(title: str) -> None:
        rows = [title, "Current Tableau:",
                "OBJ\t" + "\t".join(fmt.H3(float(v)) for v in T[0])]
        rows += [f"r{i}\t" + "\t".join(fmt.H3(float(v)) for v in T[i])
                 for i in range(1, T.shape[0])]
        snaps.append("".join(r + nl for r in rows))

    for kind, a, b, rows_now in events:
        if kind == EV_CALL:
            mode, steps = a, (bool(b) if a != MODE_CUTTING_PLANE else True)
            if mode == MODE_PRIMAL2:
                snaps, it, pending = [], 0, True
        live = mode == MODE_PRIMAL2
        if kind == EV_CUT or kind >= EV_PIVOT:
            blk = next(nxt, None)
            if blk is None:
                raise NarrationStopped("a data block was not kept")
            if live and pending:
                capture(f"Start of iter {it}")                                      # :51
            if live:
                capture(f"Before pivot (iter {it + 1}) at row {a}, col {b}")        # :71
                if steps:
                    it += 1
            T = (np.vstack([T, np.asarray(blk).reshape(1, -1)]) if kind == EV_CUT
                 else np.asarray(blk, dtype=np.float64).reshape(rows_now, T.shape[1]))
            if live:
                capture(f"After pivot (iter {it}) at row {a}, col {b}")             # :82
                pending = True
        elif kind == EV_SOLVE_END and live:
            if pending and not (a == ST_PIVOT_LIMIT and not b):  # :90 returns behind the pivot
                capture(f"Start of iter {it}")
            pending = False
    return snaps


def max_cuts_of(max_cuts: int) -> int:
    """The row capacity a handle adds per item: <= 0 is 64."""
    return int(max_cuts) if int(max_cuts) > 0 else DEFAULT_MAX_CUTS


def footprint_g(rows: int, cols: int, max_cuts: int) -> int:
    """Bytes of dynamic LDS an item needs in form G (cut_batch_footprint_g): the tableau at full
    row capacity, the factor column and the pivot row."""
    rcap = rows + max_cuts_of(max_cuts)
    return 8 * (rcap * cols + rcap + cols)


def fits_g(rows: int, cols: int, max_cuts: int) -> bool:
    return footprint_g(rows, cols, max_cuts) <= MAX_LDS_G


def form_of(rows: int, cols: int, max_cuts: int, variant: int = 0) -> int:
    """The form batch_pick_form gives an item (no form W)."""
    if variant == VARIANT_H:
        return FORM_H
    return FORM_G if fits_g(rows, cols, max_cuts) else FORM_H


def launches_for(pivots: int, chunk: int) -> int:
    """Launches of an item that performs ``pivots`` pivots in one call and ends without a refused
    pivot pending: it stops only in front of pivot chunk + 1, 2 chunk + 1, ..."""
    return max(1, -(-int(pivots) // int(chunk)))


class PackedTableaux(NamedTuple):
    """The packed arrays of lpr_cut_batch_create."""
    rows: np.ndarray      # int32, per item
    cols: np.ndarray      # int32, per item
    tableaux: np.ndarray  # float64, rows x cols row-major blocks


def pack_tableaux(tableaux: Sequence[np.ndarray], max_cuts: int = 0) -> PackedTableaux:
    """Tableaux -> the packed ABI arrays, with the checks of lpr_cut_batch_create (raises
    ValueError where the call would refuse the batch)."""
    cap = max_cuts_of(max_cuts)
    T = []
    for k, t in enumerate(tableaux):
        try:
            a = np.ascontiguousarray(t, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"item {k}: the tableau is not a rectangular array of numbers") \
                from None
        if a.ndim != 2:
            raise ValueError(f"item {k}: the tableau is not a 2-D array (ragged rows?)")
        T.append(a)
    if not T:
        raise ValueError("no tableaux")
    for k, t in enumerate(T):
        r, c = t.shape
        if r < 2 or c < 2:
            raise ValueError(f"item {k}: a {r} x {c} tableau; it needs rows >= 2 and cols >= 2")
        if r + cap > MAX_ROWS_H or c > MAX_COLS_H:
            raise ValueError(f"item {k}: a {r} x {c} tableau is {r + cap} x {c} with max_cuts "
                             f"{cap}, beyond {MAX_ROWS_H} x {MAX_COLS_H}; run it with "
                             f"Tableau.cutting_plane")
    return PackedTableaux(np.asarray([t.shape[0] for t in T], dtype=np.int32),
                          np.asarray([t.shape[1] for t in T], dtype=np.int32),
                          np.concatenate([t.reshape(-1) for t in T]))


class CuttingPlaneBatch:
    """``count`` cutting-plane tableaux in one device handle (lpr_cut_batch_*)."""

    def __init__(self, handle: C.c_void_p, engine: Engine, count: int, max_cuts: int):
        self._h = handle
        self._engine = engine
        self.Count = int(count)
        self.max_cuts = max_cuts_of(max_cuts)
        self.LastResult: Optional[N.CutBatchResult] = None
        self._narr_shape: Optional[List[Tuple[int, int]]] = None  # (rows, cols) at reserve time
        self._ev_cap = 0
        self._caps_total = 0

    @classmethod
    def from_arrays(cls, engine: Optional[Engine], tableaux: Sequence[np.ndarray],
                    max_cuts: int = 0, log_cap: int = 0) -> "CuttingPlaneBatch":
        """objectiveRow + constraintRows per item (:64-70), from host arrays."""
        p = pack_tableaux(tableaux, max_cuts)
        eng = engine or default_engine()
        h = C.c_void_p()
        N.check(N.lib.lpr_cut_batch_create(eng._h, len(p.rows), _ptr(p.rows, C.c_int32),
                                           _ptr(p.cols, C.c_int32), _ptr(p.tableaux, C.c_double),
                                           int(max_cuts), int(log_cap), C.byref(h)),
                "lpr_cut_batch_create")
        return cls(h, eng, len(p.rows), max_cuts)

    @classmethod
    def from_primal_batch(cls, batch: PrimalSimplexBatch, max_cuts: int = 0,
                          log_cap: int = 0) -> "CuttingPlaneBatch":
        """The FinalTableau of every LP of a solved PrimalSimplexBatch, device to device.  The new
        handle does not depend on ``batch`` staying alive."""
        h = C.c_void_p()
        N.check(N.lib.lpr_cut_batch_from_batch(batch._h, int(max_cuts), int(log_cap), C.byref(h)),
                "lpr_cut_batch_from_batch")
        return cls(h, batch._engine, batch.Count, max_cuts)

    def destroy(self) -> None:
        if self._h:
            N.lib.lpr_cut_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- one lpr_cutting_plane / lpr_dual_solve / lpr_primal2_solve per item --------------------
    def Run(self, mode: int = MODE_CUTTING_PLANE, max_cuts: int = 0, hard_cap: int = 0,
            max_iters: int = 10000, print_steps: Optional[bool] = None, chunk: int = 0,
            variant: int = 0) -> N.CutBatchResult:
        """print_steps defaults as the single calls do: on for the dual, off for primal2."""
        if print_steps is None:
            print_steps = mode != MODE_PRIMAL2
        opts = N.CutBatchOpts(mode=int(mode), max_cuts=int(max_cuts), hard_cap=int(hard_cap),
                              max_iters=int(max_iters), print_steps=1 if print_steps else 0,
                              chunk=int(chunk), variant=int(variant))
        res = N.CutBatchResult()
        N.check(N.lib.lpr_cut_batch_run(self._h, C.byref(opts), C.byref(res)),
                "lpr_cut_batch_run")
        self.LastResult = res
        return res

    # -- bulk reads -----------------------------------------------------------------------------
    def result_arrays(self) -> dict:
        """Per item: code (exit code in mode 0, lpr_status in modes 1 / 2) and cuts of the last
        call, rows now, log triples so far, z = T[0, cols - 1]."""
        n = self.Count
        out = dict(code=np.zeros(n, dtype=np.int32), cuts=np.zeros(n, dtype=np.int32),
                   rows=np.zeros(n, dtype=np.int32), log_count=np.zeros(n, dtype=np.int64),
                   z=np.zeros(n, dtype=np.float64))
        N.check(N.lib.lpr_cut_batch_result_read(
            self._h, _ptr(out["code"], C.c_int32), _ptr(out["cuts"], C.c_int32),
            _ptr(out["rows"], C.c_int32), _ptr(out["log_count"], C.c_int64)),
            "lpr_cut_batch_result_read")
        N.check(N.lib.lpr_cut_batch_z_read(self._h, _ptr(out["z"], C.c_double)),
                "lpr_cut_batch_z_read")
        return out

    # -- per-item reads -------------------------------------------------------------------------
    def _shape4(self, k: int) -> Tuple[int, int, int, int]:
        r, c, rc, lc = (C.c_int32() for _ in range(4))
        N.check(N.lib.lpr_cut_batch_shape(self._h, int(k), C.byref(r), C.byref(c), C.byref(rc),
                                          C.byref(lc)), "lpr_cut_batch_shape")
        return r.value, c.value, rc.value, lc.value

    def Shape(self, k: int) -> Tuple[int, int]:
        """(rows now, cols) of item k."""
        return self._shape4(k)[:2]

    def LogCap(self, k: int) -> int:
        return self._shape4(k)[3]

    def Tableau(self, k: int) -> np.ndarray:
        T = np.empty(self.Shape(k), dtype=np.float64)
        N.check(N.lib.lpr_cut_batch_tableau_read(self._h, int(k), _ptr(T, C.c_double)),
                "lpr_cut_batch_tableau_read")
        return T

    def Log(self, k: int, cap: Optional[int] = None) -> List[Tuple[int, int, int]]:
        """The (kind, row, column) triples kept for item k; LogCount gives the exact total."""
        lc = self.LogCap(k)
        cap = lc if cap is None else int(cap)
        buf = np.zeros(max(3 * cap, 3), dtype=np.int32)
        cnt = C.c_int64()
        N.check(N.lib.lpr_cut_batch_log_read(self._h, int(k), _ptr(buf, C.c_int32), cap,
                                             C.byref(cnt)), "lpr_cut_batch_log_read")
        n = min(cnt.value, cap, lc)
        return [tuple(t) for t in buf[:3 * n].reshape(-1, 3).tolist()]

    def LogCount(self, k: int) -> int:
        cnt = C.c_int64()
        N.check(N.lib.lpr_cut_batch_log_read(self._h, int(k), None, 0, C.byref(cnt)),
                "lpr_cut_batch_log_read")
        return cnt.value

    # -- narration -------------------------------------------------------
    def narrate_reserve(self, cap, ev_cap: int) -> None:
        """Makes the handle narrated, before its first Run: ``cap`` doubles of tableau data per
        item (one number for all, or one per item) and ``ev_cap`` events per item.  Caps of 0
        keep nothing and count everything (narration_info)."""
        caps = np.ascontiguousarray(np.broadcast_to(np.asarray(cap, dtype=np.int64),
                                                    (self.Count,)))
        shapes = [self.Shape(k) for k in range(self.Count)]
        N.check(N.lib.lpr_cut_batch_narrate_reserve(self._h, caps.ctypes.data_as(
            C.POINTER(C.c_int64)), int(ev_cap)), "lpr_cut_batch_narrate_reserve")
        self._narr_shape, self._ev_cap, self._caps_total = shapes, int(ev_cap), int(caps.sum())

    def narration_info(self) -> NarrationInfo:
        a = [np.zeros(self.Count, dtype=np.int64) for _ in range(4)]
        N.check(N.lib.lpr_cut_batch_narrate_info(self._h, *(_ptr(x, C.c_int64) for x in a)),
                "lpr_cut_batch_narrate_info")
        return NarrationInfo(*a)

    def Events(self, k: int) -> List[Tuple[int, int, int, int]]:
        """The (kind, a, b, rows_now) events kept for item k; narration_info gives the total."""
        cnt = C.c_int64()
        N.check(N.lib.lpr_cut_batch_narrate_events_read(self._h, int(k), None, 0, C.byref(cnt)),
                "lpr_cut_batch_narrate_events_read")
        n = min(cnt.value, self._ev_cap)
        buf = np.zeros(max(4 * n, 4), dtype=np.int32)
        N.check(N.lib.lpr_cut_batch_narrate_events_read(self._h, int(k), _ptr(buf, C.c_int32), n,
                                                        C.byref(cnt)),
                "lpr_cut_batch_narrate_events_read")
        return [tuple(t) for t in buf[:4 * n].reshape(-1, 4).tolist()]

    def NarrationData(self, k: int, first: int, n: int) -> np.ndarray:
        out = np.zeros(max(int(n), 1), dtype=np.float64)
        N.check(N.lib.lpr_cut_batch_narrate_data_read(self._h, int(k), int(first), int(n),
                                                      _ptr(out, C.c_double)),
                "lpr_cut_batch_narrate_data_read")
        return out[:int(n)]

    @staticmethod
    def _split(events, shape, data: np.ndarray):
        """Block 0 and the kept blocks after it, out of the kept doubles of one item."""
        rows0, cols = shape
        blocks = []
        for (at, n), ev in zip(block_offsets(events, rows0, cols),
                               [None] + [e for e in events if event_doubles(e[0], e[3], cols)]):
            if at + n > data.size:
                break
            blk = data[at:at + n]
            blocks.append(blk.reshape(rows0, cols) if ev is None else
                          (blk.copy() if ev[0] == EV_CUT else blk.reshape(ev[3], cols)))
        return (blocks[0] if blocks else None), blocks[1:]

    def NarrationBlocks(self, k: int):
        """(block 0, [the kept blocks after it]) of item k: a 1-D row per cut, a 2-D tableau per
        pivot."""
        kept = int(self.narration_info().doubles_kept[k])
        return self._split(self.Events(k), self._narr_shape[k], self.NarrationData(k, 0, kept))

    def narration_packed(self) -> Tuple[np.ndarray, np.ndarray]:
        """Everything in two copies (lpr_cut_batch_narrate_read_all): the events as a count x
        ev_cap x 4 array and the data slab, item k at narration_info().data_off[k]."""
        ev = np.zeros((self.Count, self._ev_cap, 4), dtype=np.int32)
        total = self._caps_total
        data = np.zeros(max(total, 1), dtype=np.float64)
        N.check(N.lib.lpr_cut_batch_narrate_read_all(self._h, _ptr(ev, C.c_int32),
                                                     ev.size // 4, _ptr(data, C.c_double), total),
                "lpr_cut_batch_narrate_read_all")
        return ev, data[:total]

    def _item_numbers(self, k: int, info: NarrationInfo, packed=None):
        made_e, made_d, kept_d = (int(info.events_made[k]), int(info.doubles_made[k]),
                                  int(info.doubles_kept[k]))
        if packed is None:
            events = self.Events(k)
            data = self.NarrationData(k, 0, kept_d)
        else:
            ev, slab = packed
            events = [tuple(t) for t in ev[k, :min(made_e, self._ev_cap)].tolist()]
            at = int(info.data_off[k])
            data = slab[at:at + kept_d]
        rec0, blocks = self._split(events, self._narr_shape[k], data)
        return events, rec0, blocks, (len(events) < made_e or kept_d < made_d)

    def NarrationText(self, k: int, newline: str = "\n", partial: bool = False,
                      _info=None, _packed=None) -> str:
        """The console text of CuttingPlaneSolution (or, in modes 1 / 2, of Solve(printSteps)) for
        item k over the handle's life (format_cutting_plane).  Raises NarrationStopped where the
        item kept fewer events or doubles than it made, or ended at exit 6, exit 7 or a hard_cap
        stop; ``partial`` returns the text up to there."""
        info = _info or self.narration_info()
        events, rec0, blocks, short = self._item_numbers(k, info, _packed)
        if rec0 is None or (short and not partial):
            if partial:
                return ""
            raise NarrationStopped(f"item {k} kept fewer events or doubles than it made "
                                   f"(narration_info)")
        text = format_cutting_plane(events, rec0, blocks, newline, partial=partial)
        return text

    def Snapshots(self, k: int) -> List[str]:
        """PrimalSimplexSolver2.IterationSnapshots of item k's last mode-2 Run
        (format_primal2_snapshots)."""
        info = self.narration_info()
        events, rec0, blocks, short = self._item_numbers(k, info)
        if rec0 is None or short:
            raise NarrationStopped(f"item {k} kept fewer events or doubles than it made")
        return format_primal2_snapshots(events, rec0, blocks)


def cutting_plane_texts(tableaux: Sequence[np.ndarray], max_cuts: int = 0, hard_cap: int = 0,
                        engine: Optional[Engine] = None, newline: str = "\n",
                        partial: bool = False) -> List[str]:
    """The console text of CuttingPlaneSolution for every tableau.  Two handles: the first runs
    with caps of 0 and counts what each item makes, the second reserves exactly that and keeps it
    (a run is deterministic, and a batch continues from its state, so the two passes cannot
    share a handle)."""
    count = CuttingPlaneBatch.from_arrays(engine, tableaux, max_cuts)
    try:
        count.narrate_reserve(0, 1)
        count.Run(hard_cap=hard_cap)
        need = count.narration_info()
    finally:
        count.destroy()
    keep = CuttingPlaneBatch.from_arrays(engine, tableaux, max_cuts)
    try:
        keep.narrate_reserve(need.doubles_made, max(1, int(need.events_made.max())))
        keep.Run(hard_cap=hard_cap)
        info, packed = keep.narration_info(), keep.narration_packed()
        return [keep.NarrationText(k, newline, partial, _info=info, _packed=packed)
                for k in range(keep.Count)]
    finally:
        keep.destroy()
