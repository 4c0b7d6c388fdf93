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


def _ptr(a: Optional[np.ndarray], ctype):
    return None if a is None or not a.size else a.ctypes.data_as(C.POINTER(ctype))


class CuttingPlaneBatch:
    """``count`` cutting-plane tableaux in one device handle (lpr_cut_batch_*)."""

    def __init__(self, handle: C.c_void_p, engine: Engine, count: int, max_cuts: int):
        self._h = handle
        self._engine = engine
        self.Count = int(count)
        self.max_cuts = max_cuts_of(max_cuts)
        self.LastResult: Optional[N.CutBatchResult] = None

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
