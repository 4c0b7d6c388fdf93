"""One solved model, many what-if scripts in one call (lpr_sens_batch_*).

A scenario is a private copy of a base ``SensState`` plus a script: a list of ``(op_name, *args)``
whose op names are the ``SensState`` method names.  Every script runs on the MI355X with no host
step per edit or per pivot and ends with the bits the same calls give on a fresh ``SensState``
holding the base state.  The reference (SensitivityAnalysis/SensitivityAnalyzer.cs) has no batch
mode: the per-scenario accessors below are named after the single-handle surface (engine.py).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .engine import RangingReport, SensState

# op name -> (code, number of integer arguments, takes a value)
EDIT_OPS = {
    "resolve_all": (N.LPR_SENS_EDIT_RESOLVE_ALL, 0, False),
    "change_nonbasic_cbar": (N.LPR_SENS_EDIT_NONBASIC_CBAR, 1, True),
    "change_basic": (N.LPR_SENS_EDIT_BASIC, 1, True),
    "change_rhs": (N.LPR_SENS_EDIT_RHS, 1, True),
    "change_nonbasic_column": (N.LPR_SENS_EDIT_NONBASIC_COLUMN, 2, True),
}
SHAPE_CHANGING_OPS = ("add_activity", "add_constraint")
NO_BASIC_ENTRY = -2 ** 31        # basicVars past a scenario's own rows in a grow batch's bulk read
MAX_ROWS_H = 1024
MAX_COLS_H = 2048
FORM_G, FORM_H = 1, 2            # lpr_sens_batch_result.form
VARIANT_G, VARIANT_H = 2, 3      # lpr_sens_batch_opts.variant
EDIT_NOT_RUN = -100
MAX_LDS_G = 160 * 1024 - 1024    # kBatchMaxLdsG


def footprint_g(rows: int, cols: int) -> int:
    """Bytes of dynamic LDS a scenario needs in form G (sens_batch_footprint_g): the tableau, the
    factor column and the pivot row in doubles, the membership counts and basicVars in int32."""
    aux = 8 * (rows + cols) + 4 * (cols + rows - 1)
    return 8 * rows * cols + ((aux + 7) & ~7)


def fits_g(rows: int, cols: int) -> bool:
    return footprint_g(rows, cols) <= MAX_LDS_G


EDIT_DTYPE = np.dtype([("op", np.int32), ("a", np.int32), ("b", np.int32),
                       ("reserved", np.int32), ("v", np.float64)])


class PackedScripts(NamedTuple):
    """The packed arrays of lpr_sens_batch_create."""
    nedits: np.ndarray   # int32, per scenario
    edits: np.ndarray    # EDIT_DTYPE (the layout of lpr_sens_edit), packed by nedits


def _int32(x, what: str) -> int:
    i = int(x)
    if i != x:
        raise ValueError(f"{what}: {x!r} is not an integer")
    # an index the int32 of lpr_sens_edit cannot hold is out of range on any tableau
    return max(-2 ** 31, min(2 ** 31 - 1, i))


def _pack_edit(name: str, args: tuple, where: str) -> tuple:
    """One shape-keeping edit as a record of EDIT_DTYPE."""
    if name not in EDIT_OPS:
        raise ValueError(f"{where}: unknown op {name!r}")
    code, nint, has_v = EDIT_OPS[name]
    if len(args) != nint + (1 if has_v else 0):
        raise ValueError(f"{where}: {name} takes {nint + has_v} arguments, got {len(args)}")
    ints = [_int32(a, where) for a in args[:nint]] + [0, 0]
    return (code, ints[0], ints[1], 0, float(args[nint]) if has_v else 0.0)


def pack_scripts(scripts: Sequence[Sequence[tuple]]) -> PackedScripts:
    """Scripts -> the packed ABI arrays, with the checks of lpr_sens_batch_create (raises
    ValueError where the call would refuse the batch): at least one scenario, known ops, and no op
    that changes the tableau's shape."""
    if len(scripts) < 1:
        raise ValueError("no scenarios")
    nedits = np.zeros(len(scripts), dtype=np.int32)
    flat = []
    for k, script in enumerate(scripts):
        nedits[k] = len(script)
        for q, edit in enumerate(script):
            name, args = edit[0], tuple(edit[1:])
            if len(args) == 1 and isinstance(args[0], (tuple, list)):
                args = tuple(args[0])    # (op, (args...)) as the test scripts write it
            if name in SHAPE_CHANGING_OPS:
                raise ValueError(f"scenario {k} edit {q}: {name} changes the tableau's shape; "
                                 f"call SensState.{name} on a single handle")
            flat.append(_pack_edit(name, args, f"scenario {k} edit {q}"))
    edits = np.array(flat, dtype=EDIT_DTYPE) if flat else np.zeros(0, dtype=EDIT_DTYPE)
    return PackedScripts(nedits, edits)


class PackedGrowScripts(NamedTuple):
    """The packed arrays of lpr_sens_batch_create_grow."""
    nedits: np.ndarray   # int32, per scenario
    edits: np.ndarray    # EDIT_DTYPE; an add edit holds its payload offset in a, its length in b
    payload: np.ndarray  # float64: the vectors of the add edits, in script order


def _vector(x, what: str) -> np.ndarray:
    try:
        v = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {x!r} is not a vector of numbers") from None
    if v.ndim != 1:
        raise ValueError(f"{what}: {x!r} is not a vector of numbers")
    return v


def pack_grow_scripts(scripts: Sequence[Sequence[tuple]]) -> PackedGrowScripts:
    """Scripts -> the packed arrays of lpr_sens_batch_create_grow.  Besides the five ops of
    pack_scripts, which pack exactly as there, a script may hold ``("add_activity", c_new, a_new)``
    and ``("add_constraint", tech, rhs)`` as SensState spells them; their vectors go into one
    payload pool in script order."""
    if len(scripts) < 1:
        raise ValueError("no scenarios")
    nedits = np.zeros(len(scripts), dtype=np.int32)
    flat, pool, at = [], [], 0
    for k, script in enumerate(scripts):
        nedits[k] = len(script)
        for q, edit in enumerate(script):
            where = f"scenario {k} edit {q}"
            name, args = edit[0], tuple(edit[1:])
            if len(args) == 1 and isinstance(args[0], (tuple, list)):
                args = tuple(args[0])    # (op, (args...)) as the test scripts write it
            if name not in SHAPE_CHANGING_OPS:
                flat.append(_pack_edit(name, args, where))
                continue
            if len(args) != 2:
                raise ValueError(f"{where}: {name} takes 2 arguments, got {len(args)}")
            if name == "add_activity":
                code, value, vec = N.LPR_SENS_EDIT_ADD_ACTIVITY, args[0], args[1]
            else:
                code, value, vec = N.LPR_SENS_EDIT_ADD_CONSTRAINT, args[1], args[0]
            vec = _vector(vec, where)
            try:
                value = float(value)
            except (TypeError, ValueError):
                raise ValueError(f"{where}: {value!r} is not a number") from None
            if at + vec.size > 2 ** 31 - 1:
                raise ValueError(f"{where}: the payload pool is past 2^31 - 1 doubles")
            flat.append((code, at, vec.size, 0, value))
            pool.append(vec)
            at += vec.size
    edits = np.array(flat, dtype=EDIT_DTYPE) if flat else np.zeros(0, dtype=EDIT_DTYPE)
    payload = np.concatenate(pool) if pool else np.zeros(0, dtype=np.float64)
    return PackedGrowScripts(nedits, edits, payload)


RANGING_COLUMN_FIELDS = ("kind", "var_row", "reduced_cost", "cost_lo", "cost_hi")
RANGING_ROW_FIELDS = ("shadow", "rhs_lo", "rhs_hi", "rhs_now")


def trim_ranging(padded: RangingReport, k: int, rows: int, cols: int) -> RangingReport:
    """Row k of the padded arrays of ``ranging_arrays()`` cut to a rows x cols scenario: the
    per-column fields keep cols - 1 entries, the per-constraint fields rows - 1.  What is cut off
    must be the padding fill (NO_BASIC_ENTRY / NaN) and nothing else."""
    out = {}
    for fields, keep in ((RANGING_COLUMN_FIELDS, cols - 1), (RANGING_ROW_FIELDS, rows - 1)):
        for f in fields:
            row = getattr(padded, f)[k]
            if keep < 0 or keep > row.shape[0]:
                raise ValueError(f"{f}: a {rows} x {cols} scenario does not fit a padded row of "
                                 f"{row.shape[0]}")
            tail = row[keep:]
            fill = (tail == NO_BASIC_ENTRY) if row.dtype == np.int32 else np.isnan(tail)
            if not fill.all():
                raise ValueError(f"{f}: scenario {k} has data past its own shape {rows} x {cols}")
            out[f] = row[:keep].copy()
    return RangingReport(**out)


class SensitivityBatch:
    """``len(scripts)`` scenarios over the state ``base`` holds now (lpr_sens_batch_*).  The base
    is only read and may be destroyed afterwards."""

    def __init__(self, base: SensState, scripts: Sequence[Sequence[tuple]], log_cap: int = 0):
        self._h = None
        p = self._pack(scripts)
        self._engine = base.engine
        self._attach(self._create(base, p, int(log_cap)), p)

    def _attach(self, h: C.c_void_p, p) -> None:
        self._h = h
        self.Count = len(p.nedits)
        self.nedits = p.nedits.tolist()
        self._off = np.concatenate([[0], np.cumsum(p.nedits)]).astype(np.int64)
        cnt, r, c, lc, f = (C.c_int32() for _ in range(5))
        te = C.c_int64()
        N.check(N.lib.lpr_sens_batch_info(self._h, C.byref(cnt), C.byref(r), C.byref(c),
                                          C.byref(te), C.byref(lc), C.byref(f)),
                "lpr_sens_batch_info")
        self.Rows, self.Cols, self.LogCap = r.value, c.value, lc.value
        self.TotalEdits = te.value
        self.LastResult: Optional[N.SensBatchResult] = None

    _pack = staticmethod(pack_scripts)

    @staticmethod
    def _create(base: SensState, p: PackedScripts, log_cap: int) -> C.c_void_p:
        h = C.c_void_p()
        eptr = p.edits.ctypes.data_as(C.POINTER(N.SensEdit)) if p.edits.size else None
        N.check(N.lib.lpr_sens_batch_create(base._h, len(p.nedits),
                                            p.nedits.ctypes.data_as(C.POINTER(C.c_int32)), eptr,
                                            log_cap, C.byref(h)), "lpr_sens_batch_create")
        return h

    def destroy(self) -> None:
        if self._h:
            N.lib.lpr_sens_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- every script, edit after edit ----------------------------------------------------------
    def Run(self, max_pivots: int = 0, chunk: int = 0, variant: int = 0) -> N.SensBatchResult:
        opts = N.SensBatchOpts(max_pivots=int(max_pivots), chunk=int(chunk), variant=int(variant))
        res = N.SensBatchResult()
        N.check(N.lib.lpr_sens_batch_run(self._h, C.byref(opts), C.byref(res)),
                "lpr_sens_batch_run")
        self.LastResult = res
        return res

    # -- bulk reads -----------------------------------------------------------------------------
    def outcome_arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        """(outcome, pivots) per edit, packed as the scripts are."""
        n = max(self.TotalEdits, 1)
        oc = np.full(n, EDIT_NOT_RUN, dtype=np.int32)
        pv = np.zeros(n, dtype=np.int64)
        N.check(N.lib.lpr_sens_batch_outcomes_read(
            self._h, oc.ctypes.data_as(C.POINTER(C.c_int32)),
            pv.ctypes.data_as(C.POINTER(C.c_int64))), "lpr_sens_batch_outcomes_read")
        return oc[:self.TotalEdits], pv[:self.TotalEdits]

    def state_arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(z, solutionVector.Count, basicVars as a Count x (rows - 1) array)"""
        m = self.Rows - 1
        z = np.zeros(self.Count, dtype=np.float64)
        ns = np.zeros(self.Count, dtype=np.int32)
        basic = np.zeros(max(self.Count * m, 1), dtype=np.int32)
        N.check(N.lib.lpr_sens_batch_state_read(
            self._h, z.ctypes.data_as(C.POINTER(C.c_double)),
            ns.ctypes.data_as(C.POINTER(C.c_int32)),
            basic.ctypes.data_as(C.POINTER(C.c_int32))), "lpr_sens_batch_state_read")
        return z, ns, basic[:self.Count * m].reshape(self.Count, m)

    def _shape_read(self) -> Tuple[np.ndarray, np.ndarray, int, int]:
        """(rows, cols) per scenario as of now and the batch-wide (max_rows, max_cols); in a
        fixed-shape batch every entry is the base's shape."""
        rows = np.zeros(self.Count, dtype=np.int32)
        cols = np.zeros(self.Count, dtype=np.int32)
        mr, mc = C.c_int32(), C.c_int32()
        N.check(N.lib.lpr_sens_batch_shape_read(
            self._h, rows.ctypes.data_as(C.POINTER(C.c_int32)),
            cols.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(mr), C.byref(mc)),
            "lpr_sens_batch_shape_read")
        return rows, cols, mr.value, mc.value

    def ranging_arrays(self) -> RangingReport:
        """The sensitivity report of every scenario from one device call (lpr_sens_batch_ranging):
        the nine arrays of ``SensState.ranging()``, scenario k in row k.  The per-column arrays are
        Count x (max_cols - 1), the per-constraint arrays Count x (max_rows - 1); entries past a
        scenario's own shape are NO_BASIC_ENTRY (int) or NaN (float)."""
        _, _, mr, mc = self._shape_read()
        # the call writes every cell, the padding included
        ints = [np.empty((self.Count, mc - 1), dtype=np.int32) for _ in range(2)]
        cols = [np.empty((self.Count, mc - 1), dtype=np.float64) for _ in range(3)]
        rows = [np.empty((self.Count, mr - 1), dtype=np.float64) for _ in range(4)]
        N.check(N.lib.lpr_sens_batch_ranging(
            self._h, *[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in ints],
            *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in cols + rows]),
            "lpr_sens_batch_ranging")
        return RangingReport(*ints, *cols, *rows)

    def Ranging(self, k: int) -> RangingReport:
        """Scenario k's report at its own shape, as ``SensState.ranging()`` returns one."""
        rows, cols, _, _ = self._shape_read()
        return trim_ranging(self.ranging_arrays(), int(k), int(rows[k]), int(cols[k]))

    def RangingTime(self) -> float:
        """Device milliseconds of the last ranging_arrays() / Ranging() call's kernel, from events."""
        ms = C.c_double()
        N.check(N.lib.lpr_sens_batch_ranging_time(self._h, C.byref(ms)),
                "lpr_sens_batch_ranging_time")
        return ms.value

    # -- per-scenario reads ---------------------------------------------------------------------
    def Outcomes(self, k: int) -> List[int]:
        oc, _ = self.outcome_arrays()
        return oc[self._off[k]:self._off[k + 1]].tolist()

    def Pivots(self, k: int) -> List[int]:
        _, pv = self.outcome_arrays()
        return pv[self._off[k]:self._off[k + 1]].tolist()

    def Tableau(self, k: int) -> np.ndarray:
        T = np.empty((self.Rows, self.Cols), dtype=np.float64)
        N.check(N.lib.lpr_sens_batch_tableau_read(
            self._h, int(k), T.ctypes.data_as(C.POINTER(C.c_double))),
            "lpr_sens_batch_tableau_read")
        return T

    def Solution(self, k: int) -> np.ndarray:
        cnt = C.c_int32()
        N.check(N.lib.lpr_sens_batch_solution_read(self._h, int(k), None, 0, C.byref(cnt)),
                "lpr_sens_batch_solution_read")
        cap = max(cnt.value, 1)
        x = np.zeros(cap, dtype=np.float64)
        N.check(N.lib.lpr_sens_batch_solution_read(
            self._h, int(k), x.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(cnt)),
            "lpr_sens_batch_solution_read")
        return x[:cnt.value]

    def Log(self, k: int, cap: Optional[int] = None) -> List[Tuple[int, int, int]]:
        """The pivot triples kept for scenario k (at most LogCap); LogCount gives the exact total."""
        cap = self.LogCap if cap is None else int(cap)
        buf = np.zeros(max(3 * cap, 3), dtype=np.int32)
        cnt = C.c_int64()
        N.check(N.lib.lpr_sens_batch_log_read(
            self._h, int(k), buf.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(cnt)),
            "lpr_sens_batch_log_read")
        n = min(cnt.value, cap, self.LogCap)
        return [tuple(t) for t in buf[:3 * n].reshape(-1, 3).tolist()]

    def LogCount(self, k: int) -> int:
        cnt = C.c_int64()
        N.check(N.lib.lpr_sens_batch_log_read(self._h, int(k), None, 0, C.byref(cnt)),
                "lpr_sens_batch_log_read")
        return cnt.value

    def State(self, k: int) -> dict:
        """Scenario k as ``OracleSens.state()`` lays a state out: T, basic, sol, z."""
        z, _, basic = self.state_arrays()
        return dict(T=self.Tableau(k), basic=basic[k].tolist(), sol=self.Solution(k),
                    z=float(z[k]))


class SensitivityGrowBatch(SensitivityBatch):
    """A ``SensitivityBatch`` whose scripts may also hold ``add_activity`` and ``add_constraint``
    (lpr_sens_batch_create_grow): a scenario's tableau grows as its script runs.  ``Rows`` and
    ``Cols`` stay the base's shape; ``Shape(k)`` is scenario k's own, ``MaxRows`` x ``MaxCols`` the
    largest any script can reach."""

    _pack = staticmethod(pack_grow_scripts)

    @staticmethod
    def _create(base: SensState, p: PackedGrowScripts, log_cap: int) -> C.c_void_p:
        h = C.c_void_p()
        eptr = p.edits.ctypes.data_as(C.POINTER(N.SensEdit)) if p.edits.size else None
        pptr = p.payload.ctypes.data_as(C.POINTER(C.c_double)) if p.payload.size else None
        N.check(N.lib.lpr_sens_batch_create_grow(
            base._h, len(p.nedits), p.nedits.ctypes.data_as(C.POINTER(C.c_int32)), eptr, pptr,
            p.payload.size, log_cap, C.byref(h)), "lpr_sens_batch_create_grow")
        return h

    def shape_arrays(self) -> Tuple[np.ndarray, np.ndarray, int, int]:
        """(rows, cols) per scenario as of now, and the batch-wide (max_rows, max_cols)."""
        rows = np.zeros(self.Count, dtype=np.int32)
        cols = np.zeros(self.Count, dtype=np.int32)
        mr, mc = C.c_int32(), C.c_int32()
        N.check(N.lib.lpr_sens_batch_shape_read(
            self._h, rows.ctypes.data_as(C.POINTER(C.c_int32)),
            cols.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(mr), C.byref(mc)),
            "lpr_sens_batch_shape_read")
        return rows, cols, mr.value, mc.value

    @property
    def MaxRows(self) -> int:
        return self.shape_arrays()[2]

    @property
    def MaxCols(self) -> int:
        return self.shape_arrays()[3]

    def Shape(self, k: int) -> Tuple[int, int]:
        rows, cols, _, _ = self.shape_arrays()
        return int(rows[k]), int(cols[k])

    def state_arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(z, solutionVector.Count, basicVars as a Count x (max_rows - 1) array whose entries
        past a scenario's own rows - 1 are NO_BASIC_ENTRY)"""
        m = self.MaxRows - 1
        z = np.zeros(self.Count, dtype=np.float64)
        ns = np.zeros(self.Count, dtype=np.int32)
        basic = np.zeros(max(self.Count * m, 1), dtype=np.int32)
        N.check(N.lib.lpr_sens_batch_state_read(
            self._h, z.ctypes.data_as(C.POINTER(C.c_double)),
            ns.ctypes.data_as(C.POINTER(C.c_int32)),
            basic.ctypes.data_as(C.POINTER(C.c_int32))), "lpr_sens_batch_state_read")
        return z, ns, basic[:self.Count * m].reshape(self.Count, m)

    def Tableau(self, k: int) -> np.ndarray:
        T = np.empty(self.Shape(k), dtype=np.float64)
        N.check(N.lib.lpr_sens_batch_tableau_read(
            self._h, int(k), T.ctypes.data_as(C.POINTER(C.c_double))),
            "lpr_sens_batch_tableau_read")
        return T

    def State(self, k: int) -> dict:
        st = super().State(k)
        st["basic"] = st["basic"][:self.Shape(k)[0] - 1]
        return st


def optimal_items(lp_batch) -> List[int]:
    """The indices of a solved ``PrimalSimplexBatch`` whose status is optimal: the LPs a
    ``SensitivityModelBatch`` can be built on."""
    st, _, _ = lp_batch.status_arrays()
    return [int(k) for k in np.flatnonzero(st == N.LPR_OK_OPTIMAL)]


class SensitivityModelBatch(SensitivityGrowBatch):
    """Many solved models, one script each (lpr_sens_batch_from_batch): scenario k is a fresh
    analyzer on LP ``items[k]`` of a solved ``PrimalSimplexBatch`` -- what Program.cs:147-151 builds
    from ``GetFinalTableau()``, ``SolutionVector``, ``FinalZ`` and ``BasicVariables`` -- followed by
    ``scripts[k]`` (``pack_grow_scripts`` form).  ``items`` may repeat an index and come in any
    order; None means LP k for scenario k.  Every item must be optimal (``optimal_items``).  The LP
    batch is only read and may be destroyed afterwards.  ``Rows`` x ``Cols`` is the largest base
    shape over the chosen LPs; ``Shape(k)`` is scenario k's own."""

    def __init__(self, lp_batch, scripts: Sequence[Sequence[tuple]],
                 items: Optional[Sequence[int]] = None, log_cap: int = 0):
        self._h = None
        p = pack_grow_scripts(scripts)
        count = len(p.nedits)
        if items is None:
            self._items = list(range(count))
            iptr = None
        else:
            self._items = [_int32(i, "items") for i in items]
            if len(self._items) != count:
                raise ValueError(f"{len(self._items)} items for {count} scripts")
            arr = np.asarray(self._items, dtype=np.int32)
            iptr = arr.ctypes.data_as(C.POINTER(C.c_int32))
        self._engine = lp_batch._engine
        h = C.c_void_p()
        eptr = p.edits.ctypes.data_as(C.POINTER(N.SensEdit)) if p.edits.size else None
        pptr = p.payload.ctypes.data_as(C.POINTER(C.c_double)) if p.payload.size else None
        N.check(N.lib.lpr_sens_batch_from_batch(
            lp_batch._h, count, iptr, p.nedits.ctypes.data_as(C.POINTER(C.c_int32)), eptr, pptr,
            p.payload.size, int(log_cap), C.byref(h)), "lpr_sens_batch_from_batch")
        self._attach(h, p)

    def Item(self, k: int) -> int:
        """The LP of the batch this one was built from that scenario k started on."""
        return self._items[k]

    def ConstructTime(self) -> float:
        """Device milliseconds of the constructor kernel of this batch, from events."""
        ms = C.c_double()
        N.check(N.lib.lpr_sens_batch_from_batch_time(self._h, C.byref(ms)),
                "lpr_sens_batch_from_batch_time")
        return ms.value
