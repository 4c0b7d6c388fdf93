"""Many independent ``RevisedPrimalSimplexSolver`` runs in one call (lpr_rev_batch_*, DESIGN.md
section 17).

Every LP of a batch is built and solved on the MI355X with the rules of
Simplex/RevisedPrimalSimplexSolver.cs, the same bits ``RevisedPrimalSimplexSolver`` gives for that
LP alone.  The reference has no batch mode: the members below are per-LP lists / accessors named
after the single-model mirror (revised_primal_simplex_solver.py).  A batch made with
``trace_cap > 0`` is traced: its solve also records every snapshot
``CaptureSnapshot`` would have appended, as numbers on the device, and ``IterationSnapshots(k)``
formats them with the single mirror's formatter; an untraced batch keeps none.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import numpy as np

from . import _native as N
from ._native import _ptr
from .engine import Engine, default_engine
from .revised_primal_simplex_solver import MESSAGES, SolverException, format_snapshot


class PackedRevisedModels(NamedTuple):
    """The packed arrays of lpr_rev_batch_create."""
    n: np.ndarray          # int32, per LP
    m: np.ndarray          # int32, per LP
    objective: np.ndarray  # float64, packed by n
    A: np.ndarray          # float64, m x n row-major blocks
    b: np.ndarray          # float64, packed by m
    is_min: np.ndarray     # int8, per LP


def pack_revised_models(models) -> PackedRevisedModels:
    """``(objective, constraints, isMinimization)`` triples -> the packed ABI arrays, with the
    constructor's checks (RevisedPrimalSimplexSolver.cs:43-44, :57-58) per model; the messages are
    the C#'s, prefixed by the model's index.  Relation is never read (:55-61)."""
    models = list(models)
    if not models:
        raise ValueError("no models")
    ns, ms, obj, A, b, mn = [], [], [], [], [], []
    for k, (objective, constraints, is_min) in enumerate(models):
        if objective is None or len(objective) == 0:  # :43
            raise ValueError(f"model {k}: Objective cannot be null or empty.")
        if constraints is None or len(constraints) == 0:  # :44
            raise ValueError(f"model {k}: Constraints cannot be null or empty.")
        n, m = len(objective), len(constraints)
        block = np.zeros((m, n), dtype=np.float64)
        rhs = np.zeros(m, dtype=np.float64)
        for i, c in enumerate(constraints):
            if len(c.Coefficients) != n:  # :57-58
                raise ValueError(f"model {k}: Constraint {i + 1} has incorrect number of "
                                 "coefficients.")
            block[i, :] = c.Coefficients
            rhs[i] = c.RHS
        ns.append(n)
        ms.append(m)
        obj.append(np.asarray(objective, dtype=np.float64).reshape(-1))
        A.append(block.reshape(-1))
        b.append(rhs)
        mn.append(1 if is_min else 0)
    return PackedRevisedModels(
        np.asarray(ns, dtype=np.int32), np.asarray(ms, dtype=np.int32), np.concatenate(obj),
        np.concatenate(A), np.concatenate(b), np.asarray(mn, dtype=np.int8))


# The form rule of rev_batch_common.hpp / batch_common.hpp, for tests and tuning: what an LP keeps
# resident in doubles, and the smallest form that holds it.
VEC_M = 6            # kRevBatchVecM
MAX_LDS_W = ((64 << 10) - (1 << 10)) // 4   # kBatchMaxLdsW
MAX_LDS_G = (160 << 10) - (1 << 10)         # kBatchMaxLdsG
MAX_M, MAX_NM = 1023, 2047                  # kRevBatchMaxM, kRevBatchMaxNM
FORM_W, FORM_G, FORM_H = 0, 1, 2
CHUNK = (256, 128, 16)                      # kRevBatchChunk


def footprint(m: int, n: int) -> int:
    """rev_batch_footprint: doubles of LDS one LP needs in forms W and G."""
    vectors = VEC_M * m + n + (n + m) + (m + 1) // 2 + (n + m + 7) // 8
    return m * (m | 1) + m * (n | 1) + vectors


def pick_form(m: int, n: int, variant: int = 0) -> int:
    """batch_pick_form on the footprint's bytes."""
    nbytes = 8 * footprint(m, n)
    fit_w, fit_g = nbytes <= MAX_LDS_W, nbytes <= MAX_LDS_G
    if variant == 1 and fit_w:
        return FORM_W
    if variant == 2 and fit_g:
        return FORM_G
    if variant == 3:
        return FORM_H
    return FORM_W if fit_w else (FORM_G if fit_g else FORM_H)


# One record of a traced batch (rev_trace_* of rev_batch_common.hpp), in doubles: six scalars,
# then the fields below in this order.
TRACE_SCALARS = ("entering", "leaving_row", "leaving_var", "rc_pre", "z_working", "z_original")
TRACE_FIELDS = ("y", "rcX", "rcS", "u_pre", "ratios_pre", "basis_pre", "basis_post", "xB",
                "BInvA", "BInv")


def trace_offsets(m: int, n: int) -> dict:
    """Field name -> (offset, length) in doubles inside one record."""
    sizes = dict(y=m, rcX=n, rcS=m, u_pre=m, ratios_pre=m, basis_pre=m, basis_post=m, xB=m,
                 BInvA=m * n, BInv=m * m)
    out, at = {}, len(TRACE_SCALARS)
    for name in TRACE_FIELDS:
        out[name] = (at, sizes[name])
        at += sizes[name]
    return out


def trace_stride(m: int, n: int) -> int:
    """rev_trace_stride: doubles of one record, 6 + 7 m + n + m n + m m."""
    at, ln = trace_offsets(m, n)["BInv"]
    return at + ln


def trace_record(r: np.ndarray, m: int, n: int) -> dict:
    """One record as the dict ``oracle.revised_trace`` gives for a snapshot."""
    d = dict(entering=int(r[0]), leaving_row=int(r[1]), leaving_var=int(r[2]), rc_pre=r[3],
             z_working=r[4], z_original=r[5])
    for name, (at, ln) in trace_offsets(m, n).items():
        d[name] = r[at:at + ln].copy()
    d["BInvA"] = d["BInvA"].reshape(m, n)
    d["BInv"] = d["BInv"].reshape(m, m)
    d["basis_pre"] = d["basis_pre"].astype(np.int32)
    d["basis_post"] = d["basis_post"].astype(np.int32)
    return d


class RevisedSimplexBatch:
    """``count`` RevisedPrimalSimplexSolver models in one device handle.

    ``Status[k]``, ``FinalZ[k]`` and ``SolutionVector[k]`` follow the single mirror: FinalZ and
    the vector are set only on the optimal exit (0.0 and [] otherwise).  ``Iterations[k]`` is the
    C#'s ``iteration``.  ``Raise(k)`` raises what the single mirror's Solve() raises."""

    def __init__(self, models, engine: Optional[Engine] = None, log_cap: int = 0,
                 trace_cap: int = 0):
        models = list(models)
        p = pack_revised_models(models)
        self._engine = engine or default_engine()
        self._h = None
        h = C.c_void_p()
        N.check(N.lib.lpr_rev_batch_create(
            self._engine._h, len(p.n), _ptr(p.n, C.c_int32), _ptr(p.m, C.c_int32),
            _ptr(p.objective, C.c_double), _ptr(p.A, C.c_double), _ptr(p.b, C.c_double),
            _ptr(p.is_min, C.c_int8), int(log_cap), C.byref(h)), "lpr_rev_batch_create")
        self._h = h
        self._shapes = [(int(n), int(m)) for n, m in zip(p.n, p.m)]
        # triples kept per LP (include/lpr_engine.h: 0 means 4 * (n + 2 m), at most 4096)
        self._log_caps = [int(log_cap) if log_cap > 0 else min(4096, 4 * (n + 2 * m))
                          for n, m in self._shapes]
        self._x_at = np.concatenate([[0], np.cumsum([s[0] for s in self._shapes])])
        self._b_at = np.concatenate([[0], np.cumsum([s[1] for s in self._shapes])])
        self._basis = None
        self.Count = len(self._shapes)
        self.Status: List[Optional[int]] = [None] * self.Count
        self.FinalZ: List[float] = [0.0] * self.Count
        self.SolutionVector: List[List[float]] = [[] for _ in range(self.Count)]
        self.Iterations: List[int] = [0] * self.Count
        self.LastResult: Optional[N.RevBatchResult] = None
        self._is_min = [bool(v) for v in p.is_min]
        self.TraceCap = 0  # records kept per LP; 0: untraced
        if trace_cap:
            self.trace_reserve(trace_cap)

    def trace_reserve(self, trace_cap: int) -> None:
        """Make the batch traced (lpr_rev_batch_trace_reserve): only before the first Solve."""
        N.check(N.lib.lpr_rev_batch_trace_reserve(self._h, int(trace_cap)),
                "lpr_rev_batch_trace_reserve")
        self.TraceCap = int(trace_cap)

    def destroy(self) -> None:
        if self._h:
            N.lib.lpr_rev_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- Solve :82-251, per LP -------------------------------------------------------------
    def Solve(self, max_pivots: int = 0, chunk: int = 0, variant: int = 0) -> N.RevBatchResult:
        opts = N.RevBatchOpts(max_pivots=int(max_pivots), chunk=int(chunk), variant=int(variant))
        res = N.RevBatchResult()
        N.check(N.lib.lpr_rev_batch_solve(self._h, C.byref(opts), C.byref(res)),
                "lpr_rev_batch_solve")
        self.LastResult = res
        self._basis = None
        st, it, z = self.status_arrays()
        x = self.solution_packed()
        for k in range(self.Count):
            self.Status[k] = int(st[k])
            self.Iterations[k] = int(it[k])
            if st[k] == N.LPR_OK_OPTIMAL:  # :124-146
                self.FinalZ[k] = float(z[k])
                self.SolutionVector[k] = [float(v) for v in x[self._x_at[k]:self._x_at[k + 1]]]
        return res

    def Raise(self, k: int) -> None:
        """The exception ``RevisedPrimalSimplexSolver.Solve()`` throws for LP k's status (:91,
        :179, :183, :267); nothing for an optimal LP or one at the pivot limit."""
        if self.Status[k] in MESSAGES:
            raise SolverException(self.Status[k])

    # -- bulk reads ------------------------------------------------------------------------
    def status_arrays(self):
        """(status int32[count], iterations int64[count], FinalZ float64[count])."""
        st = np.zeros(self.Count, dtype=np.int32)
        it = np.zeros(self.Count, dtype=np.int64)
        z = np.zeros(self.Count, dtype=np.float64)
        N.check(N.lib.lpr_rev_batch_status_read(self._h, _ptr(st, C.c_int32),
                                                _ptr(it, C.c_int64), _ptr(z, C.c_double)),
                "lpr_rev_batch_status_read")
        return st, it, z

    def solution_packed(self) -> np.ndarray:
        x = np.zeros(int(self._x_at[-1]), dtype=np.float64)
        N.check(N.lib.lpr_rev_batch_solution_read(self._h, _ptr(x, C.c_double)),
                "lpr_rev_batch_solution_read")
        return x

    def basis_packed(self) -> np.ndarray:
        b = np.zeros(int(self._b_at[-1]), dtype=np.int32)
        N.check(N.lib.lpr_rev_batch_basis_read(self._h, _ptr(b, C.c_int32)),
                "lpr_rev_batch_basis_read")
        return b

    # -- per-LP reads ----------------------------------------------------------------------
    def Shape(self, k: int):
        """(n, m) of LP k."""
        return self._shapes[k]

    def BasicVariables(self, k: int) -> List[int]:  # :39
        if self._basis is None:  # one packed read per solve
            self._basis = self.basis_packed()
        return [int(v) for v in self._basis[self._b_at[k]:self._b_at[k + 1]]]

    def PivotLog(self, k: int, cap: Optional[int] = None) -> np.ndarray:
        """(leavingRow 0-based, entering variable, leaving variable) of every iteration kept."""
        if cap is None:
            cap = self._log_caps[k]
        row = np.zeros(max(cap, 1), dtype=np.int32)
        enter = np.zeros(max(cap, 1), dtype=np.int32)
        leave = np.zeros(max(cap, 1), dtype=np.int32)
        cnt = C.c_int64()
        N.check(N.lib.lpr_rev_batch_log_read(self._h, int(k), _ptr(row, C.c_int32),
                                             _ptr(enter, C.c_int32), _ptr(leave, C.c_int32),
                                             int(cap), C.byref(cnt)), "lpr_rev_batch_log_read")
        c = min(cnt.value, cap)
        return np.stack([row[:c], enter[:c], leave[:c]], axis=1)

    def BInverse(self, k: int) -> np.ndarray:
        m = self._shapes[k][1]
        out = np.empty((m, m), dtype=np.float64)
        N.check(N.lib.lpr_rev_batch_binv_read(self._h, int(k), _ptr(out, C.c_double)),
                "lpr_rev_batch_binv_read")
        return out

    def XB(self, k: int) -> np.ndarray:
        out = np.empty(self._shapes[k][1], dtype=np.float64)
        N.check(N.lib.lpr_rev_batch_xb_read(self._h, int(k), _ptr(out, C.c_double)),
                "lpr_rev_batch_xb_read")
        return out

    # -- the trace --------------------------------------------------
    def trace_info(self):
        """(snapshots, offset, stride), int64[count] each: the exact number of records of every
        LP (min(snapshots, TraceCap) are kept), where its records start in the trace slab and the
        doubles of one record."""
        snaps = np.zeros(self.Count, dtype=np.int64)
        off = np.zeros(self.Count, dtype=np.int64)
        stride = np.zeros(self.Count, dtype=np.int64)
        N.check(N.lib.lpr_rev_batch_trace_info(self._h, _ptr(snaps, C.c_int64),
                                               _ptr(off, C.c_int64), _ptr(stride, C.c_int64)),
                "lpr_rev_batch_trace_info")
        return snaps, off, stride

    def trace_packed(self):
        """(slab, snapshots, offset, stride): every LP's records in one copy."""
        snaps, off, stride = self.trace_info()
        slab = np.zeros(int(self.TraceCap * stride.sum()), dtype=np.float64)
        N.check(N.lib.lpr_rev_batch_trace_read_all(self._h, _ptr(slab, C.c_double), slab.size),
                "lpr_rev_batch_trace_read_all")
        return slab, snaps, off, stride

    def trace_read(self, k: int, first: int, n: int) -> np.ndarray:
        """Records [first, first + n) of LP k, one per row."""
        nv, m = self._shapes[k]
        out = np.zeros((max(int(n), 0), trace_stride(m, nv)), dtype=np.float64)
        N.check(N.lib.lpr_rev_batch_trace_read(self._h, int(k), int(first), int(n),
                                               _ptr(out, C.c_double)),
                "lpr_rev_batch_trace_read")
        return out

    def SnapshotCount(self, k: int) -> int:
        """Snapshots the C# list of LP k would hold (may exceed TraceCap)."""
        return int(self.trace_info()[0][k])

    def Snapshot(self, k: int, i: int) -> dict:
        """Snapshot i of LP k as numbers, with the keys of one ``CaptureSnapshot`` call: entering,
        leaving_row, leaving_var, rc_pre, z_working, z_original, y, rcX, rcS, u_pre, ratios_pre,
        basis_pre, basis_post, xB, BInvA, BInv."""
        nv, m = self._shapes[k]
        return trace_record(self.trace_read(k, i, 1)[0], m, nv)

    def IterationSnapshots(self, k: int) -> List[str]:  # :35, filled by CaptureSnapshot :294-387
        """The C#'s list of text blocks for LP k: "Iteration i" per pivot and "Optimal"; past
        TraceCap it stops after the kept prefix."""
        nv, m = self._shapes[k]
        count = self.SnapshotCount(k)
        recs = self.trace_read(k, 0, min(count, self.TraceCap))
        out = []
        for i, r in enumerate(recs):
            snap = trace_record(r, m, nv)
            title = "Optimal" if snap["entering"] < 0 else f"Iteration {i + 1}"
            out.append(format_snapshot(title, nv, m, self._is_min[k], snap))
        return out
