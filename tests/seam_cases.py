"""Constructed seam items for the primal, revised and B&B batches (TEST ONLY; DESIGN.md sections
12, 13 and 17).  Every selection of those bodies is a per-lane scan over a strided walk, a combine
across the lanes of a wave (quad, half-row, row, bcast15, bcast31) and a combine across the waves
of a workgroup -- or, in the revised body, a sequential replay in windows of 64 that carries
`best` / `brow` from window to window.  The C# takes the FIRST candidate that wins, so a kernel
that is wrong on one seam is right on all data but the data that ties exactly across that seam.
Each item here plants such a tie (or EPS band) and declares it:

    engine      "primal" | "revised" | "bb"
    kind        the selection (KINDS)
    seam        the seam class (SEAMS)
    form, nt    the form its shape lands in under the project's form rule, and that form's NT
    at          where the plant is live: the iteration (primal, revised); for B&B the record id
                of the child whose first pivot of phase `phase` it is (bv, pivot_row: record 1)
    planted     the tied indices as the log reports them (rows of the primal batch are 1-based)
    lane0       index - lane0 is the position in the walk (lane = position % nt)
    winner      the index that must be selected
    mutants     the wrong selectors below that pick another index on this item
    equal       "bits" (the planted values are the same double), "value" (+0.0 / -0.0), "band"
                (all within 3 EPS of the winner's value, revised folds only) or "takes" (the fold
                takes every planted index in turn)

The shapes come from the form rules themselves: batch_trace_cases.W_MAX / G_MAX for the primal
batch, revised_batch.footprint / pick_form, and the B&B footprint 8 (2 r c + r) against
kBatchMaxLdsW / kBatchMaxLdsG.  test_batch_seams_cpu.py checks every declaration against the
Python restatements and the C oracle; test_batch_seams_gpu.py runs the items on the device.

Form W of the revised batch cannot hold m >= 64 (footprint(64, 1) is above kBatchMaxLdsW / 8
doubles), so the ratio fold's window seam exists in forms G and H only."""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np

import batch_trace_cases as btc
from ref_py import DBL_MAX, REV_EPS

FORM_NAME = ("W", "G", "H")
NT_OF_FORM = (64, 256, 256)
SEAMS = ("dpp", "wave", "stride", "partial", "window", "lane63")
KINDS = dict(primal=("entering", "leaving", "leaving_dblmax"),
             revised=("enter_fold", "ratio_fold"),
             bb=("bv", "dual_row", "dual_theta", "dual_first0", "primal_col", "primal_row",
                 "primal_first0", "pivot_row"))
DPP_PAIRS = ((1, 2), (3, 4), (7, 8), (15, 16), (31, 32))  # quad, half-row, row, bcast15, bcast31
STRIDE_T = 3  # the lane of the stride plants


# ------------------------------------------------------------------------------ seam pairs
def seam_pairs(nt: int, count: int, last: Optional[int] = None, reduced: bool = False):
    """[(seam class, label, walk positions ascending)] for a walk of `count` positions with stride
    nt; the first position must win.  DPP pairs cycle through the waves of the group; the stride
    plant is (t, t - 1 + nt, t + nt): the winner's own lane holds a tie one round later and the
    lane below it holds one too; the partial plant ends at `last` (default count - 1), the last
    position of a round that is not full, and starts one lane above it in the round before.
    reduced: the subset the H items use (both broadcasts, one wave seam, stride, partial)."""
    waves = nt // 64
    last = count - 1 if last is None else last
    assert count % nt != 0 and last >= nt + STRIDE_T and last // nt == (count - 1) // nt
    out = []
    for q, (lo, hi) in enumerate(DPP_PAIRS):
        if reduced and lo < 15:
            continue
        base = 64 * (q % waves)
        out.append(("dpp", f"lanes {base + lo}|{base + hi}", (base + lo, base + hi)))
    for w in range(1, waves):
        if reduced and w > 1:
            continue
        out.append(("wave", f"waves {64 * w - 1}|{64 * w}", (64 * w - 1, 64 * w)))
    t = STRIDE_T
    out.append(("stride", f"stride {t}|{t + nt}, decoy {t - 1 + nt}", (t, t - 1 + nt, t + nt)))
    out.append(("partial", f"last round {last - nt + 1}|{last}", (last - nt + 1, last)))
    return out


def mutants_of_seam(seam: str):
    return ("last_wins", "lane_major") if seam in ("stride", "partial") else ("last_wins",)


def free_index(taken, start=5):
    """The first index from `start` on that no plant uses."""
    k = start
    while k in taken:
        k += 1
    return k


# ------------------------------------------------------------------------------ selectors
# A view is what a selection sees: view.vals maps candidate index -> value (smaller wins), view.nt
# and view.lane0 give the walk.  The revised folds see view.seq (a list over the walk, None: not a
# candidate; the entering fold's values are -rc) and, for the ratio fold, view.basic.
def first_min(view) -> int:
    """The C#'s strict `<` scan: the minimum at its lowest index (-1: none)."""
    best, at = None, -1
    for i in sorted(view.vals):
        if best is None or view.vals[i] < best:
            best, at = view.vals[i], i
    return at


def enter_fold(seq, lo=0, hi=None, best=math.inf):
    """RevisedPrimalSimplexSolver.cs:105-121 on v = -rc: take when v < best - EPS."""
    cur = -1
    for i in range(lo, len(seq) if hi is None else hi):
        if seq[i] is not None and seq[i] < best - REV_EPS:
            best, cur = seq[i], i
    return cur, best


def ratio_fold(seq, basic, lo=0, hi=None, best=DBL_MAX, row=-1, clause=lambda i, row: True):
    """:154-176: ratio < best - EPS, or within EPS of best and (none yet or a lower basic index).
    clause(i, row): may the tie clause compare basic[i] with basic[row]?"""
    for i in range(lo, len(seq) if hi is None else hi):
        r = seq[i]
        if r is None:
            continue
        if r < best - REV_EPS or (abs(r - best) <= REV_EPS and
                                  (row == -1 or (clause(i, row) and basic[i] < basic[row]))):
            best, row = r, i
    return row, best


def select(view) -> int:
    """The right selection of a view."""
    if view.rule == "enter_fold":
        return enter_fold(view.seq)[0]
    if view.rule == "ratio_fold":
        return ratio_fold(view.seq, view.basic)[0]
    return first_min(view)


def _seq_vals(view) -> Dict[int, float]:
    return view.vals if view.rule == "first_min" else \
        {i: v for i, v in enumerate(view.seq) if v is not None}


# ---- the mutants: deliberately wrong selectors, each the defect of a plausible kernel ----------
def last_wins(view) -> int:
    """Ties go to the highest index."""
    vals = _seq_vals(view)
    m = min(vals.values())
    return max(i for i, v in vals.items() if v == m)


def lane_major(view) -> int:
    """Ties go to the lowest lane, then the lowest round: a reduction that never compares indices."""
    vals = _seq_vals(view)
    m = min(vals.values())
    return min((i for i, v in vals.items() if v == m),
               key=lambda i: ((i - view.lane0) % view.nt, (i - view.lane0) // view.nt))


def window_restart(view) -> int:
    """The revised folds restarted at every window of 64, the windows combined by plain minimum."""
    best, at = None, -1
    for b0 in range(0, len(view.seq), 64):
        if view.rule == "enter_fold":
            i, v = enter_fold(view.seq, b0, min(b0 + 64, len(view.seq)))
        else:
            i, v = ratio_fold(view.seq, view.basic, b0, min(b0 + 64, len(view.seq)))
        if i >= 0 and (best is None or v < best):
            best, at = v, i
    return at


def plain_argmin(view) -> int:
    """The revised folds without the EPS band: the minimum at its lowest index."""
    return first_min(SimpleNamespace(vals=_seq_vals(view)))


def tie_clause_in_window_only(view) -> int:
    """The ratio fold's tie clause compares basic[] only with a row taken in the same window."""
    return ratio_fold(view.seq, view.basic, clause=lambda i, row: i // 64 == row // 64)[0]


def lane63_stops(view) -> int:
    """A take at lane 63 of a window ends the fold: the `alive` mask of that take is carried into
    the next window instead of being reset."""
    best = math.inf if view.rule == "enter_fold" else DBL_MAX
    row = -1
    for b0 in range(0, len(view.seq), 64):
        hi = min(b0 + 64, len(view.seq))
        if view.rule == "enter_fold":
            i, v = enter_fold(view.seq, b0, hi, best)
            if i >= 0:
                row, best = i, v
        else:
            row, best = ratio_fold(view.seq, view.basic, b0, hi, best, row)
        if row == b0 + 63:
            break
    return row


MUTANTS = dict(last_wins=last_wins, lane_major=lane_major, window_restart=window_restart,
               plain_argmin=plain_argmin, tie_clause_in_window_only=tie_clause_in_window_only,
               lane63_stops=lane63_stops)


def _item(**kw):
    kw.setdefault("equal", "bits")
    kw.setdefault("lane0", 0)
    kw.setdefault("phase", None)
    kw["nt"] = NT_OF_FORM[kw["form"]]
    kw["name"] = "{engine}_{kind}_{f}_{seam}_{w}{t}".format(
        f=FORM_NAME[kw["form"]], w="_".join(str(p) for p in kw["planted"]),
        t=kw.pop("tag", ""), **kw)
    return SimpleNamespace(**kw)


# ============================================================================== primal batch
PRIMAL_PIVOTS = 2  # max_pivots of every primal item: the plant is at iteration 0


def primal_form(rows: int, cols: int) -> int:
    assert rows <= 1024 and cols <= 2048
    return btc.form_of(rows, cols)


def primal_shapes(kind: str):
    """(form, rows, cols) per form, from the form rule: the walk of `kind` (columns for entering,
    rows for leaving) is as long as the form's footprint allows next to a short other side."""
    if kind == "entering":  # W: 13 rows, G: 30 rows, H: the G width with twice the rows
        w = (13, btc.W_MAX // 13 - 1)
        g = (30, btc.G_MAX // 30 - 1)
        h = (60, g[1])
    else:  # W: 13 columns, G: 38 columns, H: the G height with more columns
        w = (btc.W_MAX // 14, 13)
        g = (btc.G_MAX // 39, 38)
        h = (g[0], 60)
    return [(0,) + w, (1,) + g, (2,) + h]


def _primal_body(rows, cols):
    """Small positive integers everywhere below the Z row, a positive RHS: bounded, and no entry
    of a column is <= 1e-9."""
    i = np.arange(rows).reshape(-1, 1)
    j = np.arange(cols).reshape(1, -1)
    T = 1.0 + ((7 * i + 3 * j) % 3)
    T[:, -1] = 40.0 + (np.arange(rows) % 5)
    return T


def primal_entering_item(form, rows, cols, seam, label, pos):
    """The most negative Z entry (-2) at every planted column, -1 at every other."""
    T = _primal_body(rows, cols)
    T[0, :-1] = -1.0
    T[0, -1] = 0.0
    T[0, list(pos)] = -2.0
    return _item(engine="primal", kind="entering", seam=seam, label=label, form=form, at=0,
                 planted=tuple(pos), winner=pos[0], mutants=mutants_of_seam(seam),
                 T=T, basis=cols + np.arange(rows - 1, dtype=np.int32))


def _primal_leaving_base(rows, cols):
    """Column 2 enters (Z = -5, every other Z entry -1); its entries are 1 and the RHS 40..44."""
    T = _primal_body(rows, cols)
    T[0, :-1] = -1.0
    T[0, 2] = -5.0
    T[0, -1] = 0.0
    T[1:, 2] = 1.0
    return T


def primal_leaving_item(form, rows, cols, seam, label, pos, zero_pair=False):
    """The minimum ratio 4 = 4/1 = 8/2 = 16/4 at every planted row (1-based: lane + 1); with
    zero_pair the ratios are +0.0 and -0.0 (b = -0.0): both pass `ratio >= 0`, `<` keeps the
    first."""
    T = _primal_leaving_base(rows, cols)
    planted = tuple(p + 1 for p in pos)
    for q, r in enumerate(planted):
        T[r, 2] = float(1 << q)
        T[r, -1] = 4.0 * (1 << q)
        if zero_pair:
            T[r, -1] = 0.0 if q == 0 else -0.0
    return _item(engine="primal", kind="leaving", seam=seam, label=label, form=form, at=0, lane0=1,
                 planted=planted, winner=planted[0], mutants=mutants_of_seam(seam),
                 equal="value" if zero_pair else "bits", tag="_zeros" if zero_pair else "",
                 T=T, basis=cols + np.arange(rows - 1, dtype=np.int32))


def primal_dblmax_item(form, rows, cols, pos):
    """The only candidate of the lanes up to pos[0] has ratio exactly DBL_MAX, which the C#'s
    `ratio < minRatio` refuses and the kernel uses as its start value; the row just across the
    seam holds the real minimum.  No tie: no mutant of the list is aimed at it."""
    T = _primal_leaving_base(rows, cols)
    lo, hi = pos[0] + 1, pos[1] + 1
    T[1:lo, 2] = 0.0
    T[lo, -1] = DBL_MAX
    T[hi, -1] = 4.0
    it = _item(engine="primal", kind="leaving_dblmax", seam="wave" if pos[1] % 64 == 0 else "dpp",
               label=f"DBL_MAX below {pos[0]}|{pos[1]}", form=form, at=0, lane0=1,
               planted=(hi,), winner=hi, mutants=(), dblmax_row=lo,
               T=T, basis=cols + np.arange(rows - 1, dtype=np.int32))
    return it


def primal_items() -> List[SimpleNamespace]:
    out = []
    for form, rows, cols in primal_shapes("entering"):
        assert primal_form(rows, cols) == form
        for seam, label, pos in seam_pairs(NT_OF_FORM[form], cols - 1, reduced=form == 2):
            out.append(primal_entering_item(form, rows, cols, seam, label, pos))
    for form, rows, cols in primal_shapes("leaving"):
        assert primal_form(rows, cols) == form
        nt = NT_OF_FORM[form]
        for seam, label, pos in seam_pairs(nt, rows - 1, reduced=form == 2):
            out.append(primal_leaving_item(form, rows, cols, seam, label, pos))
        zp = (31, 32) if nt == 64 else (63, 64)
        out.append(primal_leaving_item(form, rows, cols, "dpp" if nt == 64 else "wave",
                                       f"+0.0|-0.0 at {zp[0]}|{zp[1]}", zp, zero_pair=True))
        out.append(primal_dblmax_item(form, rows, cols, zp))
    return out


def py_primal(T):
    """ref_py.PyPrimal on a ready tableau."""
    from ref_py import PyPrimal
    p = PyPrimal.__new__(PyPrimal)
    p.t = [[float(v) for v in row] for row in np.asarray(T)]
    p.n = max(0, T.shape[1] - T.shape[0])
    p.m = T.shape[0] - 1
    p.basic = [0] * p.m
    p.log = []
    p.status = None
    p.FinalZ = 0.0
    p.SolutionVector = None
    return p


def primal_view(item):
    """The candidates of the planted selection, from ref_py.PyPrimal stepped to item.at."""
    p = py_primal(item.T)
    for _ in range(item.at):
        e = p.find_entering()
        p.pivot(p.find_leaving(e), e)
    t = p.t
    if item.kind == "entering":
        vals = {j: v for j, v in enumerate(t[0][:-1]) if v < 0}
    else:
        e = p.find_entering()
        vals = {}
        for i in range(1, len(t)):
            if t[i][e] > 1e-9:
                ratio = t[i][-1] / t[i][e]
                if 0 <= ratio < DBL_MAX:
                    vals[i] = ratio
    return SimpleNamespace(rule="first_min", vals=vals, nt=item.nt, lane0=item.lane0)


# ============================================================================== revised batch
REV_CAP = 5  # max_pivots of every revised item: the latest plant is at iteration 2


def rev_model(c, A, b):
    from revised_batch_cases import to_model
    return to_model(c, A, b)


def rev_form(m, n):
    from lpr_381_group_v22_amd import revised_batch as rb
    return rb.pick_form(m, n)


def rev_enter_shapes(n):
    """(form, m, n): n structural columns, m the smallest row count (from 3) of each form under
    revised_batch.pick_form."""
    out = []
    m = 3
    assert rev_form(m, n) == 0
    out.append((0, m, n))
    while rev_form(m, n) != 1:
        m += 1
    out.append((1, m, n))
    while rev_form(m, n) != 2:
        m += 1
    out.append((2, m, n))
    return out


def _rev_enter_model(m, n, c):
    """Every column of A is ones, b = 10 + i % 3: whichever column enters, the ratio test is a
    plain one; at iteration 0 rc = c."""
    return rev_model(c, np.ones((m, n)), [10.0 + (i % 3) for i in range(m)])


def rev_enter_items():
    out = []
    # 134 structural columns: windows 0..2 of the fold at iteration 0, when rc = c
    for form, m, n in rev_enter_shapes(134):
        def item(seam, label, planted, winner, mutants, c, equal="bits", at=0, model=None, m=m,
                 n=n):
            assert rev_form(m, n) == form
            return _item(engine="revised", kind="enter_fold", seam=seam, label=label, form=form,
                         at=at, planted=planted, winner=winner, mutants=mutants, equal=equal,
                         m=m, n=n, model=model or _rev_enter_model(m, n, c))
        for lo in (63, 127):  # exact ties on a window seam
            c = [1.0 + (j % 3) for j in range(n)]
            c[lo] = c[lo + 1] = 5.0
            out.append(item("window", f"tie {lo}|{lo + 1}", (lo, lo + 1), lo, ("last_wins",), c))
        # the staircase: 60 is taken (5), 62..64 stay inside its band, 65 leaves it and is taken,
        # 66 stays inside 65's band.  A fold restarted at 64 takes 64 and then 66; arg-max is 66.
        c = [1.0 + (j % 3) for j in range(n)]
        for j, d in ((60, 0.0), (62, 0.6e-9), (63, 0.9e-9), (64, 0.95e-9), (65, 1.5e-9),
                     (66, 2.2e-9)):
            c[j] = 5.0 + d
        out.append(item("window", "EPS staircase 62..66", (60, 62, 63, 64, 65, 66), 65,
                        ("window_restart", "plain_argmin", "last_wins"), c, equal="band"))
        # a take at lane 63, then one at lane 0 of the next window
        c = [1.0 + (j % 3) for j in range(n)]
        c[63], c[64] = 5.0, 7.0
        out.append(item("lane63", "take at 63, then at 64", (63, 64), 64, ("lane63_stops",), c,
                        equal="takes"))
    # n = 128: the last structural column is lane 63 of window 1 and the first slack lane 0 of
    # window 2, so the band below straddles the window seam too
    for form, m, n in rev_enter_shapes(128):
        # the band across the last structural column and the first slack, live at iteration 2:
        # x0 enters and row 0 leaves, x1 enters and row 1 leaves, then y = (-16, 6, 0, ...), so
        # slack n has rc = 16 and column n - 1 has rc = 6 - 5e-10 + 16 - 6: inside the band.
        A = np.zeros((m, n))
        A[0, :] = 1.0
        A[1, :] = 2.0
        A[0, 1], A[1, 0], A[1, 1], A[1, n - 1] = 0.125, 4.0, 1.0, 1.0
        A[2:, 2:] = 1.0
        c = [1.0 + (j % 3) for j in range(n)]
        c[0], c[1], c[n - 1] = 8.0, 4.0, 6.0 - 0.5e-9
        b = [1.0, 6.0] + [50.0] * (m - 2)
        assert (n - 1) % 64 == 63 and rev_form(m, n) == form
        out.append(_item(engine="revised", kind="enter_fold", seam="window", form=form, at=2,
                         label=f"band across structural|slack {n - 1}|{n}", planted=(n - 1, n),
                         winner=n - 1, mutants=("plain_argmin", "last_wins"), equal="band",
                         tag="_slack", m=m, n=n, model=rev_model(c, A, b)))
    return out


def rev_ratio_shapes():
    """(form, m, n) with m >= 130 rows (three windows of the ratio fold) and n = 4."""
    n, m = 4, 134
    assert rev_form(m, n) == 1
    out = [(1, m, n)]
    while rev_form(m, n) != 2:
        m += 1
    out.append((2, m, n))
    return out


def rev_ratio_items():
    out = []
    for form, m, n in rev_ratio_shapes():
        def item(seam, label, planted, winner, mutants, b=None, equal="bits", at=0, model=None):
            if model is None:  # column 0 enters (c = 8), its entries are 1: ratio_i = b_i
                A = np.ones((m, n))
                model = rev_model([8.0, 1.0, 2.0, 3.0], A, b)
            return _item(engine="revised", kind="ratio_fold", seam=seam, label=label, form=form,
                         at=at, planted=planted, winner=winner, mutants=mutants, equal=equal,
                         m=m, n=n, model=model)
        base = [100.0 + (i % 7) for i in range(m)]
        # the staircase of the entering fold, mirrored
        b = list(base)
        for i, d in ((62, 0.0), (63, 0.9e-9), (64, 0.95e-9), (65, 1.5e-9), (66, 2.2e-9)):
            b[i] = 5.0 - d
        out.append(item("window", "EPS staircase 62..66", (62, 63, 64, 65, 66), 65,
                        ("window_restart", "plain_argmin", "last_wins"), b, equal="band"))
        b = list(base)
        b[63] = b[64] = 5.0
        out.append(item("window", "tie 63|64", (63, 64), 63, ("last_wins",), b))
        b = list(base)
        b[63], b[64] = 5.0, 3.0
        out.append(item("lane63", "take at 63, then at 64", (63, 64), 64, ("lane63_stops",), b,
                        equal="takes"))
        # the tie clause across a window seam: x0 enters into row 70 (second window); then x1
        # enters, row 10 (basic n + 10) is taken with ratio 4 - 5e-10 and row 70 (basic 0) ties
        # within EPS: the clause must replace row 10, with the brow carried from window 0.
        A = np.zeros((m, n))
        A[70, :] = 1.0
        A[70, 1] = 0.25
        A[10, 1] = 1.0
        A[90, 1] = 1.0
        b = [50.0] * m
        b[70], b[10] = 1.0, 4.0 - 0.5e-9
        out.append(item("window", "tie clause across rows 10|70", (10, 70), 70,
                        ("tie_clause_in_window_only", "plain_argmin", "window_restart"),
                        equal="band", at=1, model=rev_model([8.0, 4.0, 1.0, 2.0], A, b)))
    return out


def revised_items():
    return rev_enter_items() + rev_ratio_items()


def revised_probe(item):
    """The instrumented fold (revised_batch_cases.tie_stats) stepped through item.at."""
    from revised_batch_cases import tie_stats
    probe = []
    tie_stats(item.model, max_iter=item.at + 1, probe=probe)
    assert len(probe) > item.at, (item.name, len(probe))
    return probe[item.at]


def revised_view(item):
    p = revised_probe(item)
    if item.kind == "enter_fold":
        seq = [None if v is None else -v for v in p["rc"]]
        return SimpleNamespace(rule="enter_fold", seq=seq, nt=item.nt, lane0=0, basic=None)
    return SimpleNamespace(rule="ratio_fold", seq=p["ratios"], nt=item.nt, lane0=0,
                           basic=p["basic"])


def fold_edge_distance(view) -> float:
    """The smallest distance of a candidate from an edge of the band it is compared with."""
    seq = view.seq
    d = math.inf
    if view.rule == "enter_fold":
        best = math.inf
        for v in seq:
            if v is None:
                continue
            if best != math.inf:
                d = min(d, abs(v - (best - REV_EPS)))
            if v < best - REV_EPS:
                best = v
    else:
        best, row = DBL_MAX, -1
        for i, r in enumerate(seq):
            if r is None:
                continue
            if row >= 0:
                d = min(d, abs(r - (best - REV_EPS)), abs(r - (best + REV_EPS)))
            if r < best - REV_EPS or (abs(r - best) <= REV_EPS and
                                      (row == -1 or view.basic[i] < view.basic[row])):
                best, row = r, i
    return d


# ============================================================================== B&B batch
BB_CAP = 1  # node cap of every B&B item: the root is popped, its two children are solved
BB_W_MAX, BB_G_MAX = (64 * 1024 - 1024) // 4, 160 * 1024 - 1024  # kBatchMaxLdsW / kBatchMaxLdsG


def bb_form(T, cap=BB_CAP) -> int:
    r, c = T.shape[0] + cap, T.shape[1] + cap
    b = 8 * (2 * r * c + r)
    return 0 if b <= BB_W_MAX else (1 if b <= BB_G_MAX else 2)


def _bb_grow(T, form, tall: bool):
    """T padded to form H's footprint with inert rows (zeros, RHS 5) where the walk runs over
    columns, or inert non-basic columns (Z = 2, zeros below) where it runs over rows."""
    while bb_form(T) < form:
        if tall:  # the walk is over rows: widen
            col = np.zeros((T.shape[0], 1))
            col[0, 0] = 2.0
            T = np.hstack([T[:, :-1], col, T[:, -1:]])
        else:
            row = np.zeros((1, T.shape[1]))
            row[0, -1] = 5.0
            T = np.vstack([T, row])
    assert bb_form(T) == form, (T.shape, form)
    return T


def _bb_item(kind, form, seam, label, planted, winner, T, nv, tall, at=1, phase=None, lane0=0,
             mutants=None, **kw):
    T = _bb_grow(np.asarray(T, dtype=np.float64), form, tall)
    return _item(engine="bb", kind=kind, seam=seam, label=label, form=form, at=at, phase=phase,
                 lane0=lane0, planted=tuple(planted), winner=winner,
                 mutants=mutants_of_seam(seam) if mutants is None else mutants, T=T, nv=nv, **kw)


def _bb_counts(form):
    """Walk length per form: past one stride, not a multiple of it."""
    return 75 if form == 0 else 267


def bb_bv_items(form):
    """The branching variable: decision variables at the planted indices are basic at .25 / .75
    (or .5 / .5 on the DPP seams with an odd pair number), one more at .125 (farther from .5)."""
    out = []
    nv = _bb_counts(form)
    for q, (seam, label, pos) in enumerate(seam_pairs(NT_OF_FORM[form], nv, reduced=form == 2)):
        far = free_index(pos, 9)
        cols = nv + 2  # the decision columns, one non-basic column, the RHS
        T = np.zeros((2 + len(pos) + 1, cols))
        T[0, nv], T[0, -1] = 2.0, 40.0
        fr = (0.5, 0.5, 0.5) if q % 2 else (0.25, 0.75, 0.25)
        for k, var in enumerate(tuple(pos) + (far,)):
            T[1 + k, var] = 1.0
            T[1 + k, nv] = 2.0
            T[1 + k, -1] = 2.0 + k + (fr[k] if k < len(pos) else 0.125)
        T[-1, -1] = 5.0
        out.append(_bb_item("bv", form, seam, label, pos, pos[0], T, nv, tall=False))
    return out


def bb_dual_row_items(form):
    """The dual phase's row: the minimum negative RHS (-3) at the planted rows of the lower child;
    on the partial seam the second row is the child's own new row (2 - 2.5 = -0.5).  Each planted
    row has its one negative entry in a column of its own, so another row changes the column too."""
    out = []
    Rc = _bb_counts(form)
    Rn = Rc - 1
    for seam, label, pos in seam_pairs(NT_OF_FORM[form], Rc, reduced=form == 2):
        p = free_index(pos, 5)
        T = np.zeros((Rn, 4 + len(pos)))  # x0, x1, q, one column per planted row, the RHS
        T[0, 1:-1] = 3.0
        T[0, -1] = 40.0
        T[1:, -1] = 5.0
        T[p, 0], T[p, 2], T[p, -1] = 1.0, 2.0, 2.5
        v = -0.5 if pos[-1] == Rn else -3.0
        for k, r in enumerate(pos):
            if r < Rn:
                T[r, 3 + k] = -1.0
                T[r, -1] = v
        out.append(_bb_item("dual_row", form, seam, label, pos, pos[0], T, 2, tall=True, phase=0,
                            observe="row"))
    return out


def bb_dual_theta_items(form, zeros=False):
    """The dual phase's column in the lower child, whose only negative RHS is its new row
    -(row p) with p the basic row of x0: theta_j = Z_j / a_pj is 2 = 2/1 = 4/2 = 8/4 at the
    planted columns and 3 elsewhere; zeros: Z_j = 0 at the planted columns (a = 2) and every
    other theta is +inf, so the column is the first zero theta."""
    out = []
    Cn = _bb_counts(form)  # the child walks its Cn - 1 parent columns and the new slack
    for seam, label, pos in seam_pairs(NT_OF_FORM[form], Cn, last=Cn - 2, reduced=form == 2):
        if zeros and seam == "dpp" and pos[0] % 64 not in (15, 31):
            continue
        T = np.zeros((3, Cn))
        T[0, -1], T[1, -1], T[2, -1] = 40.0, 2.5, 5.0
        T[1, 0] = 1.0
        if zeros:
            T[0, 1:-1] = 3.0
            T[0, list(pos)] = 0.0
            T[1, list(pos)] = 2.0
        else:
            T[0, 1:-1] = 3.0
            T[1, 1:-1] = 1.0
            for k, j in enumerate(pos):
                T[0, j] = 2.0 * (1 << k)
                T[1, j] = float(1 << k)
        out.append(_bb_item("dual_first0" if zeros else "dual_theta", form, seam, label, pos,
                            pos[0], T, 1, tall=False, phase=0, observe="col"))
    return out


def bb_primal_col_items(form):
    """The primal phase's column: the dual phase of the lower child is one pivot on a column with
    Z = 0 that no other row uses, which leaves the Z row as the root has it: -2 at the planted
    columns, 3 elsewhere.  Each planted column has a row of its own to leave through."""
    out = []
    Cn = _bb_counts(form)
    for seam, label, pos in seam_pairs(NT_OF_FORM[form], Cn, last=Cn - 2, reduced=form == 2):
        q = free_index(pos, 5)
        T = np.zeros((2 + len(pos), Cn))
        T[0, 1:-1] = 3.0
        T[0, q] = 0.0
        T[0, list(pos)] = -2.0
        T[0, -1] = 40.0
        T[1, 0], T[1, q], T[1, -1] = 1.0, 2.0, 2.5
        for k, j in enumerate(pos):
            T[2 + k, j] = 1.0
            T[2 + k, -1] = 5.0
        out.append(_bb_item("primal_col", form, seam, label, pos, pos[0], T, 1, tall=False,
                            phase=1, observe="col"))
    return out


def bb_primal_row_items(form, zeros=False):
    """The primal phase's row (rows from 1: lane = row - 1) in the column with Z = -2: theta is
    2 = 2/1 = 4/2 = 8/4 at the planted rows and 5 at two others.  The child's new row cannot hold
    a candidate (its entry in that column would give the dual phase a positive theta), so the
    partial seam ends at the parent's last row, still in the round that is not full.  zeros: b = 0 at the planted rows and no other row has an entry, so there is no positive theta
    and the row is the first zero theta."""
    out = []
    Rn = _bb_counts(form)  # the child walks rows 1..Rn
    for seam, label, pos in seam_pairs(NT_OF_FORM[form], Rn, last=Rn - 2, reduced=form == 2):
        if zeros and seam == "dpp" and pos[0] % 64 not in (15, 31):
            continue
        rows = tuple(x + 1 for x in pos)
        p = free_index(rows, 5)
        T = np.zeros((Rn, 4))  # x0, the entering column, the dual pivot's column, the RHS
        T[0, 1], T[0, -1] = -2.0, 40.0
        T[1:, -1] = 5.0
        T[p, 0], T[p, 2], T[p, -1] = 1.0, 2.0, 2.5
        if zeros:
            for r in rows:
                T[r, 1], T[r, -1] = 2.0, 0.0
        else:
            for k, r in enumerate(rows):
                T[r, 1], T[r, -1] = float(1 << k), 2.0 * (1 << k)
        if not zeros:
            for r in (free_index(rows + (p,), 20), free_index(rows + (p,), 40)):
                T[r, 1] = 1.0
        out.append(_bb_item("primal_first0" if zeros else "primal_row", form, seam, label, rows,
                            rows[0], T, 1, tall=True, phase=1, lane0=1, observe="row"))
    return out


def bb_pivot_row_items(form):
    """add_constraint's pivotRow search for the column of x0: its first rounded 1.0 sits in row
    nt + 5 (lane 5, second round) and another in row 2 nt + 3 (lane 3, third round); a -1 keeps
    the column's sum at 1 so that it counts as basic.  The two rows have their other entry in
    different columns, so the child's first dual pivot shows which row was used."""
    nt = NT_OF_FORM[form]
    p1, p2 = nt + 5, 2 * nt + 3
    Rn = 2 * nt + 8
    T = np.zeros((Rn, 4))  # x0, q1, q2, the RHS
    T[0, 1], T[0, 2], T[0, -1] = 2.0, 2.0, 40.0
    T[1:, -1] = 5.0
    T[p1, 0], T[p1, 1], T[p1, -1] = 1.0, 2.0, 2.5
    T[p2, 0], T[p2, 2], T[p2, -1] = 1.0, 2.0, 4.5
    T[1, 0] = -1.0
    return [_bb_item("pivot_row", form, "stride", f"rows {p1}|{p2}: lane 5 round 1, lane 3 round 2",
                     (p1, p2), p1, T, 1, tall=True, phase=0, observe="col", observed=1,
                     mutants=("last_wins", "lane_major"))]


def bb_items():
    out = []
    for form in (0, 1, 2):
        out += bb_bv_items(form)
        out += bb_dual_row_items(form)
        out += bb_dual_theta_items(form)
        out += bb_dual_theta_items(form, zeros=True)
        out += bb_primal_col_items(form)
        out += bb_primal_row_items(form)
        out += bb_primal_row_items(form, zeros=True)
        out += bb_pivot_row_items(form)
    return out


def bb_child(item):
    """ref_py_bb stepped to the plant: (BranchAndBound, rounded root, decision values, the lower
    child after AddConstraint, the child's tableau at the first pivot of item.phase)."""
    import ref_py_bb as rb
    bb = rb.BranchAndBound(item.nv, BB_CAP)
    root = bb.RoundTableau([list(map(float, r)) for r in item.T])
    vals = bb._decision(root)
    dist = {i: abs((v - rb.floor_total(v)) - 0.5) for i, v in enumerate(vals)
            if not bb.IsInteger(v)}
    var = min(sorted(dist), key=lambda i: dist[i])
    con = [1.0 if i == var else 0.0 for i in range(item.nv)] + \
        [float(rb.to_int32(rb.floor_total(vals[var]))), 0.0]
    child = bb.AddConstraint(con, root)
    tab = [list(r) for r in child]
    if item.phase == 1:  # through the dual phase
        s = rb.DualSimplexSolverBB()
        while True:
            rb._clean(tab)
            if all(row[-1] >= -1e-9 for row in tab):
                break
            tab, th = s.PerformDualPivot(tab)
            assert th is not None, item.name
    else:
        rb._clean(tab)
    return SimpleNamespace(bb=bb, root=root, vals=vals, dist=dist, var=var, child=child, tab=tab)


def bb_view(item):
    """The candidates of the planted selection, from ref_py_bb."""
    import ref_py_bb as rb
    c = bb_child(item)
    t = c.tab
    if item.kind == "bv":
        vals = c.dist
    elif item.kind == "pivot_row":  # the rows of the parent whose rounded entry is a 1.0
        vals = {i: 0.0 for i in range(len(c.root))
                if abs(rb.round4(c.root[i][c.var]) - 1.0) <= 1e-6}
    elif item.kind == "dual_row":
        vals = {i: row[-1] for i, row in enumerate(t) if row[-1] < 0}
    elif item.kind in ("dual_theta", "dual_first0"):
        rhs = [row[-1] for row in t]
        pr = rb._index_of(rhs, min(x for x in rhs if x < 0))
        th = [abs(rb._div(t[0][j], t[pr][j])) if t[pr][j] < 0 else math.inf
              for j in range(len(t[pr]) - 1)]
        all0 = all(x == 0 or x == math.inf for x in th)
        assert all0 == (item.kind == "dual_first0"), item.name
        vals = {j: x for j, x in enumerate(th) if (x == 0 if all0 else 0 < x < math.inf)}
    elif item.kind == "primal_col":
        vals = {j: x for j, x in enumerate(t[0][:-1]) if x < 0}
    else:  # primal_row, primal_first0
        neg = [x for x in t[0][:-1] if x < 0]
        pc = rb._index_of(t[0], min(neg))
        th = {i: (rb._div(t[i][-1], t[i][pc]) if t[i][pc] != 0 else math.inf)
              for i in range(1, len(t))}
        pos = {i: x for i, x in th.items() if 0 < x < math.inf}
        assert bool(pos) == (item.kind == "primal_row"), item.name
        vals = pos if pos else {i: x for i, x in th.items() if x == 0}
    return SimpleNamespace(rule="first_min", vals=vals, nt=item.nt, lane0=item.lane0)


def bb_observed(ref, item):
    """What the log of a B&B run (the oracle's dict, or Records / Trace of a batch) holds at the
    plant: the branched variable of record 1, or the row / column of the first pivot of
    item.phase in the lower child's trace."""
    if item.kind == "bv":
        return ref["records"][1]["var"]
    quad = next(q for q in ref["trace"] if q[0] == item.at and q[1] == item.phase)
    return quad[2] if item.observe == "row" else quad[3]


def bb_expected(item):
    """The value bb_observed must give.  pivot_row's winner is not in the log: the row used shows
    in the column of the child's first dual pivot (column 1 for the first row, 2 for the other)."""
    return item.observed if item.kind == "pivot_row" else item.winner


# ============================================================================== all items
_ITEMS = {}


def items(engine: str):
    """The items of one engine, built once."""
    if engine not in _ITEMS:
        _ITEMS[engine] = dict(primal=primal_items, revised=revised_items, bb=bb_items)[engine]()
        names = [it.name for it in _ITEMS[engine]]
        assert len(set(names)) == len(names), names
    return _ITEMS[engine]


def view_of(item):
    return dict(primal=primal_view, revised=revised_view, bb=bb_view)[item.engine](item)


# The coverage every later change must keep: (engine, kind, form) and (engine, kind, seam class).
EXPECTED_FORM_CELLS = sorted(
    [("primal", k, f) for k in ("entering", "leaving", "leaving_dblmax") for f in "WGH"] +
    [("revised", "enter_fold", f) for f in "WGH"] +
    [("revised", "ratio_fold", f) for f in "GH"] +  # W cannot hold m >= 64
    [("bb", k, f) for k in ("bv", "dual_row", "dual_theta", "dual_first0", "primal_col",
                            "primal_row", "primal_first0", "pivot_row") for f in "WGH"])
EXPECTED_SEAM_CELLS = sorted(
    [("primal", k, s) for k in ("entering", "leaving")
     for s in ("dpp", "wave", "stride", "partial")] +
    [("primal", "leaving_dblmax", s) for s in ("dpp", "wave")] +
    [("revised", "enter_fold", s) for s in ("window", "lane63")] +
    [("revised", "ratio_fold", s) for s in ("window", "lane63")] +
    [("bb", k, s) for k in ("bv", "dual_row", "dual_theta", "primal_col", "primal_row")
     for s in ("dpp", "wave", "stride", "partial")] +
    [("bb", "dual_first0", s) for s in ("dpp", "wave", "stride", "partial")] +
    [("bb", "primal_first0", s) for s in ("dpp", "wave", "stride", "partial")] +
    [("bb", "pivot_row", "stride")])


def coverage_cells():
    form_cells, seam_cells = set(), set()
    for eng in ("primal", "revised", "bb"):
        for it in items(eng):
            form_cells.add((eng, it.kind, FORM_NAME[it.form]))
            seam_cells.add((eng, it.kind, it.seam))
    return sorted(form_cells), sorted(seam_cells)


# ============================================================================== oracle references
_REFS = {}


def primal_ref(oracle, item):
    """test_batch_gpu.oracle_from_tableau of a primal item, computed once and left unchanged."""
    from test_batch_gpu import oracle_from_tableau
    if item.name not in _REFS:
        _REFS[item.name] = oracle_from_tableau(oracle, item.T, item.basis,
                                               max(0, item.T.shape[1] - item.T.shape[0]),
                                               max_pivots=PRIMAL_PIVOTS)
    return _REFS[item.name]


def revised_ref(oracle, item):
    from revised_batch_cases import oracle_ref
    if item.name not in _REFS:
        _REFS[item.name] = oracle_ref(oracle, item.model, REV_CAP)
    return _REFS[item.name]


def bb_ref(oracle, item):
    if item.name not in _REFS:
        _REFS[item.name] = oracle.bb_solve(item.T, item.nv, node_cap=BB_CAP, piv_cap=1 << 12)
    return _REFS[item.name]
