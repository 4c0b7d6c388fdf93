"""Independent pure-Python restatement (TEST ONLY) of what the cutting-plane path WRITES, from the
C# text: IntegerProgramming/CuttingPlaneSolver.cs:47-54, 64-229 (the recursion unrolled),
Simplex/DualSimplex.cs:14-114, 193-207, 228-239 and Simplex/PrimalSimplexSolver2.cs:46-97,
168-189.  It steps the solvers with Python floats (the pivot and Frac of ref_py_cut), collects the
console text as the C# prints it, and on the way records the events and data blocks a narrated
batch keeps: the reference for both.  Not derived from
cut_batch.format_cutting_plane: the text is written where the C# writes it, with the test-side
number formatters of ref_py_text.

The cut limit (exit 6) and hard_cap have no C# counterpart; they stop the walk where the batch
stops, and the text up to there is the prefix the batch's partial text must equal."""
from __future__ import annotations

from ref_py_cut import EPS, INF, PivotTooSmall, _frac, _pivot
from ref_py_text import CRLF, py_fixed, py_format_table

EV_CALL, EV_LEVEL, EV_CUT, EV_SOLVE_BEGIN, EV_SOLVE_END, EV_EXIT, EV_PIVOT = 0, 1, 2, 3, 4, 5, 8
OK, UNBOUNDED, INFEASIBLE, TOO_SMALL, LIMIT = 0, 1, 2, 3, 5   # lpr_status


def py_hashes(v: float, digits: int) -> str:
    """double.ToString("0.###" / "0.####"): the fixed-point image with its trailing zeros (and a
    bare point) dropped; NaN and the infinities as words."""
    s = py_fixed(v, digits)
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return "0" if s in ("", "-", "-0") else s


class Narrated:
    """One item: obj / rows as the C# holds them, the console, the events and the blocks."""

    def __init__(self, tableau, hard_cap=0, text=True, text_limit=None):
        self.with_text = text   # False: the numbers alone (large items)
        self.text_limit = text_limit   # characters after which the console is no longer kept:
        self.text_len = 0              # the text is then a prefix of what the C# writes
        self.obj = [float(v) for v in tableau[0]]
        self.rows = [[float(v) for v in r] for r in tableau[1:]]
        self.hard_cap = hard_cap
        self.console = []
        self.events = []
        self.record0 = self.table()
        self.blocks = []
        self.log = []
        self.snapshots = []
        self.stopped = False   # ended where the C# cannot: exit 6 / 7 or a hard_cap stop

    # -- what is kept ---------------------------------------------------------------------------
    def table(self):
        return [list(self.obj)] + [list(r) for r in self.rows]

    def ev(self, kind, a=0, b=0):
        self.events.append((kind, a, b, len(self.rows) + 1))

    def pivot_done(self, q, row, col):
        self.log.append((q, row, col))
        self.ev(EV_PIVOT + q, row, col)
        self.blocks.append(self.table())

    def write_line(self, s=""):
        if self.with_text:
            self.console.append(s + CRLF)
            self.text_len += len(s) + len(CRLF)
            if self.text_limit is not None and self.text_len >= self.text_limit:
                self.with_text = False

    # -- CuttingPlaneSolver.PrintTableau :47-54 ---------------------------------------------------
    def print_tableau(self, title):
        if not self.with_text:
            return
        self.write_line(title)
        self.write_line("z:  " + "\t".join(py_hashes(v, 4) for v in self.obj))
        for i, r in enumerate(self.rows):
            self.write_line("r%d: " % (i + 1) + "\t".join(py_hashes(v, 4) for v in r))
        self.write_line()

    # -- DualSimplexSolver.Solve :14-114 ----------------------------------------------------------
    def dual_print(self):  # PrintTableau :193-207 with NumVars :228-234
        if not self.with_text:
            return
        n = len(self.obj) - 1 - len(self.rows)
        self.write_line(py_format_table(self.table(), n, "Dual Simplex Tableau"))

    def dual_solve(self, max_iters=10_000, print_steps=True):
        obj, rows = self.obj, self.rows
        width = len(obj)
        it = done = 0
        while True:
            pivot_row, most_neg = -1, 0.0
            for r in range(len(rows)):
                rhs = rows[r][width - 1]
                if rhs < most_neg - EPS or (abs(rhs - most_neg) <= EPS and pivot_row != -1
                                            and r < pivot_row):
                    most_neg, pivot_row = rhs, r
            if pivot_row == -1:
                if print_steps:
                    self.write_line("Dual phase complete: all RHS >= 0.")
                return self.end(OK)
            pivot_col, best = -1, INF
            for j in range(width - 1):
                a = rows[pivot_row][j]
                if a < -EPS:
                    num = obj[j]
                    if abs(num) > EPS:
                        ratio = abs(num / a)
                        if ratio < best - EPS or (abs(ratio - best) <= EPS
                                                  and (pivot_col == -1 or j < pivot_col)):
                            best, pivot_col = ratio, j
            if pivot_col == -1:
                if print_steps:
                    self.write_line("Infeasible: pivot row has no negative coefficients with "
                                    "non-zero ratios.")
                return self.end(INFEASIBLE)
            if self.hard_cap and done >= self.hard_cap:
                return self.end(LIMIT, hard=1)
            if abs(rows[pivot_row][pivot_col]) <= EPS:   # Pivot throws :155-156
                self.end(TOO_SMALL)
                raise PivotTooSmall()
            if print_steps:
                it += 1
                n = width - 1 - len(rows)
                label = "x%d" % (pivot_col + 1) if pivot_col < n else "t%d" % (pivot_col - n + 1)
                self.write_line("\nIteration %d: pivot @ constraint %d, column %s"
                                % (it, pivot_row + 1, label))
                self.dual_print()
            _pivot(obj, rows, pivot_row, pivot_col)
            self.pivot_done(0, pivot_row, pivot_col)
            done += 1
            if print_steps:
                self.write_line("After pivot:")
                self.dual_print()
            if it >= max_iters:
                if print_steps:
                    self.write_line("Max iterations reached.")
                return self.end(LIMIT)

    # -- PrimalSimplexSolver2.Solve :46-97 --------------------------------------------------------
    def capture(self, title):  # CaptureSnapshot :168-182
        if not self.with_text:
            return
        t = self.table()
        sb = [title + CRLF, "Current Tableau:" + CRLF,
              "OBJ\t" + "\t".join(py_hashes(v, 3) for v in t[0]) + CRLF]
        for i in range(1, len(t)):
            sb.append("r%d\t" % i + "\t".join(py_hashes(v, 3) for v in t[i]) + CRLF)
        self.snapshots.append("".join(sb))

    def primal2_print(self):  # :184-189
        if not self.with_text:
            return
        t = self.table()
        self.write_line("OBJ: " + "\t".join(py_hashes(v, 4) for v in t[0]))
        for i in range(1, len(t)):
            self.write_line("r%d: " % i + "\t".join(py_hashes(v, 4) for v in t[i]))

    def primal2_solve(self, max_iters=10_000, print_steps=False):
        # the C# works on its own double[,] and the caller copies it back; the numbers are the same
        self.snapshots = []
        R, C = len(self.rows) + 1, len(self.obj)
        rhs = C - 1
        it = done = 0

        def at(i):
            return self.obj if i == 0 else self.rows[i - 1]

        while True:
            self.capture("Start of iter %d" % it)
            pc, most_neg = -1, 0.0
            for j in range(rhs):
                c = self.obj[j]
                if c < most_neg - EPS or (abs(c - most_neg) <= EPS and pc != -1 and j < pc):
                    most_neg, pc = c, j
            if pc == -1:
                if print_steps:
                    self.write_line("Optimal reached.")
                return self.end(OK)
            best_row, best = -1, INF
            for i in range(1, R):
                a = at(i)[pc]
                if a > EPS:
                    ratio = at(i)[rhs] / a
                    second = True if (abs(ratio - best) <= EPS and best_row == -1) \
                        else (i < best_row)
                    if (ratio > EPS and ratio < best - EPS) or second:
                        best, best_row = ratio, i
            if best_row == -1:
                if print_steps:
                    self.write_line("Unbounded: no valid leaving row.")
                return self.end(UNBOUNDED)
            if self.hard_cap and done >= self.hard_cap:
                return self.end(LIMIT, hard=1)
            piv = at(best_row)[pc]
            if abs(piv) <= EPS:   # Pivot throws :148-149 (the batch ends before the prints)
                self.end(TOO_SMALL)
                raise PivotTooSmall()
            self.capture("Before pivot (iter %d) at row %d, col %d" % (it + 1, best_row, pc))
            if print_steps:
                it += 1
                self.write_line("\nIter %d: pivot @ row %d, col %d" % (it, best_row, pc))
                self.primal2_print()
            prow = at(best_row)
            for j in range(C):
                prow[j] = prow[j] / piv
            for i in range(R):
                if i == best_row:
                    continue
                f = at(i)[pc]
                if abs(f) <= EPS:
                    continue
                row = at(i)
                for j in range(C):
                    row[j] = row[j] - f * prow[j]
            self.pivot_done(1, best_row, pc)
            done += 1
            self.capture("After pivot (iter %d) at row %d, col %d" % (it, best_row, pc))
            if print_steps:
                self.write_line("After pivot:")
                self.primal2_print()
            if it >= max_iters:
                if print_steps:
                    self.write_line("Max iterations reached.")
                return self.end(LIMIT)

    def end(self, status, hard=0):
        self.ev(EV_SOLVE_END, status, hard)
        if hard or status == TOO_SMALL:
            self.stopped = True
        return status

    # -- CuttingPlaneSolution :64-229, one level per pass -----------------------------------------
    def cutting_plane(self, max_cuts=64):
        """-> (exit code, cuts)"""
        self.ev(EV_CALL, 0, 1)
        code, cuts = self._levels(max_cuts)
        self.ev(EV_EXIT, code, 0)
        if code in (6, 7):
            self.stopped = True
        return code, cuts

    def _levels(self, max_cuts):
        obj, rows = self.obj, self.rows
        cuts = 0
        while True:
            self.ev(EV_LEVEL)
            self.print_tableau("Initial tableau:")
            fractional = []
            for i, row in enumerate(rows):
                fr = _frac(row[-1])
                if fr > EPS:
                    fractional.append((i, fr))
            if not fractional:
                self.write_line("All RHS are integers. No Gomory cut needed.")
                return 1, cuts
            if cuts >= max_cuts:
                return 6, cuts
            fractional.sort(key=lambda t: abs(t[1] - 0.5))   # a stable sort on this input
            src = fractional[0][0]
            n = len(obj)
            cut = [-_frac(rows[src][j]) for j in range(n)]
            rows.append(cut)
            cuts += 1
            self.ev(EV_CUT, src)
            self.blocks.append(list(cut))
            cut_idx = len(rows) - 1
            pc, best = -1, INF
            for j in range(n - 1):
                a = cut[j]
                if a < -EPS:
                    num = obj[j]
                    if abs(num) > EPS:
                        ratio = abs(num / a)
                        if ratio < best - EPS or (abs(ratio - best) <= EPS
                                                  and (pc == -1 or j < pc)):
                            best, pc = ratio, j
            if pc == -1:
                self.write_line("No valid pivot column on the cut (need a negative cut coeff "
                                "with non-zero obj coeff).")
                return 2, cuts
            self.print_tableau("Before pivot on cut: row %d, col %d" % (cut_idx + 1, pc + 1))
            if abs(rows[cut_idx][pc]) <= EPS:
                self.write_line("Pivot too small/zero.")
                return 3, cuts
            _pivot(obj, rows, cut_idx, pc)
            self.pivot_done(2, cut_idx, pc)
            self.print_tableau("After pivot on cut: row %d, col %d" % (cut_idx + 1, pc + 1))
            need_dual = any(r[-1] < -EPS for r in rows)
            need_primal = any(obj[j] < -EPS for j in range(n - 1))
            try:
                if need_dual:
                    self.write_line("Negative RHS detected → running Dual Simplex...")
                    self.ev(EV_SOLVE_BEGIN, 0)
                    if self.dual_solve(print_steps=True) != OK:
                        self.write_line("Dual Simplex failed (infeasible or max iters).")
                        return 4, cuts
                    self.print_tableau("After Dual Simplex:")
                    need_primal = any(obj[j] < -EPS for j in range(n - 1))
                if need_primal:
                    self.write_line("Negative reduced cost detected → running Primal "
                                    "Simplex...")
                    self.ev(EV_SOLVE_BEGIN, 1)
                    self.primal2_solve(print_steps=True)
                    self.print_tableau("After Primal Simplex:")
            except PivotTooSmall:
                return 7, cuts
            if not any(obj[j] < -EPS for j in range(n - 1)) and \
                    not any(r[-1] < -EPS for r in rows):
                if any(_frac(r[-1]) > EPS for r in rows):
                    self.write_line("Objective optimal but RHS has fractional values → "
                                    "adding another Gomory cut...")
                    continue
                self.write_line("Displayed the Optimal Tableau.")
                return 0, cuts
            self.write_line("Cutting-plane step finished (further steps may be required).")
            return 5, cuts

    # -- one Solve alone (modes 1 / 2 of the batch) -----------------------------------------------
    def solve_alone(self, mode, max_iters=10_000, print_steps=True):
        """-> lpr_status"""
        self.ev(EV_CALL, mode, 1 if print_steps else 0)
        self.ev(EV_SOLVE_BEGIN, mode - 1)
        try:
            st = (self.dual_solve if mode == 1 else self.primal2_solve)(max_iters, print_steps)
        except PivotTooSmall:
            st = TOO_SMALL
        self.ev(EV_EXIT, st, 0)
        return st

    @property
    def text(self):
        return "".join(self.console)


def narrate_cutting_plane(tableau, max_cuts=64, hard_cap=0, text=True, text_limit=None):
    n = Narrated(tableau, hard_cap, text, text_limit)
    code, cuts = n.cutting_plane(max_cuts)
    return n, code, cuts


def narrate_solve(tableau, mode, max_iters=10_000, print_steps=True, hard_cap=0, text=True):
    n = Narrated(tableau, hard_cap, text)
    return n, n.solve_alone(mode, max_iters, print_steps)
