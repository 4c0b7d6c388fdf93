// GpuSolvers.cs -- drop-in bodies for the three solver classes of LPR_381_Group_V22, calling the
// MI355X engine through NativeMethods.  UNVERIFIED (never compiled: no C# toolchain in the build
// image).  Public members, argument meaning and error behaviour are those of the reference classes
// so that Program.cs (cases "1", "2", "3", "5") compiles unchanged when these replace
// Simplex/PrimalSimplexSolver.cs, Simplex/RevisedPrimalSimplexSolver.cs,
// IntegerProgramming/BranchAndBoundAdapter.cs and IntegerProgramming/KnapsackBranchBoundSolver.cs
// (an empty class in the reference; KnapsackBranchBoundSimplex is defined nowhere there).
using System;
using System.Collections.Generic;
using System.Linq;
using LPR_381_Group_V22.Native;
using LPR_381_Group_V22.Utilities;
using IOConstraint = LPR_381_Group_V22.IO.InputFileParser.Constraint;

namespace LPR_381_Group_V22.Simplex
{
    public class PrimalSimplexSolver : IDisposable
    {
        private readonly int numVariables, numConstraints;
        internal IntPtr Tableau;                       // lpr_tableau*
        public List<string> IterationSnapshots = new List<string>();
        public double FinalZ { get; private set; }
        public List<double> SolutionVector { get; private set; }
        public double[,] FinalTableau { get; private set; }
        /// <summary>Snapshots are O(R*C) text each; off above this many elements.</summary>
        public static int SnapshotElementLimit = 4096;

        public PrimalSimplexSolver(List<double> objective, List<IOConstraint> constraints, bool isMaximization = true)
        {
            numVariables = objective.Count;
            numConstraints = constraints.Count;
            int n = numVariables, m = numConstraints;
            var A = new double[Math.Max(1, m * n)];
            var ncoef = new int[Math.Max(1, m)];
            var rel = new sbyte[Math.Max(1, m)];
            var rhs = new double[Math.Max(1, m)];
            for (int i = 0; i < m; i++)
            {
                int k = Math.Min(n, constraints[i].Coefficients.Count);   // PrimalSimplexSolver.cs:68-72
                for (int j = 0; j < k; j++) A[i * n + j] = constraints[i].Coefficients[j];
                ncoef[i] = k;
                rel[i] = (sbyte)(constraints[i].Relation == ">=" ? 1 : constraints[i].Relation == "=" ? 2 : 0);
                rhs[i] = constraints[i].RHS;
            }
            NativeMethods.ThrowIfError(NativeMethods.lpr_tableau_from_lp(Engine.Handle, n, m, objective.ToArray(), A, n,
                ncoef, rel, rhs, isMaximization ? 1 : 0, out Tableau), "lpr_tableau_from_lp");
            if ((long)(m + 1) * (n + m + 1) <= SnapshotElementLimit) CaptureSnapshot("Initial Tableau");
        }

        public void Solve()
        {
            var opts = new LprSolveOpts();
            NativeMethods.ThrowIfError(NativeMethods.lpr_primal_solve(Tableau, ref opts, out var res), "lpr_primal_solve");
            if (res.status == (int)LprStatus.Optimal)
            {
                var x = new double[Math.Max(1, numVariables)];
                NativeMethods.lpr_extract_solution(Tableau, numVariables, x, out double z);
                FinalZ = z;                                            // :113
                SolutionVector = x.Take(numVariables).ToList();        // :114
                FinalTableau = GetFinalTableau();                      // :116
                Console.WriteLine("Optimal Solution Found!");
            }
            else if (res.status == (int)LprStatus.Unbounded)
            {
                Console.WriteLine("Unbounded Solution!");             // :131, FinalZ stays 0, SolutionVector null
                FinalTableau = GetFinalTableau();
            }
        }

        public double[,] GetFinalTableau()
        {
            NativeMethods.lpr_tableau_shape(Tableau, out int r, out int c, out _);
            var t = new double[r, c];
            NativeMethods.ThrowIfError(NativeMethods.lpr_tableau_read(Tableau, t), "lpr_tableau_read");
            return t;
        }

        public List<int> BasicVariables
        {
            get { var b = new int[Math.Max(1, numConstraints)]; NativeMethods.lpr_basis_read(Tableau, b); return b.Take(numConstraints).ToList(); }
        }

        private void CaptureSnapshot(string title) =>
            IterationSnapshots.Add(TableIterationFormater.Format(GetFinalTableau(), numVariables, title));

        public void Dispose() { if (Tableau != IntPtr.Zero) { NativeMethods.lpr_tableau_destroy(Tableau); Tableau = IntPtr.Zero; } }
    }

    /// <summary>
    /// Many PrimalSimplexSolver models in one call (no reference counterpart: the reference solves one model per
    /// object).  Each LP is built and solved on the device with the rules of PrimalSimplexSolver.cs, the same bits a
    /// PrimalSimplexSolver gives for it alone; members are per-LP versions of that class's.  With traceCap > 0 the
    /// batch is traced (DESIGN.md section 22): the device stores the tableau after every pivot and
    /// IterationSnapshots(k) formats LP k's; an untraced batch keeps none.
    /// </summary>
    public class PrimalSimplexBatch : IDisposable
    {
        private IntPtr batch;                           // lpr_batch*
        internal IntPtr Handle => batch;
        private readonly int[] rows, cols, nvars;
        private readonly int traceCap;                  // records kept per LP; 0: untraced
        private long[] traceRecords;                    // lpr_batch_trace_info's counts, read once per Solve
        public int Count { get; }
        public List<int> Status { get; } = new List<int>();
        public List<long> Iterations { get; } = new List<long>();
        public List<double> FinalZ { get; } = new List<double>();
        public List<List<double>> SolutionVector { get; } = new List<List<double>>();

        public PrimalSimplexBatch(List<(List<double> objective, List<IOConstraint> constraints, bool isMaximization)> models, int logCap = 0, int traceCap = 0)
        {
            Count = models.Count;
            var n = new int[Count]; var m = new int[Count]; var isMax = new sbyte[Count];
            var obj = new List<double>(); var A = new List<double>(); var ncoef = new List<int>();
            var rel = new List<sbyte>(); var rhs = new List<double>();
            rows = new int[Count]; cols = new int[Count]; nvars = new int[Count];
            for (int k = 0; k < Count; k++)
            {
                var (objective, constraints, isMaximization) = models[k];
                n[k] = objective.Count; m[k] = constraints.Count; isMax[k] = (sbyte)(isMaximization ? 1 : 0);
                obj.AddRange(objective);
                foreach (var c in constraints)
                {
                    int cnt = Math.Min(n[k], c.Coefficients.Count);        // PrimalSimplexSolver.cs:68-72
                    for (int j = 0; j < n[k]; j++) A.Add(j < cnt ? c.Coefficients[j] : 0.0);
                    ncoef.Add(cnt);
                    rel.Add((sbyte)(c.Relation == ">=" ? 1 : c.Relation == "=" ? 2 : 0));
                    rhs.Add(c.RHS);
                }
                rows[k] = m[k] + 1; cols[k] = n[k] + m[k] + 1; nvars[k] = n[k];
            }
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_from_lps(Engine.Handle, Count, n, m, NonEmpty(obj), NonEmpty(A),
                NonEmpty(ncoef), NonEmpty(rel), NonEmpty(rhs), isMax, logCap, out batch), "lpr_batch_from_lps");
            if (traceCap > 0) NativeMethods.ThrowIfError(NativeMethods.lpr_batch_trace_reserve(batch, traceCap), "lpr_batch_trace_reserve");
            this.traceCap = traceCap;
        }

        private static T[] NonEmpty<T>(List<T> l) => l.Count > 0 ? l.ToArray() : new T[1];

        /// <summary>Solve() of every unfinished LP; an LP stopped by maxPivots resumes on the next call.</summary>
        public void Solve(long maxPivots = 0)
        {
            var opts = new LprBatchOpts { max_pivots = maxPivots };
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_solve(batch, ref opts, out _), "lpr_batch_solve");
            var st = new int[Count]; var piv = new long[Count]; var z = new double[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_status_read(batch, st, piv, z), "lpr_batch_status_read");
            var x = new double[Math.Max(1, nvars.Sum())];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_solution_read(batch, x), "lpr_batch_solution_read");
            Status.Clear(); Iterations.Clear(); FinalZ.Clear(); SolutionVector.Clear();
            traceRecords = null;
            for (int k = 0, at = 0; k < Count; at += nvars[k], k++)
            {
                Status.Add(st[k]); Iterations.Add(piv[k]);
                bool optimal = st[k] == (int)LprStatus.Optimal;
                FinalZ.Add(optimal ? z[k] : 0.0);                          // :113; stays 0 on the unbounded exit
                SolutionVector.Add(optimal ? x.Skip(at).Take(nvars[k]).ToList() : null);
            }
        }

        public List<int> BasicVariables(int k)
        {
            var b = new int[Math.Max(1, rows.Sum() - Count)];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_basis_read(batch, b), "lpr_batch_basis_read");
            return b.Skip(rows.Take(k).Sum() - k).Take(rows[k] - 1).ToList();
        }

        public List<(int row, int col)> PivotLog(int k)
        {
            const int cap = 1 << 16;
            var r = new int[cap]; var c = new int[cap];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_log_read(batch, k, r, c, cap, out long count), "lpr_batch_log_read");
            var log = new List<(int, int)>();
            for (long q = 0; q < count; q++) log.Add((r[q], c[q]));
            return log;
        }

        public double[,] GetFinalTableau(int k)
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_shape(batch, k, out int r, out int c, out _), "lpr_batch_shape");
            var t = new double[r, c];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_tableau_read(batch, k, t), "lpr_batch_tableau_read");
            return t;
        }

        /// <summary>Records LP k has: 1 + pivots (may exceed traceCap).  The reference's list holds one more entry when
        /// the LP is optimal or unbounded.</summary>
        public long RecordCount(int k)
        {
            if (traceRecords == null)
            {
                var recs = new long[Count];
                NativeMethods.ThrowIfError(NativeMethods.lpr_batch_trace_info(batch, recs, null, null), "lpr_batch_trace_info");
                traceRecords = recs;
            }
            return traceRecords[k];
        }

        /// <summary>Every LP's records in one copy: record i of LP k starts at offset[k] + i * stride[k].</summary>
        public double[] TracePacked(out long[] records, out long[] offset, out long[] stride)
        {
            records = new long[Count]; offset = new long[Count]; stride = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_trace_info(batch, records, offset, stride), "lpr_batch_trace_info");
            var slab = new double[checked((long)traceCap * stride.Sum())];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_trace_read_all(batch, slab, slab.LongLength), "lpr_batch_trace_read_all");
            return slab;
        }

        /// <summary>IterationSnapshots of LP k (PrimalSimplexSolver.cs:86, :148, :118-122, :133): "Initial Tableau" and
        /// "Iteration i - After pivot" formatted from the device's records (past traceCap the kept prefix), then the final
        /// block from the LP's tableau in the batch.  Call after Solve().</summary>
        public List<string> IterationSnapshots(int k)
        {
            int r = rows[k], c = cols[k];
            long stride = 2 + (long)r * c;                               // batch_trace_stride
            long kept = Math.Min(RecordCount(k), traceCap);
            var recs = new double[Math.Max(1L, checked(kept * stride))];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_trace_read(batch, k, 0, kept, recs), "lpr_batch_trace_read");
            var list = new List<string>();
            for (long q = 0; q < kept; q++)
            {
                var t = new double[r, c];
                Array.Copy(recs, q * stride + 2, t, 0L, (long)r * c);      // long indices: kept records may pass 2 GB
                list.Add(TableIterationFormater.Format(t, nvars[k], q == 0 ? "Initial Tableau" : $"Iteration {q} - After pivot"));
            }
            if (Status[k] == (int)LprStatus.Optimal)
            {
                var sb = new System.Text.StringBuilder();
                sb.AppendLine(TableIterationFormater.Format(GetFinalTableau(k), nvars[k], "Final Tableau (Optimal)"));
                var sum = new System.Text.StringBuilder();                  // SolutionSummary :256-267
                sum.AppendLine("Optimal solution:");
                sum.AppendLine($"Z = {FinalZ[k]:F6}");
                for (int i = 0; i < nvars[k]; i++) sum.AppendLine($"x{i + 1} = {SolutionVector[k][i]:F6}");
                sb.AppendLine(sum.ToString());
                list.Add(sb.ToString());
            }
            else if (Status[k] == (int)LprStatus.Unbounded)
                list.Add(TableIterationFormater.Format(GetFinalTableau(k), nvars[k], "Unbounded Tableau"));
            return list;
        }

        /// <summary>Every kept record of every LP, and the final tableau of every LP that ended, formatted on the device
        /// (DESIGN.md section 25): block firstBlock[k] + i is the body of LP k's record i, the block after its kept records
        /// the body of its final tableau.  Prepend "\n" + title + ":" + Environment.NewLine for the text Format gives.</summary>
        public DeviceText FormatTrace(out long[] firstBlock)
        {
            firstBlock = new long[Count + 1];
            NativeMethods.ThrowIfError(NativeMethods.lpr_batch_trace_text(batch, firstBlock, out IntPtr text), "lpr_batch_trace_text");
            return new DeviceText(text);
        }

        public void Dispose() { if (batch != IntPtr.Zero) { NativeMethods.ThrowIfError(NativeMethods.lpr_batch_destroy(batch), "lpr_batch_destroy"); batch = IntPtr.Zero; } }
    }

    /// <summary>Blocks of TableIterationFormater.Format (TableIterationFormater.cs:22-48) without their title lines, written on
    /// the device (DESIGN.md section 25).  Owns the lpr_text handle; offsets and bytes are read once.</summary>
    public class DeviceText : IDisposable
    {
        private IntPtr text;                            // lpr_text*
        private long[] offsets;
        private byte[] data;
        public long Count { get; }
        public long Bytes { get; }
        public double KernelMs { get; }

        internal DeviceText(IntPtr handle)
        {
            text = handle;
            NativeMethods.ThrowIfError(NativeMethods.lpr_text_info(text, out long blocks, out long bytes, out double ms), "lpr_text_info");
            Count = blocks; Bytes = bytes; KernelMs = ms;
        }

        /// <summary>One block per tableau: Format(tab, nvars[k], title) without its title line.</summary>
        public static DeviceText FormatTableaux(IntPtr engine, List<double[,]> tableaux, int[] nvars)
        {
            var rows = tableaux.Select(t => t.GetLength(0)).ToArray();
            var cols = tableaux.Select(t => t.GetLength(1)).ToArray();
            var flat = new List<double>();
            foreach (var t in tableaux) foreach (double v in t) flat.Add(v);   // row-major
            NativeMethods.ThrowIfError(NativeMethods.lpr_text_format_tableaux(engine, tableaux.Count, rows, cols, nvars, flat.ToArray(), out IntPtr h),
                                       "lpr_text_format_tableaux");
            return new DeviceText(h);
        }

        /// <summary>DisplayTableau (BranchBoundSimplexSolver.cs:623-640) per tableau: Format of tableau k after round4[k]
        /// (0, 1 or 2) applications of Math.Round(v, 4), without its title line (DESIGN.md section 26).</summary>
        public static DeviceText FormatTableauxRounded(IntPtr engine, List<double[,]> tableaux, int[] nvars, int[] round4)
        {
            var rows = tableaux.Select(t => t.GetLength(0)).ToArray();
            var cols = tableaux.Select(t => t.GetLength(1)).ToArray();
            var flat = new List<double>();
            foreach (var t in tableaux) foreach (double v in t) flat.Add(v);   // row-major
            NativeMethods.ThrowIfError(NativeMethods.lpr_text_format_tableaux_rounded(engine, tableaux.Count, rows, cols, nvars, round4, flat.ToArray(), out IntPtr h),
                                       "lpr_text_format_tableaux_rounded");
            return new DeviceText(h);
        }

        public string Block(long i)
        {
            if (data == null)
            {
                offsets = new long[Count + 1];
                NativeMethods.ThrowIfError(NativeMethods.lpr_text_offsets_read(text, offsets), "lpr_text_offsets_read");
                data = new byte[Math.Max(1L, Bytes)];
                NativeMethods.ThrowIfError(NativeMethods.lpr_text_read(text, 0, Bytes, data), "lpr_text_read");
            }
            return System.Text.Encoding.ASCII.GetString(data, checked((int)offsets[i]), checked((int)(offsets[i + 1] - offsets[i])));
        }

        public void Dispose() { if (text != IntPtr.Zero) { NativeMethods.ThrowIfError(NativeMethods.lpr_text_destroy(text), "lpr_text_destroy"); text = IntPtr.Zero; } }
    }

    /// <summary>RevisedPrimalSimplexSolver.Solve() + ExtractSolution (RevisedPrimalSimplexSolver.cs:82-251, :277-287) for many
    /// LPs in one device call (DESIGN.md section 17); each LP gives the bits of RevisedPrimalSimplexSolver alone.  With
    /// traceCap > 0 the batch is traced (section 21): the device records every CaptureSnapshot as numbers and
    /// IterationSnapshots(k) formats LP k's; an untraced batch keeps none.</summary>
    public class RevisedSimplexBatch : IDisposable
    {
        private IntPtr batch;                           // lpr_rev_batch*
        private readonly int[] nvars, ncons;
        private readonly bool[] isMinModel;
        private readonly int traceCap;                  // records kept per LP; 0: untraced
        public int Count { get; }
        public List<int> Status { get; } = new List<int>();
        public List<long> Iterations { get; } = new List<long>();
        public List<double> FinalZ { get; } = new List<double>();
        public List<List<double>> SolutionVector { get; } = new List<List<double>>();

        public RevisedSimplexBatch(List<(List<double> objective, List<IOConstraint> constraints, bool isMinimization)> models, int logCap = 0, int traceCap = 0)
        {
            Count = models.Count;
            nvars = new int[Count]; ncons = new int[Count]; var isMin = new sbyte[Count];
            isMinModel = models.Select(mdl => mdl.isMinimization).ToArray();
            var obj = new List<double>(); var A = new List<double>(); var b = new List<double>();
            for (int k = 0; k < Count; k++)
            {
                var (objective, constraints, isMinimization) = models[k];
                if (objective == null || objective.Count == 0) throw new ArgumentException($"model {k}: Objective cannot be null or empty.");          // :43
                if (constraints == null || constraints.Count == 0) throw new ArgumentException($"model {k}: Constraints cannot be null or empty.");  // :44
                nvars[k] = objective.Count; ncons[k] = constraints.Count; isMin[k] = (sbyte)(isMinimization ? 1 : 0);
                obj.AddRange(objective);
                for (int i = 0; i < constraints.Count; i++)
                {
                    if (constraints[i].Coefficients.Count != nvars[k]) throw new ArgumentException($"model {k}: Constraint {i + 1} has incorrect number of coefficients.");  // :57-58
                    A.AddRange(constraints[i].Coefficients); b.Add(constraints[i].RHS);   // Relation is never read (:55-61)
                }
            }
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_create(Engine.Handle, Count, nvars, ncons, obj.ToArray(), A.ToArray(),
                b.ToArray(), isMin, logCap, out batch), "lpr_rev_batch_create");
            if (traceCap > 0) NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_trace_reserve(batch, traceCap), "lpr_rev_batch_trace_reserve");
            this.traceCap = traceCap;
        }

        /// <summary>Solve() of every unfinished LP; an LP stopped by maxPivots resumes on the next call.</summary>
        public void Solve(long maxPivots = 0)
        {
            var opts = new LprRevBatchOpts { max_pivots = maxPivots };
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_solve(batch, ref opts, out _), "lpr_rev_batch_solve");
            var st = new int[Count]; var it = new long[Count]; var z = new double[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_status_read(batch, st, it, z), "lpr_rev_batch_status_read");
            var x = new double[nvars.Sum()];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_solution_read(batch, x), "lpr_rev_batch_solution_read");
            Status.Clear(); Iterations.Clear(); FinalZ.Clear(); SolutionVector.Clear();
            for (int k = 0, at = 0; k < Count; at += nvars[k], k++)
            {
                Status.Add(st[k]); Iterations.Add(it[k]);
                bool optimal = st[k] == (int)LprStatus.Optimal;
                FinalZ.Add(optimal ? z[k] : 0.0);                                  // :284, set on the optimal exit only
                SolutionVector.Add(optimal ? x.Skip(at).Take(nvars[k]).ToList() : null);
            }
        }

        public List<int> BasicVariables(int k)
        {
            var all = new int[ncons.Sum()];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_basis_read(batch, all), "lpr_rev_batch_basis_read");
            return all.Skip(ncons.Take(k).Sum()).Take(ncons[k]).ToList();
        }

        public List<(int row, int enter, int leave)> PivotLog(int k)
        {
            const int cap = 1 << 12;
            var r = new int[cap]; var e = new int[cap]; var l = new int[cap];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_log_read(batch, k, r, e, l, cap, out long count), "lpr_rev_batch_log_read");
            var log = new List<(int, int, int)>();
            for (long q = 0; q < Math.Min(count, cap); q++) log.Add((r[q], e[q], l[q]));
            return log;
        }

        public double[,] BInverse(int k)
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_shape(batch, k, out _, out int m), "lpr_rev_batch_shape");
            var t = new double[m, m];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_binv_read(batch, k, t), "lpr_rev_batch_binv_read");
            return t;
        }

        public double[] XB(int k)
        {
            var xb = new double[ncons[k]];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_xb_read(batch, k, xb), "lpr_rev_batch_xb_read");
            return xb;
        }

        /// <summary>Snapshots the reference's list of LP k would hold (may exceed traceCap).</summary>
        public long SnapshotCount(int k)
        {
            var snaps = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_trace_info(batch, snaps, null, null), "lpr_rev_batch_trace_info");
            return snaps[k];
        }

        /// <summary>Every LP's records in one copy: record i of LP k starts at offset[k] + i * stride[k].</summary>
        public double[] TracePacked(out long[] snapshots, out long[] offset, out long[] stride)
        {
            snapshots = new long[Count]; offset = new long[Count]; stride = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_trace_info(batch, snapshots, offset, stride), "lpr_rev_batch_trace_info");
            var slab = new double[traceCap * stride.Sum()];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_trace_read_all(batch, slab, slab.LongLength), "lpr_rev_batch_trace_read_all");
            return slab;
        }

        /// <summary>IterationSnapshots of LP k (RevisedPrimalSimplexSolver.cs:35): "Iteration i" per pivot and "Optimal",
        /// formatted from the device's records; past traceCap the list stops after the kept prefix.</summary>
        public List<string> IterationSnapshots(int k)
        {
            int n = nvars[k], m = ncons[k];
            long stride = 6 + 7L * m + n + (long)m * n + (long)m * m;   // rev_trace_stride
            long kept = Math.Min(SnapshotCount(k), traceCap);
            var recs = new double[Math.Max(1, kept * stride)];
            NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_trace_read(batch, k, 0, kept, recs), "lpr_rev_batch_trace_read");
            var list = new List<string>();
            for (long q = 0; q < kept; q++)
            {
                long at = q * stride;
                Func<long, int, double[]> take = (off, len) => { var v = new double[len]; Array.Copy(recs, at + off, v, 0, len); return v; };
                int entering = (int)recs[at], leavingRow = (int)recs[at + 1], leavingVar = (int)recs[at + 2];
                long o = 6;
                double[] y = take(o, m); o += m;
                double[] rcX = take(o, n); o += n;
                double[] rcS = take(o, m); o += m;
                double[] u = take(o, m); o += m;
                double[] ratios = take(o, m); o += m;
                List<int> basisPre = take(o, m).Select(v => (int)v).ToList(); o += m;
                List<int> basisPost = take(o, m).Select(v => (int)v).ToList(); o += m;
                double[] xB = take(o, m); o += m;
                var binvA = new double[m, n]; var binv = new double[m, m];
                Buffer.BlockCopy(recs, (int)((at + o) * sizeof(double)), binvA, 0, m * n * sizeof(double)); o += (long)m * n;
                Buffer.BlockCopy(recs, (int)((at + o) * sizeof(double)), binv, 0, m * m * sizeof(double));
                list.Add(RevisedPrimalSimplexSolver.FormatSnapshot(n, m, isMinModel[k], basisPost, entering < 0 ? "Optimal" : $"Iteration {q + 1}", xB, y,
                    rcX, rcS, entering, recs[at + 3], u, ratios, basisPre, leavingRow, leavingVar, recs[at + 4], recs[at + 5], binvA, binv));
            }
            return list;
        }

        public void Dispose() { if (batch != IntPtr.Zero) { NativeMethods.ThrowIfError(NativeMethods.lpr_rev_batch_destroy(batch), "lpr_rev_batch_destroy"); batch = IntPtr.Zero; } }
    }

    /// <summary>BranchAndBoundAdapter.SolveFromPrimal + ExecuteBranchAndBound (BranchBoundSimplexSolver.cs:1006-1233)
    /// for many IPs in one device call (DESIGN.md section 13); each IP gives the bits of BranchAndBound alone.</summary>
    public class BranchAndBoundBatch : IDisposable
    {
        private IntPtr bb;                              // lpr_bb_batch*
        private readonly int[] nvars;
        private readonly int[] rootRows, rootCols;      // the roots' shapes: a child at depth d is d larger each way
        private readonly int nodeCap;
        public int Count { get; }
        public List<int> Status { get; } = new List<int>();
        public List<double> OptimalValue { get; } = new List<double>();
        public List<List<double>> OptimalSolution { get; } = new List<List<double>>();

        /// <summary>Root tableaux (FinalTableau of each primal solve) and SetNumVars per IP.</summary>
        public BranchAndBoundBatch(List<double[,]> roots, List<int> numVars, int nodeCap = 0, int traceCap = 0)
        {
            Count = roots.Count;
            var r = new int[Count]; var c = new int[Count]; var flat = new List<double>();
            nvars = numVars.ToArray();
            for (int k = 0; k < Count; k++)
            {
                r[k] = roots[k].GetLength(0); c[k] = roots[k].GetLength(1);
                foreach (var v in roots[k]) flat.Add(v);                       // row-major
            }
            rootRows = r; rootCols = c;
            this.nodeCap = nodeCap > 0 ? nodeCap : 20;
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_create(Engine.Handle, Count, r, c, flat.ToArray(), nvars,
                nodeCap, traceCap, out bb), "lpr_bb_batch_create");
        }

        /// <summary>SolveFromPrimal (BranchAndBoundAdapter.cs:9-24) for every LP of a solved PrimalSimplexBatch.</summary>
        public BranchAndBoundBatch(PrimalSimplexBatch primal, int nodeCap = 0, int traceCap = 0)
        {
            Count = primal.Count;
            nvars = new int[Count]; rootRows = new int[Count]; rootCols = new int[Count];
            for (int k = 0; k < Count; k++)                                     // :20
            {
                var root = primal.GetFinalTableau(k);
                rootRows[k] = root.GetLength(0); rootCols[k] = root.GetLength(1);
                nvars[k] = primal.SolutionVector[k] != null ? primal.SolutionVector[k].Count : Math.Max(1, rootCols[k] - 1);
            }
            this.nodeCap = nodeCap > 0 ? nodeCap : 20;
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_from_batch(primal.Handle, nodeCap, traceCap, out bb),
                "lpr_bb_batch_from_batch");
        }

        /// <summary>ExecuteBranchAndBound for every IP; x is null where no integer solution was found (:1215-1232).</summary>
        public void Run(bool enablePruning = false)
        {
            var opts = new LprBbBatchOpts { enable_pruning = enablePruning ? 1 : 0 };
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_run(bb, ref opts, out _), "lpr_bb_batch_run");
            var st = new int[Count]; var found = new int[Count]; var z = new double[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_result_read(bb, st, found, null, null, z, null, null),
                "lpr_bb_batch_result_read");
            var x = new double[Math.Max(1, nvars.Sum())];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_solution_read(bb, x), "lpr_bb_batch_solution_read");
            Status.Clear(); OptimalValue.Clear(); OptimalSolution.Clear();
            for (int k = 0, at = 0; k < Count; at += nvars[k], k++)
            {
                Status.Add(st[k]); OptimalValue.Add(z[k]);
                OptimalSolution.Add(found[k] != 0 ? x.Skip(at).Take(nvars[k]).ToList() : null);
            }
        }

        public List<int> PopOrder(int k)
        {
            var ids = new int[nodeCap];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_pop_order_read(bb, k, ids, nodeCap, out long count),
                "lpr_bb_batch_pop_order_read");
            return ids.Take((int)count).ToList();
        }

        public List<(int parent, int kind, int depth, int var, double bound, int status, double z)> Records(int k)
        {
            int cap = 1 + 2 * nodeCap;
            var p = new int[cap]; var kd = new int[cap]; var d = new int[cap]; var v = new int[cap];
            var b = new double[cap]; var s = new int[cap]; var z = new double[cap];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_records_read(bb, k, p, kd, d, v, b, s, z, cap, out long count),
                "lpr_bb_batch_records_read");
            var recs = new List<(int, int, int, int, double, int, double)>();
            for (long q = 0; q < count; q++) recs.Add((p[q], kd[q], d[q], v[q], b[q], s[q], z[q]));
            return recs;
        }

        public List<(int node, int phase, int row, int col)> Trace(int k, int cap = 1 << 16)
        {
            var q4 = new int[4 * cap];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_trace_read(bb, k, q4, cap, out long count),
                "lpr_bb_batch_trace_read");
            var tr = new List<(int, int, int, int)>();
            for (long q = 0; q < count; q++) tr.Add((q4[4 * q], q4[4 * q + 1], q4[4 * q + 2], q4[4 * q + 3]));
            return tr;
        }

        // ---- narration (DESIGN.md section 23): what ExecuteBranchAndBound writes to the console, from the device's numbers ----
        private bool pruning;                          // of the last Narrate

        /// <summary>The two-pass flow: reserve nothing, run, read the exact needs, reserve them, run again (a run is
        /// deterministic and starts from the roots).</summary>
        public void Narrate(bool enablePruning = false)
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_reserve(bb, new long[Count]), "lpr_bb_batch_narrate_reserve");
            Run(enablePruning);
            var need = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_info(bb, null, need, null, null), "lpr_bb_batch_narrate_info");
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_reserve(bb, need), "lpr_bb_batch_narrate_reserve");
            Run(enablePruning);
            pruning = enablePruning;
        }

        /// <summary>The whole slab of child tableaux in one copy; `total` is the sum of the reserved doubles.</summary>
        public double[] NarrationSlab(long total)
        {
            var slab = new double[Math.Max(1, total)];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_read_all(bb, slab, slab.LongLength), "lpr_bb_batch_narrate_read_all");
            return slab;
        }

        private static double[,] Block(double[] flat, long at, int rows, int cols)
        {
            var t = new double[rows, cols];
            Buffer.BlockCopy(flat, (int)(at * sizeof(double)), t, 0, rows * cols * sizeof(double));
            return t;
        }

        private static double[,] Rounded(double[,] t)   // RoundTableau :552-567
        {
            var r = (double[,])t.Clone();
            for (int i = 0; i < r.GetLength(0); i++) for (int j = 0; j < r.GetLength(1); j++) r[i, j] = Math.Round(r[i, j], 4);
            return r;
        }

        private static string G(double v) => v.ToString();

        /// <summary>The console text of ExecuteBranchAndBound (:1006-1233) for IP k alone, from the records a narrated
        /// run kept.  Throws where the IP kept fewer tableaux or trace quads than it made, or hit a child pivot limit:
        /// the text of a search has no gaps.  (`failed: {e}` (:1147 / :1207) carries the exception's message, no stack trace.)</summary>
        public string Narration(int k) => NarrationCore(k, null, null);

        /// <summary>DisplayTableau (:623-640) of every kept child tableau and of every incumbent's tableau, written on the
        /// device (DESIGN.md section 26): IP k's blocks start at firstBlock[k], one per kept tableau in record-id order,
        /// then the incumbent's.  The text does not depend on the batch staying as it is.</summary>
        public DeviceText FormatNarration(out long[] firstBlock)
        {
            firstBlock = new long[Count + 1];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_text(bb, firstBlock, out IntPtr text), "lpr_bb_batch_narrate_text");
            return new DeviceText(text);
        }

        /// <summary>Narration(k) with every displayed tableau taken from FormatNarration's blocks: no cell is rounded or
        /// formatted on the host.</summary>
        public string NarrationText(int k, DeviceText text, long[] firstBlock) => NarrationCore(k, text, firstBlock);

        private string NarrationCore(int k, DeviceText text, long[] firstBlock)
        {
            var made = new long[Count]; var kept = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_info(bb, null, made, kept, null), "lpr_bb_batch_narrate_info");
            if (kept[k] < made[k]) throw new InvalidOperationException($"IP {k} made {made[k]} doubles of child tableaux and keeps {kept[k]}");
            if (Status[k] == (int)LprStatus.PivotLimit) throw new InvalidOperationException($"IP {k} ended with LPR_PIVOT_LIMIT");
            var piv = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_result_read(bb, null, null, null, null, null, piv, null), "lpr_bb_batch_result_read");
            var trace = Trace(k, (int)Math.Max(1, piv[k]));
            if (trace.Count < piv[k]) throw new InvalidOperationException($"IP {k} made {piv[k]} trace quads and keeps {trace.Count}");
            var recs = Records(k);
            int n = nvars[k], cap = 1 + 2 * nodeCap;
            var off = new long[cap]; var nt = new int[cap];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_children_read(bb, k, off, nt, cap, out _), "lpr_bb_batch_narrate_children_read");
            var fl = new int[nodeCap]; var zs = new double[nodeCap]; var vals = new double[Math.Max(1, nodeCap * n)];
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_pops_read(bb, k, fl, zs, vals, nodeCap, out long pops), "lpr_bb_batch_narrate_pops_read");
            var ids = PopOrder(k);
            var flat = new double[text == null ? Math.Max(1, kept[k]) : 1];
            if (text == null && kept[k] > 0) NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_tableaux_read(bb, k, 0, kept[k], flat), "lpr_bb_batch_narrate_tableaux_read");
            int rootRows = this.rootRows[k], rootCols = this.rootCols[k];
            var sb = new System.Text.StringBuilder();
            Action<string> wl = s => sb.Append(s).Append(Environment.NewLine);
            Action<double[,], string> display = (t, caption) =>                 // DisplayTableau :623-640
            {
                if (t == null || t.Length == 0) wl($"{caption} (empty)");
                else wl(TableIterationFormater.Format(Rounded(t), n, caption));
            };
            var firstOf = new long[recs.Count + 1];                             // blocks before record q's (kept == made here)
            for (int q = 0; q < recs.Count; q++) firstOf[q + 1] = firstOf[q] + nt[q];
            Action<long, string> body = (block, caption) => wl("\n" + caption + ":" + Environment.NewLine + text.Block(block));
            wl("Initiating Branch and Bound Algorithm");
            wl(pruning ? "Pruning: Enabled" : "Pruning: Disabled");
            wl(new string('-', 50));
            var label = new Dictionary<int, string> { [0] = "0" };
            var path = new Dictionary<int, List<string>> { [0] = new List<string>() };
            var counters = new Dictionary<string, int>();
            string optimalLabel = null; double optimalValue = double.NegativeInfinity; List<double> optimalX = null;
            for (int i = 0; i < pops; i++)
            {
                int id = ids[i]; var rec = recs[id]; string lab = label[id];
                wl($"\n--- Processing branch {lab} (Depth {rec.depth}) ---");
                if (rec.parent >= 0) wl($"Parent branch: {label[rec.parent]}");
                wl($"Constraint Path: [{string.Join(", ", path[id])}]");
                if ((fl[i] & 1) == 0) { wl($"branch {lab} pruned"); continue; }
                var sol = vals.Skip(i * n).Take(n).ToList();
                string joined = string.Join(", ", sol.Select(G));
                if ((fl[i] & 4) != 0)
                {
                    optimalValue = zs[i]; optimalX = sol; optimalLabel = lab;
                    wl($"New optimal integer solution found: [{joined}] with value {G(zs[i])}");
                }
                else if ((fl[i] & 2) != 0) wl($"Integer solution found: [{joined}] with value {G(zs[i])} (not better than current optimal)");
                var kids = Enumerable.Range(0, recs.Count).Where(q => recs[q].parent == id).ToList();
                if (kids.Count == 0) { wl($"branch {lab}: Integer solution [{joined}] with value {G(zs[i])}"); continue; }
                int var = recs[kids[0]].var;
                wl($"Branching on x{var + 1} = {G(Math.Round(sol[var], 4))}");
                if (!counters.ContainsKey(lab)) counters[lab] = 0;
                foreach (int q in kids)
                {
                    bool lower = recs[q].kind == 1; string name = lower ? "Lower" : "Upper";
                    counters[lab]++;
                    string child = lab == "0" ? (lower ? "1" : "2") : $"{lab}.{counters[lab]}";
                    var bnd = Enumerable.Range(0, n).Select(j => j == var ? 1.0 : 0.0).Concat(new[] { recs[q].bound, lower ? 0.0 : 1.0 }).ToList();
                    sb.Append($"\n{name} Branch (branch {child}): {string.Join(", ", bnd.Select(G))} ");
                    sb.Append($"x{var + 1} ").Append(lower ? "<= " : ">= ").Append($"{G(recs[q].bound)} ");
                    foreach (var t in trace.Where(t => t.node == q && t.phase < 2)) wl($"pivot @ constraint {t.row}, column {t.col + 1}");
                    if (recs[q].status == 2)
                    {
                        wl($"{name} branch (branch {counters[lab]}) failed: System.ArgumentOutOfRangeException: Index was out of range. Must be non-negative and less than the size of the collection.");
                        continue;
                    }
                    int rows = rootRows + recs[q].depth, cols = rootCols + recs[q].depth;
                    long at = off[q], blk0 = text != null ? firstBlock[k] + firstOf[q] : 0;
                    var shown = text != null ? new List<double[,]>(new double[nt[q]][,])
                                             : Enumerable.Range(0, nt[q]).Select(j => Block(flat, at + (long)j * rows * cols, rows, cols)).ToList();
                    Action<int, string> show = (j, caption) => { if (text != null) body(blk0 + j, caption); else display(shown[j], caption); };
                    if (recs[q].status == 1)
                    {
                        if (shown.Count > 0) show(0, $"branch {child}: Infeasible tableau"); else display(null, $"branch {child}: Infeasible tableau");
                        continue;
                    }
                    label[q] = child;
                    path[q] = path[id].Concat(new[] { $"x{var + 1} {(lower ? "<=" : ">=")} {G(recs[q].bound)}" }).ToList();
                    wl($"{name} branch (branch {child}) infeasible");            // (sic) :1130 / :1193
                    for (int j = 0; j + 1 < shown.Count; j++) show(j, $"branch {child} {name} branch Tableau {j + 1}");
                    if (shown.Count > 0) show(shown.Count - 1, $"branch {child} {name} branch final tableau");
                }
            }
            if (Status[k] == (int)LprStatus.BbNodeCap) wl("Potential infinite loop detected");
            wl("\n" + new string('-', 50)); wl("BRANCH AND BOUND COMPLETED"); wl(new string('-', 50));
            if (optimalX != null)
            {
                if (text != null) body(firstBlock[k + 1] - 1, $"Optimal solution tableau at branch {optimalLabel}");   // the IP's last block
                else
                {
                    NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_best_read(bb, k, null, out int br, out int bc), "lpr_bb_batch_narrate_best_read");
                    var best = new double[br * bc];
                    NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_narrate_best_read(bb, k, best, out br, out bc), "lpr_bb_batch_narrate_best_read");
                    display(Block(best, 0, br, bc), $"Optimal solution tableau at branch {optimalLabel}");
                }
                wl($"Optimal branch: {optimalLabel}");
                wl($"Optimal integer solution: [{string.Join(", ", optimalX.Select(G))}]");
                wl($"Optimal value: {G(optimalValue)}");
            }
            else wl("No integer solution found");
            wl($"Total branchs processed: {pops}");
            return sb.ToString();
        }

        public void Dispose() { if (bb != IntPtr.Zero) { NativeMethods.ThrowIfError(NativeMethods.lpr_bb_batch_destroy(bb), "lpr_bb_batch_destroy"); bb = IntPtr.Zero; } }
    }

    /// <summary>
    /// Many CuttingPlaneSolver.CuttingPlaneSolution runs in one device call (lpr_cut_batch_*).  Narrate() runs the
    /// batch twice on two handles -- the first counts what every item makes, the second keeps it -- and Narration(k)
    /// is what CuttingPlaneSolution writes to the console for item k (CuttingPlaneSolver.cs:47-54, 64-229 with the
    /// printSteps text of DualSimplex.cs:14-114 and PrimalSimplexSolver2.cs:46-97), formatted from the events and
    /// tableaux the kernel stored.  The single-tableau path (lpr_cutting_plane) pivots on the cut in the call that
    /// appends it and cannot show the cut row: a one-item batch serves that caller.
    /// </summary>
    public class CuttingPlaneBatch : IDisposable
    {
        private IntPtr cb;                               // lpr_cut_batch*, the keeping handle after Narrate()
        private readonly int[] rows0, cols;
        private readonly double[] flat;
        private readonly int maxCuts;
        private long[] evMade, dMade, dKept, dataOff;
        private int evCap;
        private int[] quads;
        private double[] data;
        public int Count { get; }
        public int[] ExitCode { get; private set; }

        /// <summary>objectiveRow + constraintRows per item (:64-70), as row 0 and rows 1.. of each tableau.</summary>
        public CuttingPlaneBatch(List<double[,]> tableaux, int maxCuts = 0)
        {
            Count = tableaux.Count; this.maxCuts = maxCuts;
            rows0 = new int[Count]; cols = new int[Count];
            var f = new List<double>();
            for (int k = 0; k < Count; k++)
            {
                rows0[k] = tableaux[k].GetLength(0); cols[k] = tableaux[k].GetLength(1);
                foreach (var v in tableaux[k]) f.Add(v);                        // row-major
            }
            flat = f.ToArray();
        }

        private IntPtr Create()
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_create(Engine.Handle, Count, rows0, cols, flat, maxCuts, 0, out IntPtr h),
                "lpr_cut_batch_create");
            return h;
        }

        private static void RunOnce(IntPtr h)
        {
            var opts = new LprCutBatchOpts();
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_run(h, ref opts, out _), "lpr_cut_batch_run");
        }

        /// <summary>CuttingPlaneSolution for every item, keeping what its console text needs.</summary>
        public void Narrate()
        {
            Dispose();
            evMade = new long[Count]; dMade = new long[Count]; dKept = new long[Count]; dataOff = new long[Count];
            IntPtr counting = Create();
            try
            {
                NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_narrate_reserve(counting, new long[Count], 1), "lpr_cut_batch_narrate_reserve");
                RunOnce(counting);
                NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_narrate_info(counting, evMade, dMade, null, null), "lpr_cut_batch_narrate_info");
            }
            finally { NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_destroy(counting), "lpr_cut_batch_destroy"); }
            cb = Create();
            evCap = (int)Math.Max(1, evMade.Max());
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_narrate_reserve(cb, dMade, evCap), "lpr_cut_batch_narrate_reserve");
            RunOnce(cb);
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_narrate_info(cb, evMade, dMade, dKept, dataOff), "lpr_cut_batch_narrate_info");
            quads = new int[4L * Count * evCap]; data = new double[Math.Max(1, dMade.Sum())];
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_narrate_read_all(cb, quads, (long)Count * evCap, data, dMade.Sum()), "lpr_cut_batch_narrate_read_all");
            ExitCode = new int[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_result_read(cb, ExitCode, null, null, null), "lpr_cut_batch_result_read");
        }

        /// <summary>Item k's events (kind, a, b, rows_now), read on their own (Narrate() reads all of them at once).</summary>
        public int[] Events(int k)
        {
            var q = new int[4 * evCap];
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_narrate_events_read(cb, k, q, evCap, out long n), "lpr_cut_batch_narrate_events_read");
            return q.Take(4 * (int)Math.Min(n, evCap)).ToArray();
        }

        /// <summary>n doubles of item k's data blocks from `first`, read on their own.</summary>
        public double[] Data(int k, long first, long n)
        {
            var d = new double[Math.Max(1, n)];
            NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_narrate_data_read(cb, k, first, n, d), "lpr_cut_batch_narrate_data_read");
            return d;
        }

        private static string H4(double v) => v.ToString("0.####", System.Globalization.CultureInfo.InvariantCulture);

        /// <summary>The console text of CuttingPlaneSolution for item k.  Throws where the item stopped at the cut
        /// limit, on an escaped exception or kept less than it made: the reference has no text for those.</summary>
        public string Narration(int k)
        {
            if (evMade[k] > evCap || dKept[k] < dMade[k]) throw new InvalidOperationException($"item {k} kept less than it made");
            int C = cols[k], R = rows0[k];
            long at = dataOff[k];
            var T = new List<double[]>();
            Func<int, double[]> take = n => { var r = new double[n]; Array.Copy(data, at, r, 0, n); at += n; return r; };
            Action<int> load = rows => { T.Clear(); for (int i = 0; i < rows; i++) T.Add(take(C)); };
            load(R);
            var sb = new StringBuilder();
            Action<string> wl = s => sb.Append(s).Append(Environment.NewLine);
            Action<string> print = title =>                                     // CuttingPlaneSolver.PrintTableau :47-54
            {
                wl(title);
                wl("z:  " + string.Join("\t", T[0].Select(H4)));
                for (int i = 1; i < T.Count; i++) wl($"r{i}: " + string.Join("\t", T[i].Select(H4)));
                wl("");
            };
            Func<double[,]> table = () => { var t = new double[T.Count, C]; for (int i = 0; i < T.Count; i++) for (int j = 0; j < C; j++) t[i, j] = T[i][j]; return t; };
            Action dualTab = () => wl(TableIterationFormater.Format(table(), C - 1 - (T.Count - 1), "Dual Simplex Tableau"));   // DualSimplex.cs:193-207, 228-234
            Action primalTab = () =>                                            // PrimalSimplexSolver2.cs:184-189
            {
                wl("OBJ: " + string.Join("\t", T[0].Select(H4)));
                for (int i = 1; i < T.Count; i++) wl($"r{i}: " + string.Join("\t", T[i].Select(H4)));
            };
            bool fresh = true; int solver = 0, iter = 0;
            for (long e = 0; e < evMade[k]; e++)
            {
                long q = 4 * ((long)k * evCap + e);
                int kind = quads[q], a = quads[q + 1], b = quads[q + 2], rowsNow = quads[q + 3];
                switch (kind)
                {
                    case 0: fresh = true; break;                                // CALL
                    case 1:                                                     // LEVEL
                        if (!fresh) wl("Objective optimal but RHS has fractional values → adding another Gomory cut...");   // :219
                        fresh = false; print("Initial tableau:"); break;        // :74
                    case 2: T.Add(take(C)); break;                              // CUT :110
                    case 3:                                                     // SOLVE_BEGIN :188 / :198
                        solver = a; iter = 0;
                        wl(a == 0 ? "Negative RHS detected → running Dual Simplex..." : "Negative reduced cost detected → running Primal Simplex...");
                        break;
                    case 10:                                                    // the pivot on the cut :141-180
                        print($"Before pivot on cut: row {a + 1}, col {b + 1}"); load(rowsNow); print($"After pivot on cut: row {a + 1}, col {b + 1}"); break;
                    case 8:                                                     // DualSimplex.cs:91-105
                    {
                        int n = C - 1 - (T.Count - 1);
                        wl($"\nIteration {++iter}: pivot @ constraint {a + 1}, column {(b < n ? $"x{b + 1}" : $"t{b - n + 1}")}");
                        dualTab(); load(rowsNow); wl("After pivot:"); dualTab(); break;
                    }
                    case 9:                                                     // PrimalSimplexSolver2.cs:73-88
                        wl($"\nIter {++iter}: pivot @ row {a}, col {b}"); primalTab(); load(rowsNow); wl("After pivot:"); primalTab(); break;
                    case 4:                                                     // SOLVE_END
                        if (b != 0 || a == 3) throw new InvalidOperationException($"item {k}: an inner solve stopped where the reference cannot");
                        if (solver == 0)
                        {
                            wl(a == 0 ? "Dual phase complete: all RHS >= 0." : a == 2 ? "Infeasible: pivot row has no negative coefficients with non-zero ratios." : "Max iterations reached.");
                            if (a == 0) print("After Dual Simplex:"); else wl("Dual Simplex failed (infeasible or max iters).");   // :191-192
                        }
                        else
                        {
                            wl(a == 0 ? "Optimal reached." : a == 1 ? "Unbounded: no valid leaving row." : "Max iterations reached.");
                            print("After Primal Simplex:");                     // :211
                        }
                        break;
                    case 5:                                                     // EXIT
                        if (a == 0) wl("Displayed the Optimal Tableau.");        // :224
                        else if (a == 1) wl("All RHS are integers. No Gomory cut needed.");   // :89
                        else if (a == 2) wl("No valid pivot column on the cut (need a negative cut coeff with non-zero obj coeff).");   // :136
                        else if (a == 3) { print($"Before pivot on cut: row {rowsNow - 1}, col {b + 1}"); wl("Pivot too small/zero."); }   // :148
                        else if (a == 5) wl("Cutting-plane step finished (further steps may be required).");   // :228
                        else if (a != 4) throw new InvalidOperationException($"item {k} ended at exit {a}: the reference has no text for it");
                        break;
                }
            }
            return sb.ToString();
        }

        public void Dispose() { if (cb != IntPtr.Zero) { NativeMethods.ThrowIfError(NativeMethods.lpr_cut_batch_destroy(cb), "lpr_cut_batch_destroy"); cb = IntPtr.Zero; } }
    }

    public class RevisedPrimalSimplexSolver : IDisposable
    {
        private readonly int n, m;
        private readonly bool isMin;   // the reference's `isMin` field (:29), only printed
        private IntPtr solver;
        public List<string> IterationSnapshots { get; private set; } = new List<string>();
        public double FinalZ { get; private set; }
        public List<double> SolutionVector { get; private set; } = new List<double>();

        public RevisedPrimalSimplexSolver(List<double> objective, List<IOConstraint> constraints, bool isMinimization)
        {
            if (objective == null || objective.Count == 0) throw new ArgumentException("Objective cannot be null or empty.");
            if (constraints == null || constraints.Count == 0) throw new ArgumentException("Constraints cannot be null or empty.");
            n = objective.Count; m = constraints.Count; isMin = isMinimization;
            var A = new double[m, n];
            var b = new double[m];
            for (int i = 0; i < m; i++)
            {
                if (constraints[i].Coefficients.Count != n)
                    throw new ArgumentException($"Constraint {i + 1} has incorrect number of coefficients.");
                for (int j = 0; j < n; j++) A[i, j] = constraints[i].Coefficients[j];
                b[i] = constraints[i].RHS;
            }
            NativeMethods.ThrowIfError(NativeMethods.lpr_revised_create(Engine.Handle, n, m, objective.ToArray(), A, n, b,
                isMinimization ? 1 : 0, out solver), "lpr_revised_create");
        }

        /// <summary>Above this many table entries per snapshot none are kept (the reference would
        /// write megabytes of text per pivot); set before Solve() to force either way.</summary>
        public bool KeepSnapshots { get; set; }

        public void Solve()
        {
            int status;
            if (KeepSnapshots || (long)m * (n + m + 1) <= 4096)
            {
                // one pass of the reference's while-loop per call; after every pivot and at the
                // optimum the numbers of CaptureSnapshot (:294-387) are read back and formatted by
                // FormatSnapshot below
                int iteration = 0;
                while (true)
                {
                    NativeMethods.ThrowIfError(NativeMethods.lpr_revised_step(solver, out var info), "lpr_revised_step");
                    status = info.status;
                    if (status != (int)LprStatus.PivotLimit && status != (int)LprStatus.Optimal) break;
                    double[] y = new double[m], rc = new double[n + m], u = new double[m], ratios = new double[m], xB = new double[m];
                    int[] basisPre = new int[m];
                    NativeMethods.ThrowIfError(NativeMethods.lpr_revised_snapshot_read(solver, y, rc, u, ratios, basisPre, xB), "lpr_revised_snapshot_read");
                    var binvA = new double[m, n]; var binv = new double[m, m];
                    NativeMethods.ThrowIfError(NativeMethods.lpr_revised_binv_a_exact(solver, binvA), "lpr_revised_binv_a_exact");
                    NativeMethods.ThrowIfError(NativeMethods.lpr_revised_binv_read(solver, binv), "lpr_revised_binv_read");
                    bool optimal = status == (int)LprStatus.Optimal;
                    if (optimal) { u = new double[m]; for (int i = 0; i < m; i++) ratios[i] = double.PositiveInfinity; basisPre = BasicVariables.ToArray(); }
                    IterationSnapshots.Add(FormatSnapshot(n, m, isMin, BasicVariables, optimal ? "Optimal" : $"Iteration {++iteration}", xB, y,
                        rc.Take(n).ToArray(), rc.Skip(n).ToArray(), info.entering, info.entering_rc_pre, u, ratios,
                        basisPre.ToList(), info.leaving_row, info.leaving_var, info.z_working, info.z_original, binvA, binv));
                    if (optimal) break;
                }
            }
            else
            {
                var opts = new LprSolveOpts();
                NativeMethods.ThrowIfError(NativeMethods.lpr_revised_solve(solver, ref opts, out var res), "lpr_revised_solve");
                status = res.status;
            }
            switch ((LprStatus)status)
            {
                case LprStatus.Optimal:
                    var x = new double[n];
                    NativeMethods.lpr_revised_solution(solver, x, out double z);
                    SolutionVector = x.ToList(); FinalZ = z; break;
                // the reference's `throw new Exception(...)` texts (RevisedPrimalSimplexSolver.cs:91,179,183,267)
                case LprStatus.InfeasibleBasis: throw new Exception("Infeasible basis (negative basic value).");
                case LprStatus.Unbounded: throw new Exception("Unbounded problem (no positive component in direction).");
                case LprStatus.EnteringAlreadyBasic: throw new Exception("Internal error: entering variable is already basic.");
                case LprStatus.PivotTooSmall: throw new Exception("Pivot too small.");
            }
        }

        public List<int> BasicVariables { get { var b = new int[m]; NativeMethods.lpr_revised_basis_read(solver, b); return b.ToList(); } }

        // The text block of the reference's CaptureSnapshot (RevisedPrimalSimplexSolver.cs:294-387), built from the
        // numbers the engine hands back (its two matrix products arrive as binvA / binv).  Same layout as the Python
        // mirror (lpr_381_group_v22_amd/revised_primal_simplex_solver.py), which tests/test_revised_gpu.py compares
        // byte for byte with an independent restatement.  NumFormat.N3 stays the reference's own (:451-466).
        private static string Label(int idx, int nVars) => idx < nVars ? $"x{idx + 1}" : $"S{idx - nVars + 1}";   // VarLabel :289-292

        // Static: RevisedSimplexBatch formats the records of a traced batch with it (`post` = basicVariables after the pivot).
        internal static string FormatSnapshot(int n, int m, bool isMin, List<int> post, string title, double[] xB, double[] y, double[] rcX_post, double[] rcS_post,
            int enteringIdx, double enteringRC_pre, double[] u_pre, double[] ratios_pre, List<int> basisForRatios_Pre,
            int leavingRow, int leavingVarIndex_Pre, double zWorking, double zOriginal, double[,] BInvA, double[,] BInv)
        {
            Func<IEnumerable<double>, string> tabbed = v => string.Join("\t", v.Select(NumFormat.N3));
            var sb = new System.Text.StringBuilder();
            sb.AppendLine(title);
            sb.AppendLine("Current Tableau (Revised Simplex)");
            sb.AppendLine("Problem type: " + (isMin ? "MIN (solving by MAX of -c)" : "MAX"));
            sb.AppendLine();
            sb.AppendLine("Dual prices (y = c_B^T B^{-1}):");
            sb.AppendLine(tabbed(y));
            sb.AppendLine();
            sb.AppendLine("Reduced costs:");
            sb.AppendLine("  x: " + tabbed(rcX_post));
            sb.AppendLine("  s: " + tabbed(rcS_post));
            sb.AppendLine();
            if (enteringIdx >= 0)
            {
                string entering = Label(enteringIdx, n);
                sb.AppendLine($"Entering variable (chosen pre-pivot): {entering}  (reduced cost pre = {NumFormat.N3(enteringRC_pre)})");
                sb.AppendLine("Direction u = B^{-1} a_enter (pre-pivot):");
                sb.AppendLine(tabbed(u_pre));
                sb.AppendLine();
                sb.AppendLine("Ratio test (xB_i / u_i; \u221E if u_i \u2264 0)  [labels = pre-pivot basis]:");
                for (int i = 0; i < m; i++)
                    sb.AppendLine(Label(basisForRatios_Pre[i], n) + ": " +
                                  (double.IsPositiveInfinity(ratios_pre[i]) ? "\u221E" : NumFormat.N3(ratios_pre[i])));
                if (leavingRow >= 0 && leavingVarIndex_Pre >= 0)
                {
                    sb.AppendLine($"Pivot (pre\u2192post): {Label(leavingVarIndex_Pre, n)}  \u2192  {entering}    (pivot = {NumFormat.N3(u_pre[leavingRow])})");
                    sb.AppendLine();
                }
            }
            sb.AppendLine("Working objective Z_working (maxified): " + NumFormat.N3(zWorking));
            sb.AppendLine($"Original objective Z_original ({(isMin ? "MIN" : "MAX")}): {NumFormat.N3(zOriginal)}");
            sb.AppendLine();
            sb.Append("Table\t");
            for (int j = 0; j < n; j++) sb.Append($"x{j + 1}\t");
            for (int j = 0; j < m; j++) sb.Append($"S{j + 1}\t");
            sb.AppendLine("RHS");
            sb.Append("Z~\t");
            foreach (double v in rcX_post) sb.Append(NumFormat.N3(v) + "\t");
            foreach (double v in rcS_post) sb.Append(NumFormat.N3(v) + "\t");
            sb.AppendLine(NumFormat.N3(zWorking));
            for (int i = 0; i < m; i++)
            {
                sb.Append(Label(post[i], n) + "\t");
                for (int j = 0; j < n; j++) sb.Append(NumFormat.N3(BInvA[i, j]) + "\t");
                for (int j = 0; j < m; j++) sb.Append(NumFormat.N3(BInv[i, j]) + "\t");
                sb.AppendLine(NumFormat.N3(xB[i]));
            }
            sb.AppendLine("Basic Variables: " + string.Join(", ", post.Select(v => Label(v, n))));
            return sb.ToString();
        }

        /// <summary>B^-1 * A of CaptureSnapshot (:360) on the fp64 matrix cores.</summary>
        public double[,] BInverseTimesA() { var p = new double[m, n]; NativeMethods.lpr_revised_binv_a(solver, p, out _); return p; }

        public void Dispose() { if (solver != IntPtr.Zero) { NativeMethods.lpr_revised_destroy(solver); solver = IntPtr.Zero; } }
    }
}

namespace LPR_381_Group_V22.IntegerProgramming
{
    using LPR_381_Group_V22.Simplex;

    public static class BranchAndBoundAdapter
    {
        public static (List<double> x, double z) SolveFromPrimal(PrimalSimplexSolver primal, bool enablePruning = false, bool isMin = false)
        {
            if (primal.FinalTableau == null)
                throw new InvalidOperationException("Primal simplex has not been solved yet.");   // BranchAndBoundAdapter.cs:11-14
            int nvars = primal.SolutionVector?.Count ?? Math.Max(1, primal.FinalTableau.GetLength(1) - 1);   // :20
            // the FinalTableau is still resident on the device: no double[,] -> List<List<double>> conversion
            NativeMethods.ThrowIfError(NativeMethods.lpr_bb_create_from_tableau(primal.Tableau, nvars, 20, out IntPtr bb), "lpr_bb_create_from_tableau");
            try
            {
                var opts = new LprBbOpts { enable_pruning = enablePruning ? 1 : 0, node_cap = 20 };   // :1038
                var x = new double[Math.Max(1, nvars)];
                NativeMethods.ThrowIfError(NativeMethods.lpr_bb_run(bb, ref opts, x, out var res), "lpr_bb_run");
                if (res.status == (int)LprStatus.BbNodeCap) Console.WriteLine("Potential infinite loop detected");
                return res.found != 0 ? (x.Take(nvars).ToList(), res.z) : (new List<double>(), double.NegativeInfinity);   // :23
            }
            finally { NativeMethods.lpr_bb_destroy(bb); }
        }
    }
}

namespace LPR_381_Group_V22.IntegerProgramming
{
    /// <summary>An item of GetSelectedItemsOriginal() (Program.cs:455-461): original 0-based index, value, weight.</summary>
    public sealed class KnapsackItem
    {
        public int Id { get; }
        public double Value { get; }
        public double Weight { get; }
        public KnapsackItem(int id, double value, double weight) { Id = id; Value = value; Weight = weight; }
    }

    /// <summary>
    /// Menu option 5 (Program.cs:430-470): the level-synchronous knapsack branch-and-bound of DESIGN.md section 11 on the
    /// device.  Inputs: integral weights 1..2^31-1, values 0..2^31-1, capacity >= 0, 1..8192 items.
    /// </summary>
    public class KnapsackBranchBoundSimplex : IDisposable
    {
        private IntPtr h;
        private readonly double[] weights, values;
        public long NodeCap = 0;      // 0: 2^22 evaluated nodes
        public int Narrate = -1;      // node records for PrintIterations: -1 auto (4096 when n <= 64), 0 none
        public int Status { get; private set; }
        public long Evaluated { get; private set; }
        public int Levels { get; private set; }

        public KnapsackBranchBoundSimplex(int capacity, double[] weights, double[] values)
        {
            this.weights = (double[])weights.Clone();
            this.values = (double[])values.Clone();
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_bb_create(Engine.Handle, capacity, this.weights, this.values,
                this.weights.Length, out h), "lpr_knap_bb_create");
        }

        public double Solve()
        {
            var opts = new LprKnapBbOpts { node_cap = NodeCap, narrate = Narrate };
            Status = NativeMethods.lpr_knap_bb_solve(h, ref opts, out var res);
            NativeMethods.ThrowIfError(Status, "lpr_knap_bb_solve");
            Evaluated = res.evaluated;
            Levels = res.levels;
            return res.z;
        }

        /// <summary>One line per node record, the same text as knapsack.py's narration_lines.</summary>
        public void PrintIterations()
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_bb_nodes_read(h, null, null, null, null, null, null, 0, out long m), "lpr_knap_bb_nodes_read");
            int n = (int)m, c = Math.Max(1, n);
            var par = new int[c]; var br = new int[c]; var st = new int[c]; var kk = new int[c];
            var bd = new double[c]; var V = new long[c];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_bb_nodes_read(h, par, br, st, bd, kk, V, m, out m), "lpr_knap_bb_nodes_read");
            string[] statusText = { "fractional", "fractional, pruned", "integral", "infeasible" };
            var label = new string[c];
            var fixedText = new string[c];
            for (int r = 0; r < n; r++)
            {
                if (par[r] < 0) { label[r] = "0"; fixedText[r] = ""; }
                else
                {
                    label[r] = (par[r] == 0 ? "" : label[par[r]] + ".") + (br[r] + 1);
                    string f = $"x{kk[par[r]] + 1}={br[r]}";
                    fixedText[r] = fixedText[par[r]].Length > 0 ? fixedText[par[r]] + " " + f : f;
                }
                string tail = st[r] == 3 ? "bound = -; k = -; V = -"
                    : $"bound = {bd[r]}; k = {(kk[r] >= 0 ? "x" + (kk[r] + 1) : "-")}; V = {V[r]}";
                Console.WriteLine($"Node {label[r]}: fixed {(fixedText[r].Length > 0 ? fixedText[r] : "none")}; {statusText[st[r]]}; {tail}");
            }
            if (Evaluated > n)
                Console.WriteLine($"({Evaluated - n} of {Evaluated} nodes in {Levels} levels not recorded)");
        }

        public List<KnapsackItem> GetSelectedItemsOriginal()
        {
            var ids = new int[Math.Max(1, weights.Length)];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_bb_selected_read(h, ids, out int count), "lpr_knap_bb_selected_read");
            return ids.Take(count).Select(i => new KnapsackItem(i, values[i], weights[i])).ToList();
        }

        public void Dispose() { if (h != IntPtr.Zero) { NativeMethods.lpr_knap_bb_destroy(h); h = IntPtr.Zero; } }
    }

    /// <summary>The 0/1 DP cross-check of Program.cs:465 on the device (replaces the empty KnapsackBranchBoundSolver.cs).</summary>
    public static class KnapsackBranchBoundSolver
    {
        public static double Solve(int capacity, int[] weights, int[] values)
        {
            var opts = new LprKnapDpOpts();
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_dp(Engine.Handle, capacity, weights, values, weights.Length, ref opts, out long best), "lpr_knap_dp");
            return best;
        }
    }

    /// <summary>
    /// Option 5 for many instances per device call (DESIGN.md section 16): the branch-and-bound of every instance in one
    /// Solve(), the DP of every instance in one DP().  Instance k gets what KnapsackBranchBoundSimplex gives at the same NodeCap.
    /// </summary>
    public class KnapsackBatch : IDisposable
    {
        private IntPtr h;
        private readonly int[] n, off;
        public int Count => n.Length;
        public int[] Status { get; private set; }
        public double[] Z { get; private set; }
        public long[] Evaluated { get; private set; }

        /// <param name="nodeCap">evaluated nodes per instance; null or an entry &lt;= 0: 1024</param>
        /// <param name="narrate">node records kept per instance</param>
        public KnapsackBatch(long[] capacities, double[][] weights, double[][] values, long[] nodeCap = null, int narrate = 0)
        {
            n = weights.Select(w => w.Length).ToArray();
            off = new int[n.Length];
            for (int k = 1; k < n.Length; k++) off[k] = off[k - 1] + n[k - 1];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_create(Engine.Handle, n.Length, capacities, n,
                weights.SelectMany(w => w).ToArray(), values.SelectMany(v => v).ToArray(), nodeCap, narrate, out h), "lpr_knap_batch_create");
        }

        public void Solve(int chunk = 0, int variant = 0)
        {
            var opts = new LprKnapBatchOpts { chunk = chunk, variant = variant };
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_solve(h, ref opts, out _), "lpr_knap_batch_solve");
            Status = new int[Count]; Z = new double[Count]; Evaluated = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_result_read(h, Status, null, Z, Evaluated, null, null), "lpr_knap_batch_result_read");
        }

        public int[] Rank(int k)
        {
            var all = new int[n.Sum()];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_rank_read(h, all), "lpr_knap_batch_rank_read");
            return all.Skip(off[k]).Take(n[k]).ToArray();
        }

        /// <summary>The incumbent's items of every instance, ascending original indices.</summary>
        public int[][] SelectedIds()
        {
            var ids = new int[n.Sum()];
            var counts = new int[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_selected_read(h, ids, counts), "lpr_knap_batch_selected_read");
            return Enumerable.Range(0, Count).Select(k => ids.Skip(off[k]).Take(counts[k]).ToArray()).ToArray();
        }

        /// <summary>Records kept of instance k: (parent, branch, status, bound, k as an original index, V).</summary>
        public (int[] parent, int[] branch, int[] status, double[] bound, int[] kitem, long[] value) Nodes(int k)
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_nodes_read(h, k, null, null, null, null, null, null, 0, out long m), "lpr_knap_batch_nodes_read");
            int[] par = new int[m], br = new int[m], st = new int[m], kk = new int[m];
            double[] bd = new double[m];
            long[] V = new long[m];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_nodes_read(h, k, par, br, st, bd, kk, V, m, out m), "lpr_knap_batch_nodes_read");
            return (par, br, st, bd, kk, V);
        }

        /// <summary>dp[capacity] of every instance; -1 where which[k] is 0.</summary>
        public long[] DP(byte[] which = null)
        {
            var best = new long[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_dp(h, which, best), "lpr_knap_batch_dp");
            return best;
        }

        public void Dispose() { if (h != IntPtr.Zero) { NativeMethods.ThrowIfError(NativeMethods.lpr_knap_batch_destroy(h), "lpr_knap_batch_destroy"); h = IntPtr.Zero; } }
    }
}

namespace LPR_381_Group_V22.SensitivityAnalysis
{
    using LPR_381_Group_V22.Simplex;

    /// <summary>
    /// The numeric half of SensitivityAnalyzer (SensitivityAnalyzer.cs) on the device.  The reference class keeps its
    /// prompts / Console output and replaces its double[,] tableau + Pivot / ReOptimize / DualSimplexIfNeeded /
    /// RebuildBasicsFromTableau by calls on this handle.  Uncompiled here (no .NET toolchain in the build image).
    /// </summary>
    internal sealed class GpuSensitivity : IDisposable
    {
        private IntPtr h;

        // Program.cs:147-151 -- the solved tableau is copied device to device
        internal GpuSensitivity(PrimalSimplexSolver primal, int numDecisionVariables)
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_sens_create_from_tableau(primal.Tableau, numDecisionVariables, out h), "lpr_sens_create_from_tableau");
        }

        // SensitivityAnalyzer(double[,], List<double>, double, List<int>) :22-39 (basicVariables is rebuilt by :35)
        internal GpuSensitivity(double[,] finalTableau, List<double> solution, double zValue)
        {
            NativeMethods.ThrowIfError(NativeMethods.lpr_sens_create(Engine.Handle, finalTableau, finalTableau.GetLength(0), finalTableau.GetLength(1),
                solution.ToArray(), solution.Count, zValue, out h), "lpr_sens_create");
        }

        private static void Throw(int outcome)
        {
            switch (outcome)
            {
                case 1: throw new InvalidOperationException("Unbounded during re-optimization.");            // :151
                case 2: throw new InvalidOperationException("Infeasible after RHS change (dual simplex).");  // :197
                case 3: throw new InvalidOperationException("Zero pivot encountered.");                      // :101
                case 5: throw new InvalidOperationException("Re-optimization exceeded iteration limit.");    // :126 / :183
                case 9: throw new IndexOutOfRangeException();                                                // tech[basicVars[pos]] with -1, :642
            }
        }

        /// <returns>false when the C# would have printed "Invalid ..." and returned</returns>
        internal bool ChangeNonBasicReducedCost(int index, double newCbar)
        { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_change_nonbasic_cbar(h, index, newCbar, out int oc), "lpr_sens_change_nonbasic_cbar"); Throw(oc); return oc == 0; }
        internal bool ChangeBasic(int col, double delta)
        { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_change_basic(h, col, delta, out int oc), "lpr_sens_change_basic"); Throw(oc); return oc == 0; }
        /// <returns>0 re-solved, 8 rolled back (the caller prints the C#'s message :467-468), -1 invalid index</returns>
        internal int ChangeRHS(int k, double newB)
        { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_change_rhs(h, k, newB, out int oc), "lpr_sens_change_rhs"); return oc; }
        internal bool ChangeNonBasicColumn(int row, int col, double newVal)
        { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_change_nonbasic_column(h, row, col, newVal, out int oc), "lpr_sens_change_nonbasic_column"); Throw(oc); return oc == 0; }
        internal void AddNewActivity(double cNew, double[] aNew)
        { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_add_activity(h, cNew, aNew, aNew.Length, out int oc), "lpr_sens_add_activity"); Throw(oc); }
        internal void AddNewConstraint(double[] tech, double rhs)
        { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_add_constraint(h, tech, tech.Length, rhs, out int oc), "lpr_sens_add_constraint"); Throw(oc); }

        internal int GetBasicRow(int col) { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_basic_row(h, col, out int r), "lpr_sens_basic_row"); return r; }   // :69-77

        internal double[,] CurrentTableau   // :727
        {
            get
            {
                NativeMethods.lpr_sens_shape(h, out int R, out int C, out _, out _, out _, out _);
                var t = new double[R, C];
                NativeMethods.ThrowIfError(NativeMethods.lpr_sens_read(h, t, null, null), "lpr_sens_read");
                return t;
            }
        }
        internal double CurrentZ { get { NativeMethods.lpr_sens_shape(h, out _, out _, out _, out _, out double z, out _); return z; } }   // :728
        internal List<double> CurrentSolutionVector   // :729
        {
            get
            {
                NativeMethods.lpr_sens_shape(h, out _, out _, out int ns, out _, out _, out _);
                var x = new double[Math.Max(1, ns)];
                NativeMethods.ThrowIfError(NativeMethods.lpr_sens_read(h, null, null, x), "lpr_sens_read");
                return x.Take(ns).ToList();
            }
        }
        internal double[] Row(int i) { NativeMethods.lpr_sens_shape(h, out _, out int C, out _, out _, out _, out _); var r = new double[C]; NativeMethods.ThrowIfError(NativeMethods.lpr_sens_read_block(h, i, 1, 0, C, r), "lpr_sens_read_block"); return r; }
        internal double[] Column(int j) { NativeMethods.lpr_sens_shape(h, out int R, out _, out _, out _, out _, out _); var c = new double[R]; NativeMethods.ThrowIfError(NativeMethods.lpr_sens_read_block(h, 0, R, j, 1, c), "lpr_sens_read_block"); return c; }
        // A-tilde^T y of RecoverObjectiveC / PerformDuality (:236-245, :690-694), summed in the C#'s order on the device
        internal double[] ATy(double[] y, int n) { var o = new double[Math.Max(1, n)]; NativeMethods.ThrowIfError(NativeMethods.lpr_sens_column_fold(h, y, y.Length, null, n, o), "lpr_sens_column_fold"); return o; }

        // What DisplayRangeNonBasic (:276-297), DisplayRangeBasic (:324-359), DisplayRangeRHS (:396-424) and ShadowPrices (:212-222)
        // compute, for every column and every constraint, from one read of the tableau on the device.  Kind: 0 non-basic with a range,
        // 1 non-basic at the boundary, 2 non-basic and not optimal, 3 basic, 4 basic without a basic row (:337).
        internal sealed class Ranging
        {
            public int[] Kind, VarRow;                      // per column 0 .. numCols - 2
            public double[] ReducedCost, CostLo, CostHi;
            public double[] Shadow, RhsLo, RhsHi, RhsNow;   // per constraint k at k - 1
        }
        internal Ranging RangingReport()
        {
            NativeMethods.lpr_sens_shape(h, out int R, out int C, out _, out _, out _, out _);
            var r = new Ranging
            {
                Kind = new int[C - 1], VarRow = new int[C - 1], ReducedCost = new double[C - 1], CostLo = new double[C - 1], CostHi = new double[C - 1],
                Shadow = new double[R - 1], RhsLo = new double[R - 1], RhsHi = new double[R - 1], RhsNow = new double[R - 1],
            };
            NativeMethods.ThrowIfError(NativeMethods.lpr_sens_ranging(h, r.Kind, r.VarRow, r.ReducedCost, r.CostLo, r.CostHi, r.Shadow, r.RhsLo, r.RhsHi, r.RhsNow), "lpr_sens_ranging");
            return r;
        }

        public void Dispose() { if (h != IntPtr.Zero) { NativeMethods.lpr_sens_destroy(h); h = IntPtr.Zero; } }
    }

    /// One analyzer per solved model of a PrimalSimplexBatch, each with its own script of edits (lpr_sens_batch_from_batch): what
    /// Program.cs:147-151 builds from GetFinalTableau(), SolutionVector, FinalZ and BasicVariables, for every model on the device.
    /// items[k] is the model of scenario k (null: model k); every one must be optimal.  A thin wrapper: the reads are the
    /// lpr_sens_batch_* calls of NativeMethods.
    internal sealed class GpuSensitivityModelBatch : IDisposable
    {
        private IntPtr h;
        internal readonly int Count;

        internal GpuSensitivityModelBatch(PrimalSimplexBatch primal, int[] items, int[] nedits, LprSensEdit[] edits, double[] payload, int logCap = 0)
        {
            Count = nedits.Length;
            NativeMethods.ThrowIfError(NativeMethods.lpr_sens_batch_from_batch(primal.Handle, Count, items, nedits, edits, payload,
                payload == null ? 0 : payload.LongLength, logCap, out h), "lpr_sens_batch_from_batch");
        }

        internal LprSensBatchResult Run(long maxPivots = 0)
        {
            var opts = new LprSensBatchOpts { max_pivots = maxPivots };
            NativeMethods.ThrowIfError(NativeMethods.lpr_sens_batch_run(h, ref opts, out LprSensBatchResult res), "lpr_sens_batch_run");
            return res;
        }

        /// rows[k] x cols[k] of every scenario and the maxima the bulk reads are packed by
        internal void Shapes(out int[] rows, out int[] cols, out int maxRows, out int maxCols)
        {
            rows = new int[Count]; cols = new int[Count];
            NativeMethods.ThrowIfError(NativeMethods.lpr_sens_batch_shape_read(h, rows, cols, out maxRows, out maxCols), "lpr_sens_batch_shape_read");
        }

        /// The ranging report of every scenario, scenario k in row k of each array (padded to the maxima of Shapes)
        internal GpuSensitivity.Ranging RangingReport()
        {
            Shapes(out _, out _, out int R, out int C);
            int nc = Count * (C - 1), nr = Count * (R - 1);
            var r = new GpuSensitivity.Ranging
            {
                Kind = new int[nc], VarRow = new int[nc], ReducedCost = new double[nc], CostLo = new double[nc], CostHi = new double[nc],
                Shadow = new double[nr], RhsLo = new double[nr], RhsHi = new double[nr], RhsNow = new double[nr],
            };
            NativeMethods.ThrowIfError(NativeMethods.lpr_sens_batch_ranging(h, r.Kind, r.VarRow, r.ReducedCost, r.CostLo, r.CostHi, r.Shadow, r.RhsLo, r.RhsHi, r.RhsNow), "lpr_sens_batch_ranging");
            return r;
        }

        public void Dispose() { if (h != IntPtr.Zero) { NativeMethods.ThrowIfError(NativeMethods.lpr_sens_batch_destroy(h), "lpr_sens_batch_destroy"); h = IntPtr.Zero; } }
    }
}
