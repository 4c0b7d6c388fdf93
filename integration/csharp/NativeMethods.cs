// NativeMethods.cs -- P/Invoke binding of include/lpr_engine.h for LPR_381_Group_V22.
// UNVERIFIED: no C# toolchain exists in the build image, this file has never been compiled.
// Add it (and the three Gpu*.cs wrappers) to LPR_381_Group_V22.csproj, build x64
// (<PlatformTarget>x64</PlatformTarget>: the engine is a 64-bit library) and ship liblpr_engine.so
// (Linux/.NET on ROCm) next to the executable.
using System;
using System.Runtime.InteropServices;

namespace LPR_381_Group_V22.Native
{
    internal enum LprStatus
    {
        Optimal = 0, Unbounded = 1, InfeasibleBasis = 2, PivotTooSmall = 3,
        EnteringAlreadyBasic = 4, PivotLimit = 5, BbNodeCap = 6, BbDepthCap = 7,
        BadArgument = -1, DeviceError = -2, OutOfMemory = -3
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprSolveOpts
    {
        public long max_pivots; public int time_kernels; public int batch; public int variant; public int block;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprKnapDpOpts { public int variant; public int reserved; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprKnapBbOpts { public long node_cap; public int narrate; public int reserved; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprKnapBbResult
    {
        public int status; public int found; public double z; public long evaluated; public long widest; public int levels; public int reserved;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBatchOpts { public long max_pivots; public int chunk; public int variant; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBatchResult { public int optimal, unbounded, limit, launches; public long pivots; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBbBatchOpts { public int enable_pruning, chunk, variant, max_child_pivots; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprSensEdit { public int op, a, b, reserved; public double v; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprSensBatchOpts { public long max_pivots; public int chunk; public int variant; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprSensBatchResult { public int finished, running, launches, form; public long pivots; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprKnapBatchOpts { public int chunk, variant; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprKnapBatchResult { public int finished, capped, launches, items_w, items_g, items_h; public long nodes; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprRevBatchOpts { public long max_pivots; public int chunk; public int variant; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprRevBatchResult { public int optimal, unbounded, infeasible, other, limit, launches; public long iterations; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprCutBatchOpts { public int mode, max_cuts; public long hard_cap; public int max_iters, print_steps, chunk, variant; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprCutBatchResult { public int code0, code1, code2, code3, code4, code5, code6, code7, launches, items_g, items_h, reserved; public long cuts, pivots; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBbBatchResult { public int done, node_cap, pivot_limit, launches; public long pops, pivots; }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprSolveResult
    {
        public int status; public int block; public long pivots; public long total_pivots; public double z;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprRevisedSnapshotInfo
    {
        public int status, entering, leaving_row, leaving_var;
        public double entering_rc_pre, z_working, z_original;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprRevisedResult
    {
        public int status; public int reserved; public long iterations; public long total_iterations; public double z;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBbOpts
    {
        public int enable_pruning; public int node_cap; public int reserved0; public int reserved1;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBbResult
    {
        public int status; public int found; public long processed; public int best_node; public int reserved;
        public double z; public long pivots; public long nodes_created;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBbSyncOpts
    {
        public int enable_pruning; public int max_levels; public long max_nodes;
    }

    [StructLayout(LayoutKind.Sequential)]
    internal struct LprBbSyncResult
    {
        public int status; public int found; public long processed; public long pivots;
        public int levels; public int path_len; public ulong path_bits; public double z;
    }

    // transport callbacks of lpr_comm_init_custom (a host that brings its own fabric); called on the calling thread only
    [UnmanagedFunctionPointer(CallingConvention.Cdecl)] internal delegate int LprAllReduceMaxFn(IntPtr user, IntPtr inout, int count);
    [UnmanagedFunctionPointer(CallingConvention.Cdecl)] internal delegate int LprAllGatherFn(IntPtr user, IntPtr send, IntPtr recv, int bytes);

    internal static class NativeMethods
    {
        internal const int LPR_COMM_ID_BYTES = 128;
        private const string Lib = "lpr_engine"; // liblpr_engine.so
        private const CallingConvention CC = CallingConvention.Cdecl;

        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_abi_version();
        [DllImport(Lib, CallingConvention = CC)] internal static extern IntPtr lpr_last_error();
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_engine_open(int device, out IntPtr engine);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_engine_close(IntPtr engine);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_engine_sync(IntPtr engine);
        [DllImport(Lib, CallingConvention = CC)] internal static extern ulong lpr_engine_stream(IntPtr engine);

        // ---- PrimalSimplexSolver (Simplex/PrimalSimplexSolver.cs) ----
        [DllImport(Lib, CallingConvention = CC)]
        internal static extern int lpr_tableau_from_lp(IntPtr engine, int n, int m, double[] objective, double[] A, int lda,
            int[] ncoef, sbyte[] relation, double[] rhs, int is_max, out IntPtr tableau);
        [DllImport(Lib, CallingConvention = CC)]
        internal static extern int lpr_tableau_create(IntPtr engine, int rows, int cols, double[,] rowmajor, int[] basis, out IntPtr tableau);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_tableau_destroy(IntPtr tableau);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_tableau_shape(IntPtr tableau, out int rows, out int cols, out int ld);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_primal_solve(IntPtr tableau, ref LprSolveOpts opts, out LprSolveResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_select_entering(IntPtr tableau, out int col);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_select_leaving(IntPtr tableau, int col, out int row);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_pivot(IntPtr tableau, int row, int col);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_extract_solution(IntPtr tableau, int n, double[] x, out double z);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_tableau_read(IntPtr tableau, double[,] rowmajorOut);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_basis_read(IntPtr tableau, int[] basisOut);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_pivot_log_read(IntPtr tableau, int[] rows, int[] cols, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_tableau_read_block(IntPtr tableau, int row0, int nrows, int col0, int ncols, double[] block);
        // benchmark input + kernel timing (bench.py's counterparts; no reference member)
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_tableau_synthetic(IntPtr engine, int m, int n, ulong seed, out IntPtr tableau);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_tableau_kernel_stats(IntPtr tableau, out long launches, out double totalMs, out double avgMs);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_tableau_step_stats(IntPtr tableau, out long steps, out double totalMs);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_debug_head_stamps(IntPtr tableau, ulong[] stamps, long cap, out long count);

        // ---- DualSimplexSolver (Simplex/DualSimplex.cs:14-114), PrimalSimplexSolver2 (Simplex/PrimalSimplexSolver2.cs:46-97),
        //      CuttingPlaneSolver.CuttingPlaneSolution (IntegerProgramming/CuttingPlaneSolver.cs:64-229) on a tableau handle ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_dual_solve(IntPtr tableau, int maxIters, int printSteps, long hardCap, out LprSolveResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_primal2_solve(IntPtr tableau, int maxIters, int printSteps, long hardCap, out LprSolveResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cutting_plane(IntPtr tableau, int maxCuts, long hardCap, out int exitCode, out int cuts);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_log_read(IntPtr tableau, int[] triples, long cap, out long count);

        // ---- RevisedPrimalSimplexSolver (Simplex/RevisedPrimalSimplexSolver.cs) ----
        [DllImport(Lib, CallingConvention = CC)]
        internal static extern int lpr_revised_create(IntPtr engine, int n, int m, double[] objective, double[,] A, int lda, double[] b, int is_min, out IntPtr solver);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_destroy(IntPtr solver);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_solve(IntPtr solver, ref LprSolveOpts opts, out LprRevisedResult res);
        // IterationSnapshots (RevisedPrimalSimplexSolver.cs:36, CaptureSnapshot :294-387)
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_step(IntPtr solver, out LprRevisedSnapshotInfo info);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_snapshot_read(IntPtr solver, double[] y, double[] rc, double[] u, double[] ratios, int[] basisPre, double[] xB);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_binv_a_exact(IntPtr solver, double[,] product);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_binv_read(IntPtr solver, double[,] binv);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_solution(IntPtr solver, double[] x, out double z);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_basis_read(IntPtr solver, int[] basis);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_xb_read(IntPtr solver, double[] xb);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_binv_a(IntPtr solver, double[,] product, out double ms);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_log_read(IntPtr solver, int[] rows, int[] entering, int[] leaving, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_revised_synthetic(IntPtr engine, int m, int n, ulong seed, out IntPtr solver);

        // ---- BranchAndBoundAdapter / BranchBoundSimplexSolver ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_create_from_tableau(IntPtr tableau, int nvars, int max_depth, out IntPtr bb);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_create(IntPtr engine, double[,] finalTableau, int rows, int cols, int nvars, int max_depth, out IntPtr bb);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_run(IntPtr bb, ref LprBbOpts opts, double[] x, out LprBbResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_destroy(IntPtr bb);
        // node records / pop order / pivot trace of the last lpr_bb_run (what ExecuteBranchAndBound prints per branch, :1049-1230)
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_records_read(IntPtr bb, int[] parent, int[] kind, int[] depth, int[] var, double[] bound, int[] status, double[] z, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_pop_order_read(IntPtr bb, int[] ids, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_trace_read(IntPtr bb, int[] quads, long cap, out long count);
        // building blocks: batched AddConstraint (:694-803) + DoDualSimplex (:289-468) of many children, node scoring, buffers
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_expand(IntPtr bb, int count, int[] parentIds, int[] var, double[] bound, int[] kind, int[] childIds, int[] status, int[] pivots);
        // the same + what ExecuteBranchAndBound prints about each child: pivot triples and every tableau of DoDualSimplex's list
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_expand_traced(IntPtr bb, int count, int[] parentIds, int[] var, double[] bound, int[] kind, int[] childIds, int[] status, int[] pivots, int[] trace, long traceCap, long[] traceOff, double[] tableaux, long tabCap, long[] tabOff, int[] ntab);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_node_info(IntPtr bb, int[] ids, int count, double[] z, double[] vals);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_node_read(IntPtr bb, int id, double[] tableau, out int rows, out int cols);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_release(IntPtr bb, int[] ids, int count);
        // level-synchronous, multi-GPU form (cap lifted): ONE all-reduce(MAX) per level issued by the library on RCCL
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_solve_level_sync(IntPtr bb, IntPtr comm, ref LprBbSyncOpts opts, double[] x, out LprBbSyncResult res);

        // ---- multi-GPU communicator (one process per GPU; RCCL over xGMI inside the library) ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_comm_unique_id([Out] byte[] id128);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_comm_init(IntPtr engine, int rank, int world, byte[] id128, out IntPtr comm);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_comm_init_custom(int rank, int world, LprAllReduceMaxFn allReduceMax, LprAllGatherFn allGather, IntPtr user, out IntPtr comm);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_comm_destroy(IntPtr comm);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_comm_info(IntPtr comm, out int rank, out int world, out long allReduceCalls, out long allGatherCalls);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_comm_all_reduce_max(IntPtr comm, double[] inout, int count);

        // ---- SensitivityAnalyzer (SensitivityAnalysis/SensitivityAnalyzer.cs); outcome = lpr_sens_outcome ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_create(IntPtr engine, double[,] finalTableau, int rows, int cols, double[] solution, int nsol, double z, out IntPtr sens);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_create_from_tableau(IntPtr tableau, int nDecision, out IntPtr sens);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_destroy(IntPtr sens);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_shape(IntPtr sens, out int rows, out int cols, out int nsol, out int nbasic, out double z, out long lastPivots);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_read(IntPtr sens, double[,] tableau, int[] basic, double[] solution);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_read_block(IntPtr sens, int row0, int nrows, int col0, int ncols, double[] block);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_basic_row(IntPtr sens, int col, out int row);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_log_read(IntPtr sens, int[] triples, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_column_fold(IntPtr sens, double[] w, int nw, double[] init, int ncols, double[] result);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_resolve_all(IntPtr sens, out int outcome);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_change_nonbasic_cbar(IntPtr sens, int index, double newCbar, out int outcome);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_change_basic(IntPtr sens, int col, double delta, out int outcome);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_change_rhs(IntPtr sens, int k, double newB, out int outcome);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_change_nonbasic_column(IntPtr sens, int row, int col, double newVal, out int outcome);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_add_activity(IntPtr sens, double cNew, double[] aNew, int na, out int outcome);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_add_constraint(IntPtr sens, double[] tech, int ntech, double rhs, out int outcome);
        // the sensitivity report: every cost range (cols - 1 entries) and RHS range (rows - 1 entries) in one call; any array may be null
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_ranging(IntPtr sens, int[] kind, int[] varRow, double[] reducedCost, double[] costLo, double[] costHi, double[] shadow, double[] rhsLo, double[] rhsHi, double[] rhsNow);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_ranging_times(IntPtr sens, out double sweepMs, out double finishMs);

        // ---- Knapsack, menu option 5 (Program.cs:430-470): KnapsackBranchBoundSolver.Solve, KnapsackBranchBoundSimplex ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_dp(IntPtr engine, long capacity, int[] weights, int[] values, int n, ref LprKnapDpOpts opts, out long best);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_bb_create(IntPtr engine, long capacity, double[] weights, double[] values, int n, out IntPtr knap);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_bb_destroy(IntPtr knap);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_bb_solve(IntPtr knap, ref LprKnapBbOpts opts, out LprKnapBbResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_bb_rank_read(IntPtr knap, int[] rank);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_bb_selected_read(IntPtr knap, int[] ids, out int count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_bb_stats(IntPtr knap, out int levels, out long evaluated, out long widest);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_bb_nodes_read(IntPtr knap, int[] parent, int[] branch, int[] status, double[] bound, int[] kitem, long[] value, long cap, out long count);

        // ---- Batched primal simplex (DESIGN.md section 12): PrimalSimplexSolver per LP, many LPs per call ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_from_lps(IntPtr engine, int count, int[] n, int[] m, double[] objective, double[] A, int[] ncoef, sbyte[] relation, double[] rhs, sbyte[] is_max, int log_cap, out IntPtr batch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_create(IntPtr engine, int count, int[] rows, int[] cols, double[] tableaux, int[] basis, int log_cap, out IntPtr batch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_destroy(IntPtr batch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_solve(IntPtr batch, ref LprBatchOpts opts, out LprBatchResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_status_read(IntPtr batch, int[] status, long[] pivots, double[] z);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_solution_read(IntPtr batch, double[] x);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_basis_read(IntPtr batch, int[] basis);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_log_read(IntPtr batch, int k, int[] rows, int[] cols, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_tableau_read(IntPtr batch, int k, [Out] double[,] rowmajor);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_shape(IntPtr batch, int k, out int rows, out int cols, out int n);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_trace_reserve(IntPtr batch, int trace_cap);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_trace_info(IntPtr batch, long[] records, long[] offset, long[] stride);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_trace_read(IntPtr batch, int k, long first, long n, double[] records);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_trace_read_all(IntPtr batch, double[] slab, long cap_doubles);

        // ---- Batched branch and bound (DESIGN.md section 13): ExecuteBranchAndBound per IP, many IPs per call ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_create(IntPtr engine, int count, int[] rows, int[] cols, double[] tableaux, int[] nvars, int node_cap, int trace_cap, out IntPtr bbBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_from_batch(IntPtr batch, int node_cap, int trace_cap, out IntPtr bbBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_destroy(IntPtr bbBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_run(IntPtr bbBatch, ref LprBbBatchOpts opts, out LprBbBatchResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_result_read(IntPtr bbBatch, int[] status, int[] found, long[] processed, int[] best_node, double[] z, long[] pivots, long[] nodes_created);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_solution_read(IntPtr bbBatch, double[] x);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_records_read(IntPtr bbBatch, int k, int[] parent, int[] kind, int[] depth, int[] var, double[] bound, int[] status, double[] z, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_pop_order_read(IntPtr bbBatch, int k, int[] ids, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_trace_read(IntPtr bbBatch, int k, int[] quads, long cap, out long count);
        // narrated B&B batch (DESIGN.md section 23): the numbers behind ExecuteBranchAndBound's console text (:1006-1233)
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_reserve(IntPtr bbBatch, long[] cap_doubles);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_info(IntPtr bbBatch, long[] tableaux, long[] doubles_made, long[] doubles_kept, long[] offset);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_pops_read(IntPtr bbBatch, int k, int[] flags, double[] z, double[] vals, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_children_read(IntPtr bbBatch, int k, long[] tab_off, int[] ntab, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_tableaux_read(IntPtr bbBatch, int k, long first_double, long n, double[] rowmajor);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_read_all(IntPtr bbBatch, double[] rowmajor, long cap_doubles);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_best_read(IntPtr bbBatch, int k, double[] rowmajor, out int rows, out int cols);

        // ---- Sensitivity scenario batch (DESIGN.md section 14): one solved model, many what-if scripts per call ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_create(IntPtr sens, int count, int[] nedits, LprSensEdit[] edits, int log_cap, out IntPtr sensBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_create_grow(IntPtr sens, int count, int[] nedits, LprSensEdit[] edits, double[] payload, long npayload, int log_cap, out IntPtr sensBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_from_batch(IntPtr batch, int count, int[] item, int[] nedits, LprSensEdit[] edits, double[] payload, long npayload, int log_cap, out IntPtr sensBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_from_batch_time(IntPtr sensBatch, out double kernelMs);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_destroy(IntPtr sensBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_run(IntPtr sensBatch, ref LprSensBatchOpts opts, out LprSensBatchResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_info(IntPtr sensBatch, out int count, out int rows, out int cols, out long total_edits, out int log_cap, out int form);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_shape_read(IntPtr sensBatch, int[] rows, int[] cols, out int max_rows, out int max_cols);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_outcomes_read(IntPtr sensBatch, int[] outcome, long[] pivots);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_state_read(IntPtr sensBatch, double[] z, int[] nsol, int[] basic);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_solution_read(IntPtr sensBatch, int k, double[] x, int cap, out int count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_tableau_read(IntPtr sensBatch, int k, [Out] double[,] rowmajor);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_log_read(IntPtr sensBatch, int k, int[] triples, long cap, out long count);
        // the report of every scenario: count x (max_cols - 1) per column, count x (max_rows - 1) per constraint,
        // int.MinValue / NaN past a scenario's own shape; any array may be null
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_ranging(IntPtr sensBatch, int[] kind, int[] varRow, double[] reducedCost, double[] costLo, double[] costHi, double[] shadow, double[] rhsLo, double[] rhsHi, double[] rhsNow);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_sens_batch_ranging_time(IntPtr sensBatch, out double kernelMs);

        // ---- Cutting-plane batch (DESIGN.md section 15): many option-4 tableaux per call ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_create(IntPtr engine, int count, int[] rows, int[] cols, double[] tableaux, int max_cuts, int log_cap, out IntPtr cutBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_from_batch(IntPtr batch, int max_cuts, int log_cap, out IntPtr cutBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_destroy(IntPtr cutBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_run(IntPtr cutBatch, ref LprCutBatchOpts opts, out LprCutBatchResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_result_read(IntPtr cutBatch, int[] code, int[] cuts, int[] rows, long[] log_count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_shape(IntPtr cutBatch, int k, out int rows, out int cols, out int row_cap, out int log_cap);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_tableau_read(IntPtr cutBatch, int k, [Out] double[,] rowmajor);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_log_read(IntPtr cutBatch, int k, int[] triples, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_z_read(IntPtr cutBatch, double[] z);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_narrate_reserve(IntPtr cutBatch, long[] cap_doubles, int ev_cap);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_narrate_info(IntPtr cutBatch, long[] events_made, long[] doubles_made, long[] doubles_kept, long[] data_off);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_narrate_events_read(IntPtr cutBatch, int k, [Out] int[] quads, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_narrate_data_read(IntPtr cutBatch, int k, long first_double, long n, [Out] double[] data);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_cut_batch_narrate_read_all(IntPtr cutBatch, [Out] int[] quads, long cap_quads, [Out] double[] data, long cap_doubles);

        // ---- Knapsack batch (DESIGN.md section 16): many option-5 instances per call ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_create(IntPtr engine, int count, long[] capacity, int[] n, double[] weights, double[] values, long[] node_cap, int narrate, out IntPtr knapBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_destroy(IntPtr knapBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_solve(IntPtr knapBatch, ref LprKnapBatchOpts opts, out LprKnapBatchResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_result_read(IntPtr knapBatch, int[] status, int[] found, double[] z, long[] evaluated, long[] widest, int[] levels);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_rank_read(IntPtr knapBatch, int[] rank);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_selected_read(IntPtr knapBatch, int[] ids, int[] counts);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_nodes_read(IntPtr knapBatch, int k, int[] parent, int[] branch, int[] status, double[] bound, int[] kitem, long[] value, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_knap_batch_dp(IntPtr knapBatch, byte[] which, long[] best);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_create(IntPtr engine, int count, int[] n, int[] m, double[] objective, double[] A, double[] b, sbyte[] is_min, int log_cap, out IntPtr revBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_destroy(IntPtr revBatch);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_solve(IntPtr revBatch, ref LprRevBatchOpts opts, out LprRevBatchResult res);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_status_read(IntPtr revBatch, int[] status, long[] iterations, double[] z);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_solution_read(IntPtr revBatch, double[] x);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_basis_read(IntPtr revBatch, int[] basis);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_log_read(IntPtr revBatch, int k, int[] row, int[] enter, int[] leave, long cap, out long count);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_binv_read(IntPtr revBatch, int k, [Out] double[,] rowmajor);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_xb_read(IntPtr revBatch, int k, double[] xB);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_shape(IntPtr revBatch, int k, out int n, out int m);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_trace_reserve(IntPtr revBatch, int trace_cap);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_trace_info(IntPtr revBatch, long[] snapshots, long[] offset, long[] stride);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_trace_read(IntPtr revBatch, int k, long first, long n, double[] records);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_rev_batch_trace_read_all(IntPtr revBatch, double[] slab, long cap_doubles);

        // ---- Device text (DESIGN.md section 25): TableIterationFormater.Format (:22-48) without its title line, written on the device ----
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_text_format_tableaux(IntPtr engine, int count, int[] rows, int[] cols, int[] nvars, double[] tableaux, out IntPtr text);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_batch_trace_text(IntPtr batch, long[] first_block, out IntPtr text);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_text_format_tableaux_rounded(IntPtr engine, int count, int[] rows, int[] cols, int[] nvars, int[] round4, double[] tableaux, out IntPtr text);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_bb_batch_narrate_text(IntPtr bbBatch, long[] first_block, out IntPtr text);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_text_info(IntPtr text, out long blocks, out long bytes, out double kernel_ms);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_text_offsets_read(IntPtr text, long[] offsets);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_text_read(IntPtr text, long first_byte, long n, byte[] bytes);
        [DllImport(Lib, CallingConvention = CC)] internal static extern int lpr_text_destroy(IntPtr text);

        internal static string LastError() => Marshal.PtrToStringAnsi(lpr_last_error()) ?? "";

        internal static void ThrowIfError(int status, string where)
        {
            if (status < 0) throw new InvalidOperationException($"{where}: {(LprStatus)status} -- {LastError()}");
        }
    }

    /// <summary>One engine (HIP device 0 + stream) for the process, released at exit.</summary>
    internal static class Engine
    {
        private static IntPtr _handle = IntPtr.Zero;
        internal static IntPtr Handle
        {
            get
            {
                if (_handle == IntPtr.Zero)
                {
                    NativeMethods.ThrowIfError(NativeMethods.lpr_engine_open(0, out _handle), "lpr_engine_open");
                    AppDomain.CurrentDomain.ProcessExit += (s, e) => NativeMethods.lpr_engine_close(_handle);
                }
                return _handle;
            }
        }
    }
}
