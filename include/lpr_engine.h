/*
 * lpr_engine.h -- C ABI of the MI355X (gfx950) simplex pivot engine.
 *
 * This is the drop-in boundary for the dense-tableau hot path of
 * Storm-Tarran/LPR_381_Group_V22.  The reference has no FFI layer of its own;
 * its de-facto boundary is the public surface of three C# classes consumed by
 * Program.cs.  Every entry point below names the reference member it replaces
 * (paths relative to LPR_381_Group_V22/ in the reference tree).  The C# side
 * binds these with [DllImport("lpr_engine")] -- see INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no exceptions cross this boundary.
 *   - every function returns an lpr_status (>= 0: solver outcome, < 0: error);
 *     the text of the last error on the calling thread is lpr_last_error().
 *   - input buffers are borrowed for the duration of the call only (P/Invoke
 *     pins blittable arrays); outputs go to caller-allocated buffers.
 *   - handles are opaque, owned by the library, not thread-safe; one engine
 *     == one HIP device + one stream.
 *   - matrices are row-major fp64 (C# double[,] is contiguous row-major);
 *     column / variable indices are 0-based; tableau row 0 is the Z row, so
 *     constraint rows (and pivot-log rows of the tableau solver) are 1-based
 *     exactly as in PrimalSimplexSolver.cs:138,142.
 *   - all arithmetic on the device is IEEE binary64, no FMA contraction,
 *     true division -- bit-for-bit the C# expressions it replaces.
 */
#ifndef LPR_ENGINE_H
#define LPR_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPR_ABI_VERSION 1

/* Solver outcomes mirror the reference's behaviours one-to-one:
 *   OPTIMAL              PrimalSimplexSolver.cs:110-126 / RevisedPrimalSimplexSolver.cs:124-146
 *   UNBOUNDED            PrimalSimplexSolver.cs:129-135 (print + break) /
 *                        RevisedPrimalSimplexSolver.cs:178-179 (throw "Unbounded problem ...")
 *   INFEASIBLE_BASIS     RevisedPrimalSimplexSolver.cs:90-91
 *   PIVOT_TOO_SMALL      RevisedPrimalSimplexSolver.cs:267
 *   ENTERING_ALREADY_BASIC RevisedPrimalSimplexSolver.cs:182-183
 *   PIVOT_LIMIT          (no reference equivalent: the C# loops are uncapped; returned only when
 *                         the caller sets max_pivots)
 *   BB_NODE_CAP          BranchBoundSimplexSolver.cs:1038-1042 ("Potential infinite loop detected")
 *   BB_DEPTH_CAP         (no reference equivalent: lpr_bb_solve_level_sync stopped at max_levels
 *                         with fractional nodes it scored but did not branch)
 */
typedef enum lpr_status {
    LPR_OK_OPTIMAL = 0,
    LPR_UNBOUNDED = 1,
    LPR_INFEASIBLE_BASIS = 2,
    LPR_PIVOT_TOO_SMALL = 3,
    LPR_ENTERING_ALREADY_BASIC = 4,
    LPR_PIVOT_LIMIT = 5,
    LPR_BB_NODE_CAP = 6,
    LPR_BB_DEPTH_CAP = 7,
    LPR_BAD_ARGUMENT = -1,
    LPR_DEVICE_ERROR = -2,
    LPR_OUT_OF_MEMORY = -3
} lpr_status;

/* Constraint relation codes for lpr_tableau_from_lp (InputFileParser.Constraint.Relation,
 * IO/InputFileParser.cs:70-82).  Anything that is not ">=" is treated as "<=" by the reference
 * (PrimalSimplexSolver.cs:36-50). */
enum { LPR_REL_LE = 0, LPR_REL_GE = 1, LPR_REL_EQ = 2 };

typedef struct lpr_engine lpr_engine;
typedef struct lpr_tableau lpr_tableau;

/* ------------------------------------------------------------------ engine */

int lpr_abi_version(void);
/* Thread-local text of the last failure ("" if none). */
const char* lpr_last_error(void);
/* Binds HIP device `device`, creates the engine stream.  LPR_DEVICE_ERROR if no gfx950 device. */
int lpr_engine_open(int device, lpr_engine** out);
int lpr_engine_close(lpr_engine* e);
/* Blocks until all work queued on the engine stream has finished. */
int lpr_engine_sync(lpr_engine* e);
/* The engine's hipStream_t as an integer (for callers that time with their own HIP events). */
uint64_t lpr_engine_stream(lpr_engine* e);

/* ------------------------------------------------------- tableau (primal) */

/* Replaces `new PrimalSimplexSolver(objective, constraints, isMaximization)`
 * (Simplex/PrimalSimplexSolver.cs:27-87), built on the device:
 *   row 0      = -c (max) or +c (min)                         :61-62
 *   ">=" rows  negated incl. RHS; "=" and others kept as "<=" :36-50
 *   row i+1    = [first min(n, ncoef[i]) coeffs | e_i | rhs]  :68-82
 *   basis[i]   = n + i                                         :78
 * A is m x lda row-major (lda >= n); ncoef may be NULL (== n for every row). */
int lpr_tableau_from_lp(lpr_engine* e, int n, int m, const double* objective,
                        const double* A, int lda, const int32_t* ncoef,
                        const int8_t* relation, const double* rhs, int is_max,
                        lpr_tableau** out);

/* Adopts a ready (rows x cols) row-major tableau + basis (rows-1 column indices); the entry used
 * by BranchAndBoundAdapter-style callers that already hold a double[,] (BranchAndBoundAdapter.cs:31-46). */
int lpr_tableau_create(lpr_engine* e, int rows, int cols, const double* rowmajor,
                       const int32_t* basis, lpr_tableau** out);

/* Benchmark input: dense random LP generated ON the device by the counter-based
 * generator documented in DESIGN.md (SplitMix64 keyed by (seed, stream, i, j)), so that the
 * 402.8 MB tableau of the m=4096,n=8192 configuration never crosses PCIe:
 *   A[i][j] ~ U(0,1), b_i = (n/4)*(1 + 0.1*U(0,1)), c_j ~ U(0,1), all "<=", maximise. */
int lpr_tableau_synthetic(lpr_engine* e, int m, int n, uint64_t seed, lpr_tableau** out);

int lpr_tableau_destroy(lpr_tableau* t);
int lpr_tableau_shape(const lpr_tableau* t, int* rows, int* cols, int* ld);

/* Solver options.  Zero-initialise, then set fields; defaults equal the reference's literals. */
typedef struct lpr_solve_opts {
    int64_t max_pivots;    /* <= 0: uncapped like PrimalSimplexSolver.cs:107 */
    int32_t time_kernels;  /* != 0: launch eagerly and bracket rank-1 update / sweep launches with
                              HIP events on the engine stream (every sweep on the K-pivot paths,
                              one update in four on the one-pivot path); read back with
                              lpr_tableau_kernel_stats / lpr_tableau_step_stats  On the K-pivot paths a value n > 1 brackets every
                              n-th step only (the events sit on the sweep's stream: two per step
                              cost the two-stream pipeline ~3 %). */
    int32_t batch;         /* pivots queued between host polls of the device status word (0: auto) */
    int32_t variant;       /* kernel variant (0: auto); for tuning and tests only, same bits.  Decoded
                              in one place, primal_plan() of csrc/primal_plan.hpp (DESIGN 4b
                              "Control"), which names every value below.  Low 16
                              bits: path + sweep tile (0x30tr two-stream overlap, 0x40tr heads then
                              in-place sweep; tr = 0x04/0x08/0x10 rows per chunk, 0x24/0x28 two
                              chunks in flight).  0x50tr and 0x60tr named forms since retired and
                              are accepted as aliases of 0x30tr and 0x40tr (so 0x60tr with block > 8
                              now runs `block` pivots per sweep, where it used to cap them at 8).
                              Bits 16..24, K-pivot paths: 0x10000 diagnostic time stamps of the loop
                              heads, 0x20000 loop heads not confined to one XCD, 0x40000 confined
                              but hand-offs through the memory side, 0x80000 the sweep does not
                              leave the heads' XCD to them, 0x100000 it does so only once this
                              launch's heads have said where they are (no hint from the previous
                              launch), 0x200000 the heads of a step follow their predecessor
                              at once and wait for the previous sweep on a device flag instead of
                              a cross-stream event, 0x400000 the sweep of a step follows its
                              predecessor at once and asks the heads' completion word as it starts.
                              Both need the two kernels of a step to run at the same time (tools
                              that serialise kernels -- rocprofv3 --pmc -- prevent that: the
                              bounded waits then end the solve with LPR_DEVICE_ERROR) and neither
                              is faster than the events any more: opt-in only.
                              0x800000: every tile of the two-stream sweep non-temporal (by
                              default the tiles at both ends of its work queue keep the default
                              cache policy).  0x1000000: no 64-row tiles at the head of that queue
                              (by default the row tiles of its first half are handed out in pairs,
                              so that a lane loads its pivot-row slices once per 64 rows).
                              0x2000000: the two-stream path never uses the condensed working
                              layout (by default a call with a budget of 1 024 pivots or more, or
                              none, works on buffers that leave out the unit columns of its start
                              basis); 0x4000000: it uses it whatever the size of the
                              tableau or the length of the call (tests).  Same bits either way. */
    int32_t block;         /* pivots decided ahead and applied per sweep of the tableau on large
                              tableaux: 0 auto (16), 1 one pivot per sweep, 2..16 that many.  The bits
                              stored are the same for every value (each element goes through the
                              same sequence of rounded operations, in registers). */
} lpr_solve_opts;

typedef struct lpr_solve_result {
    int32_t status;        /* lpr_status */
    int32_t block;         /* pivots per sweep this call used (1 on the small-tableau paths) */
    int64_t pivots;        /* pivots performed by THIS call */
    int64_t total_pivots;  /* pivots performed on this tableau so far (== C# `iteration`) */
    double z;              /* T[0, cols-1] at exit (FinalZ, PrimalSimplexSolver.cs:113); the C#
                              leaves FinalZ = 0 on the unbounded exit -- the host mirror does that */
} lpr_solve_result;

/* Replaces PrimalSimplexSolver.Solve() (Simplex/PrimalSimplexSolver.cs:102-150): repeats
 * FindEnteringVariable -> FindLeavingVariable -> Pivot -> basicVariables[r-1] = e on the device
 * until optimal / unbounded / max_pivots.  No tableau data crosses the host boundary. */
int lpr_primal_solve(lpr_tableau* t, const lpr_solve_opts* opts, lpr_solve_result* res);

/* Single-step forms of the same three private methods, for callers (and tests) that drive the
 * loop themselves:
 *   lpr_select_entering  FindEnteringVariable  PrimalSimplexSolver.cs:152-167   (-1: optimal)
 *   lpr_select_leaving   FindLeavingVariable   PrimalSimplexSolver.cs:169-191   (-1: unbounded)
 *   lpr_pivot            Pivot                 PrimalSimplexSolver.cs:193-211   (+ basis update :142)
 */
int lpr_select_entering(lpr_tableau* t, int32_t* col);
int lpr_select_leaving(lpr_tableau* t, int32_t col, int32_t* row);
int lpr_pivot(lpr_tableau* t, int32_t row, int32_t col);

/* Replaces ExtractSolution() + FinalZ (PrimalSimplexSolver.cs:213-252, :113): x has n entries. */
int lpr_extract_solution(lpr_tableau* t, int n, double* x, double* z);

/* Result accessors (PrimalSimplexSolver.cs:18-24, 269-278). */
int lpr_tableau_read(lpr_tableau* t, double* rowmajor_out);            /* rows*cols doubles   */
int lpr_tableau_read_block(lpr_tableau* t, int row0, int nrows, int col0, int ncols,
                           double* out);                               /* nrows*ncols doubles */
int lpr_basis_read(lpr_tableau* t, int32_t* basis_out);                /* rows-1 ints         */
/* Pivot log: (row, col) pairs in order, row 1-based like the C# console line (:138).  Returns the
 * number of pairs written through *count (at most cap). */
int lpr_pivot_log_read(lpr_tableau* t, int32_t* rows_out, int32_t* cols_out, int64_t cap,
                       int64_t* count);

/* Timing of the rank-1 update launches recorded while opts.time_kernels was set:
 * launches, summed and average duration in milliseconds (HIP events on the engine stream). */
int lpr_tableau_kernel_stats(lpr_tableau* t, int64_t* launches, double* total_ms, double* avg_ms);
/* K-pivot paths: the steps timed with the sweeps above.  A step is one sweep of K pivots together
 * with the loop heads of the next K (start of one sweep to the start of the next). */
int lpr_tableau_step_stats(lpr_tableau* t, int64_t* steps, double* total_ms);
/* Diagnostic (opts.variant bit 16): s_memrealtime stamps (10 ns ticks) the lead loop-head workgroup
 * left per pivot and phase -- 64 pivots x 12 stamps, then its XCC id and whether the launch handed
 * off through the XCD's L2.  Not part of the solver surface of the reference. */
int lpr_debug_head_stamps(lpr_tableau* t, uint64_t* out, int64_t cap, int64_t* count);

/* ------------------------------------- cutting-plane side path ("next" row f3)
 * The reference's dual simplex / second primal simplex / Gomory step (dead code in its menu,
 * Program.cs:417-428) on the same device tableau: row 0 = objectiveRow, rows 1.. = constraintRows.
 * They differ from PrimalSimplexSolver by EPS-band selection rules and by leaving rows whose
 * factor is within 1e-9 of zero untouched.  `print_steps` reproduces the C# quirk that `iter`
 * (and with it max_iters) only advances when printSteps is set; hard_cap (<= 0: none) is an
 * extra pivot limit with no C# counterpart.
 *   lpr_dual_solve     DualSimplexSolver.Solve     Simplex/DualSimplex.cs:14-114
 *                      status: OPTIMAL (true) / INFEASIBLE_BASIS (false, :72-76) / PIVOT_LIMIT
 *   lpr_primal2_solve  PrimalSimplexSolver2.Solve  Simplex/PrimalSimplexSolver2.cs:46-97
 *                      status: OPTIMAL (true) / UNBOUNDED (false, :63-68) / PIVOT_LIMIT
 *   lpr_cutting_plane  CuttingPlaneSolver.CuttingPlaneSolution
 *                      IntegerProgramming/CuttingPlaneSolver.cs:64-229 (recursion unrolled, at most
 *                      max_cuts cuts; every cut appends one ROW, no slack column, :104-110).
 *                      *exit_code: 0 optimal tableau displayed (:224), 1 all RHS integral (:87-91),
 *                      2 no pivot column on the cut (:134-138), 3 pivot too small (:146-150),
 *                      4 dual simplex failed (:191), 5 "step finished" (:228), 6 max_cuts reached,
 *                      7 an InvalidOperationException escaped a solver.
 *   lpr_cut_log_read   pivots of this path in order: triples (kind 0 dual / 1 primal2 / 2 cut,
 *                      row in the C#'s own numbering, column). */
int lpr_dual_solve(lpr_tableau* t, int max_iters, int print_steps, int64_t hard_cap,
                   lpr_solve_result* res);
int lpr_primal2_solve(lpr_tableau* t, int max_iters, int print_steps, int64_t hard_cap,
                      lpr_solve_result* res);
int lpr_cutting_plane(lpr_tableau* t, int max_cuts, int64_t hard_cap, int32_t* exit_code,
                      int32_t* cuts);
int lpr_cut_log_read(lpr_tableau* t, int32_t* triples, int64_t cap, int64_t* count);

/* -------------------------------------------------- revised primal simplex */

typedef struct lpr_revised lpr_revised;

/* Replaces `new RevisedPrimalSimplexSolver(objective, constraints, isMinimization)`
 * (Simplex/RevisedPrimalSimplexSolver.cs:41-80): c = -objective if is_min (:51), dense A[m, n] and
 * b[m] copied to HBM, B^-1 = I, basis = slacks.  Every row is treated as "<=": the reference never
 * reads Constraint.Relation here.  The C# ArgumentExceptions (:43-44, :57-58: empty objective /
 * constraints, wrong coefficient count) are LPR_BAD_ARGUMENT; the row-length check is the
 * caller's because A arrives already flattened (lda >= n). */
int lpr_revised_create(lpr_engine* e, int n, int m, const double* objective, const double* A,
                       int lda, const double* b, int is_min, lpr_revised** out);
/* The synthetic dense LP of lpr_tableau_synthetic in (c, A, b) form, generated on the device. */
int lpr_revised_synthetic(lpr_engine* e, int m, int n, uint64_t seed, lpr_revised** out);
int lpr_revised_destroy(lpr_revised* s);

typedef struct lpr_revised_result {
    int32_t status;           /* lpr_status; the C# throws for 1..4 with the messages of
                                 :91 / :179 / :183 / :267 -- the host mirror re-raises them */
    int32_t reserved;
    int64_t iterations;       /* pivots performed by THIS call */
    int64_t total_iterations; /* pivots so far (the C# `iteration`, :249) */
    double z;                 /* FinalZ = Dot(cOrig, x) (:286); valid when status == OPTIMAL */
} lpr_revised_result;

/* Replaces RevisedPrimalSimplexSolver.Solve() (:82-251) + ExtractSolution (:277-287).  Per
 * iteration: x_B = B^-1 b, feasibility, y = c_B B^-1, reduced costs, entering fold (:105-121),
 * u = B^-1 a_e, ratio fold (:154-176), bookkeeping, B^-1 <- E B^-1 (:264-275).  All sums in the
 * C#'s sequential order, all on the device.  Only opts->max_pivots and opts->batch are used. */
int lpr_revised_solve(lpr_revised* s, const lpr_solve_opts* opts, lpr_revised_result* res);

/* SolutionVector / FinalZ (:36-38): x has n entries.  Valid after an OPTIMAL solve. */
int lpr_revised_solution(lpr_revised* s, double* x, double* z);
/* BasicVariables (:39): m entries, by basis row. */
int lpr_revised_basis_read(lpr_revised* s, int32_t* basis_out);
/* Pivot log: (leavingRow 0-based, entering variable, leaving variable) per iteration. */
int lpr_revised_log_read(lpr_revised* s, int32_t* row_out, int32_t* enter_out,
                         int32_t* leave_out, int64_t cap, int64_t* count);
/* BInverse (m x m row-major) and the last x_B (m), for snapshots and tests. */
int lpr_revised_binv_read(lpr_revised* s, double* out);
int lpr_revised_xb_read(lpr_revised* s, double* out);

/* Replaces `MultiplyMatrices(BInverse, A)` of CaptureSnapshot (:360, helper :426-441, zero-skip
 * |b_ik| < 1e-9): the m x n product B^-1 * A, computed on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64).  out (m x n row-major) may be NULL to keep the product on the device
 * (benchmarking); *ms, if not NULL, receives the kernel time in milliseconds (HIP events).
 * This product only feeds the printed tableau, so its contract is a tolerance
 * (|err| <= 1e-9 * sum_k |b_ik a_kj|), not bit equality -- DESIGN.md. */
int lpr_revised_binv_a(lpr_revised* s, double* out, double* ms);

/* ---- IterationSnapshots of the revised solver (RevisedPrimalSimplexSolver.cs:36, consumed by
 * Program.cs:329-347).  The C# appends one text block per iteration (CaptureSnapshot :294-387); the
 * numbers in it come from the device through the three calls below, the host only formats them
 * (NumFormat.N3 :451-466).  Meant for the models a person reads (snapshot policy "all"); a solve
 * without snapshots is lpr_revised_solve. */
typedef struct lpr_revised_snapshot_info {
    int32_t status;        /* LPR_PIVOT_LIMIT: one pivot done, the loop goes on ("Iteration k"
                              snapshot, :232-247); LPR_OK_OPTIMAL: the "Optimal" snapshot
                              (:124-146); any other status: the C# threw, no snapshot */
    int32_t entering;      /* enteringIdx (-1 on the Optimal snapshot) */
    int32_t leaving_row;   /* leavingRow, 0-based basis row */
    int32_t leaving_var;   /* leavingVarIndex_Pre */
    double entering_rc_pre;  /* :189-191 */
    double z_working;      /* Dot(cB, xB) :245 / :141 */
    double z_original;     /* ComputeOriginalZFromCurrentBasis(xB) :246 / finalZ :142 */
} lpr_revised_snapshot_info;

/* ONE pass of the while-loop of Solve() (:86-249), including the post-pivot recomputation of
 * x_B, y and the reduced costs (:217-227) that the snapshot prints.  Returns info->status.
 * Can be mixed freely with lpr_revised_solve on the same handle. */
int lpr_revised_step(lpr_revised* s, lpr_revised_snapshot_info* info);
/* What the last lpr_revised_step left: y (m), rc (n + m: rcX then rcS = -y), u_pre (m), ratios_pre
 * (m, +inf where u_i <= EPS), basisForRatios_Pre (m), x_B (m).  Any pointer may be NULL.  After
 * an "Optimal" step u / ratios / basis_pre are those of the previous pivot -- the C# prints zeros
 * and infinities there (:133-134). */
int lpr_revised_snapshot_read(lpr_revised* s, double* y, double* rc, double* u, double* ratios,
                              int32_t* basis_pre, double* xB);
/* MultiplyMatrices(BInverse, A) (:360) in the C#'s own summation order (k ascending, |a_ik| < EPS
 * skipped, product rounded then added) -- bit-exact, for the printed table of small models, where
 * a 3-decimal tie must round as the C# rounds it.  out: m x n row-major. */
int lpr_revised_binv_a_exact(lpr_revised* s, double* out);

/* ------------------------------------------------------- branch and bound */

typedef struct lpr_bb lpr_bb;

/* Replaces BranchAndBoundAdapter.SolveFromPrimal's set-up (IntegerProgramming/
 * BranchAndBoundAdapter.cs:9-24): Convert(primal.FinalTableau) (:31-46) becomes the root node
 * (node id 0) in HBM, SetNumVars(nvars) (:20).  max_depth bounds the branching depth (every level
 * adds one row and one column; node buffers are sized for it; <= 0: 64).
 *   lpr_bb_create               from a host double[,] (rows x cols row-major)
 *   lpr_bb_create_from_tableau  from a solved device tableau -- no host round trip */
int lpr_bb_create(lpr_engine* e, const double* final_tableau, int rows, int cols, int nvars,
                  int max_depth, lpr_bb** out);
int lpr_bb_create_from_tableau(lpr_tableau* t, int nvars, int max_depth, lpr_bb** out);
int lpr_bb_destroy(lpr_bb* b);

typedef struct lpr_bb_opts {
    int32_t enable_pruning; /* ShouldPrunebranch (:985-1004); Program.cs:389 passes false */
    int32_t node_cap;       /* <= 0: 20, the reference's hard stop (:1038-1042) */
    int32_t reserved[2];
} lpr_bb_opts;

typedef struct lpr_bb_result {
    int32_t status;        /* LPR_OK_OPTIMAL (stack emptied) or LPR_BB_NODE_CAP */
    int32_t found;         /* 0: "No integer solution found" -> the C# returns (null, -inf) */
    int64_t processed;     /* branchCount (:1045) */
    int32_t best_node;     /* record id of the optimal branch, -1 if none */
    int32_t reserved;
    double z;              /* optimalValue (rounded to 4 decimals like every B&B value) */
    int64_t pivots;        /* dual + primal pivots over all child LPs */
    int64_t nodes_created; /* node records (root + every child attempted) */
} lpr_bb_result;

/* Replaces BranchAndBound.ExecuteBranchAndBound (BranchBoundSimplexSolver.cs:1006-1233) in the
 * reference's own order: DFS stack, lower child first, incumbent replaced on strict improvement,
 * 4-decimal Math.Round between all stages.  Per popped node the two children (AddConstraint
 * :694-803, DoDualSimplex :289-468 = PerformDualPivot :115-201 then PerformPrimalPivot :203-279)
 * are evaluated as one batch on the device.  x (nvars entries) is written when found. */
int lpr_bb_run(lpr_bb* b, const lpr_bb_opts* opts, double* x, lpr_bb_result* res);

/* Node records of the last lpr_bb_run, in creation order (record 0 = root): parent record, kind
 * (0 root / 1 lower / 2 upper), depth, branching variable, bound, status (0 solved, 1 infeasible
 * = DoDualSimplex returned a null optimum, 2 failed = an exception escaped it), rounded z. */
int lpr_bb_records_read(lpr_bb* b, int32_t* parent, int32_t* kind, int32_t* depth, int32_t* var,
                        double* bound, int32_t* status, double* z, int64_t cap, int64_t* count);
/* Record ids in the order the nodes were popped (processed). */
int lpr_bb_pop_order_read(lpr_bb* b, int32_t* ids, int64_t cap, int64_t* count);
/* Pivot trace of the last run: quads (record id, phase 0 dual / 1 primal / 2 "last tableau
 * dropped" :395-400, row, col). */
int lpr_bb_trace_read(lpr_bb* b, int32_t* quads, int64_t cap, int64_t* count);

/* Building blocks of the same path for callers that drive the tree themselves (the
 * level-synchronous multi-GPU driver shards the frontier over ranks and calls these per level):
 *   lpr_bb_node_info  RoundAllTableaux on pop (:1047) + GetObjective (:892-897) + the decision
 *                     values of CheckIntegerBasicVar / ExtractSolution (:807-827, :899-921);
 *                     z_out[count], vals_out[count * nvars]
 *   lpr_bb_expand     for each (parent, var, bound, kind 0 "<=" / 1 ">="): AddConstraint +
 *                     DoDualSimplex + RoundAllTableaux, all children in one batch;
 *                     status_out: 2 solved (child_ids_out = new node id), 3 infeasible, 4 failed
 *   lpr_bb_release    frees node buffers
 *   lpr_bb_node_read  copies a node tableau to the host (tests / snapshots) */
int lpr_bb_node_info(lpr_bb* b, const int32_t* ids, int count, double* z_out, double* vals_out);
int lpr_bb_expand(lpr_bb* b, int count, const int32_t* parent_ids, const int32_t* var,
                  const double* bound, const int32_t* kind, int32_t* child_ids_out,
                  int32_t* status_out, int32_t* pivots_out);
/* lpr_bb_expand for a caller that also reproduces what the reference PRINTS about each child
 * (ExecuteBranchAndBound :1086-1208): the pivots of DoDualSimplex ("pivot @ constraint r, column c",
 * :198 / :276) and every tableau of its list (:292, :341, :388) for DisplayTableau (:623-640) --
 * the one AddConstraint hands it, then one per pivot; a last tableau dropped by :395-400 is dropped
 * here too.  Small models only: the tableaux are copied off the device after every pivot step.
 *   trace_out: (phase 0 dual / 1 primal / 2 "last tableau dropped", row, col) triples of all
 *     children, child k's are [trace_off_out[k], trace_off_out[k + 1]) (count + 1 offsets);
 *   tab_out: child k's ntab_out[k] tableaux, each (parent rows + 1) x (parent cols + 1) row-major,
 *     from tab_off_out[k] (doubles; count + 1 offsets).  Buffers too small: LPR_BAD_ARGUMENT, the
 *     offsets still say how much is needed. */
int lpr_bb_expand_traced(lpr_bb* b, int count, const int32_t* parent_ids, const int32_t* var,
                         const double* bound, const int32_t* kind, int32_t* child_ids_out,
                         int32_t* status_out, int32_t* pivots_out, int32_t* trace_out,
                         int64_t trace_cap, int64_t* trace_off_out, double* tab_out, int64_t tab_cap,
                         int64_t* tab_off_out, int32_t* ntab_out);
int lpr_bb_release(lpr_bb* b, const int32_t* ids, int count);
int lpr_bb_node_read(lpr_bb* b, int32_t id, double* out, int32_t* rows, int32_t* cols);

/* ---- multi-GPU Branch & Bound: one process per GPU, sub-trees sharded over the ranks, ONE
 * all-reduce(MAX) of the incumbent bound per level over RCCL / xGMI.  The reference
 * loop being sharded is ExecuteBranchAndBound (BranchBoundSimplexSolver.cs:1006-1233) with its
 * 20-node stop lifted; with pruning off (Program.cs:389) the explored tree, and so the answer,
 * does not depend on the number of ranks. */
typedef struct lpr_comm lpr_comm;
#define LPR_COMM_ID_BYTES 128
/* Rank 0 makes the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by whatever
 * channel the host has (a file, a socket, its launcher's environment); then every rank calls
 * lpr_comm_init with its engine (= its GPU): ncclCommInitRank. */
int lpr_comm_unique_id(uint8_t id[LPR_COMM_ID_BYTES]);
int lpr_comm_init(lpr_engine* e, int rank, int world, const uint8_t id[LPR_COMM_ID_BYTES],
                  lpr_comm** out);
/* The same with the caller's own transport instead of RCCL.  Both callbacks return 0 on success
 * and are invoked on the calling thread only: all_reduce_max(user, v, n) leaves in v[0..n) the
 * element-wise maximum over all ranks; all_gather(user, send, recv, bytes) leaves in
 * recv[world * bytes] the `bytes` of every rank in rank order. */
typedef int (*lpr_allreduce_max_fn)(void* user, double* inout, int count);
typedef int (*lpr_allgather_fn)(void* user, const void* send, void* recv, int bytes);
int lpr_comm_init_custom(int rank, int world, lpr_allreduce_max_fn all_reduce_max,
                         lpr_allgather_fn all_gather, void* user, lpr_comm** out);
int lpr_comm_destroy(lpr_comm* c);
/* rank, world and how many collectives this communicator has issued so far */
int lpr_comm_info(const lpr_comm* c, int* rank, int* world, int64_t* allreduce_calls,
                  int64_t* allgather_calls);
/* inout[0..count) <- maximum over all ranks (count <= 64); the collective the B&B levels use */
int lpr_comm_all_reduce_max(lpr_comm* c, double* inout, int count);

typedef struct lpr_bb_sync_opts {
    int32_t enable_pruning;  /* ShouldPrunebranch (:985-1004) against the all-reduced bound */
    int32_t max_levels;      /* <= 0: max_depth of the handle */
    int64_t max_nodes;       /* stop once a rank has processed more than this (<= 0: 2^20) */
} lpr_bb_sync_opts;

typedef struct lpr_bb_sync_result {
    int32_t status;      /* LPR_OK_OPTIMAL; LPR_BB_NODE_CAP when max_nodes stopped it; LPR_BB_DEPTH_CAP
                          * when max_levels did (the nodes of that depth are still scored); < 0: a
                          * rank failed and EVERY rank returns that status from the same level */
    int32_t found;       /* 0: no integer solution */
    int64_t processed;   /* nodes scored, all ranks */
    int64_t pivots;      /* dual + primal pivots of all child LPs, all ranks */
    int32_t levels;      /* levels branched (depth reached).  All-reduces issued = levels, + 1 when a
                          * scoring-only pass over the depth-max_levels frontier followed */
    int32_t path_len;    /* the winner's branch path: path_len sides from the root ... */
    uint64_t path_bits;  /* ... bit k = side taken at depth k (0 lower "<= floor", 1 upper) */
    double z;            /* incumbent objective (rounded to 4 decimals like every B&B value) */
} lpr_bb_sync_result;

/* Level-synchronous form of ExecuteBranchAndBound (:1006-1233): every level scores this rank's
 * frontier (IsInteger :595-599, CheckIntegerBasicVar :829-847), branches (CreateBranches
 * :859-890), evaluates ALL children in one batch (AddConstraint + DoDualSimplex on the device)
 * and issues ONE all-reduce(MAX) of {incumbent z, "someone has nodes left", "someone hit
 * max_nodes", "someone failed" (its lpr_status), "someone left nodes unbranched at max_levels"}.
 * A rank-local failure (device error, out of memory, a cycling child's pivot limit) is never
 * returned before that collective: it rides in it, so all ranks return it together instead of the
 * healthy ones waiting for ever (the per-branch catch of :1145-1148,1205-1208 is the reference's
 * analogue).  Every rank must pass the same opts and handles of the same max_depth.  The first ceil(log2(world)) levels are done by every rank alike; the frontier at
 * that depth is dealt round robin in DFS order and a sub-tree then stays on its rank -- tableaux
 * never move.  With pruning off (the reference's setting, Program.cs:389) ties on z go to the node
 * the reference's stack pops first; with enable_pruning a tied integer node that the DFS would
 * have met BEFORE the incumbent may be pruned here (same z, possibly another x).  One all-gather
 * at the end names the winner.  Test hook: the environment variable LPR_BB_INJECT_FAULT=
 * "<rank>:<level>" makes that rank fail at that level.  comm == NULL: a single rank.  Every rank passes a handle holding the
 * same root; x (nvars) is written on every rank when found. */
int lpr_bb_solve_level_sync(lpr_bb* b, lpr_comm* comm, const lpr_bb_sync_opts* opts, double* x,
                            lpr_bb_sync_result* res);

/* ------------------------------------------------------------------------------------------
 * Sensitivity re-solve ("next" row f4): SensitivityAnalysis/SensitivityAnalyzer.cs.
 * The analyzer owns a device copy of the final tableau (the C# clones it, :24).  The console
 * prompts of the C# become arguments; every edit reports an lpr_sens_outcome through *outcome
 * (the function's own return value is an lpr_status: < 0 only for API / device failures).
 * Range displays, shadow prices and the duality print-out are read-only arithmetic on a few rows
 * and columns: the host mirror does them from lpr_sens_read_block / lpr_sens_column_fold. */
typedef struct lpr_sens lpr_sens;

enum lpr_sens_outcome {
    LPR_SENS_OK = 0,                 /* re-solved; z / solution vector refreshed (:159-165)      */
    LPR_SENS_UNBOUNDED = 1,          /* "Unbounded during re-optimization." :151                 */
    LPR_SENS_INFEASIBLE = 2,         /* "Infeasible after RHS change (dual simplex)." :197       */
    LPR_SENS_ZERO_PIVOT = 3,         /* "Zero pivot encountered." :101                           */
    LPR_SENS_ITER_LIMIT = 5,         /* "Iteration limit in ReOptimize / dual simplex" :126 :183 */
    LPR_SENS_ROLLED_BACK = 8,        /* ChangeRHS caught an exception and restored (:462-469)    */
    LPR_SENS_INDEX_OUT_OF_RANGE = 9, /* AddNewConstraint: a row without a basic column (tech[-1]) */
    LPR_SENS_INVALID_INDEX = -1      /* the C# prints "Invalid ..." and returns; nothing changed */
};

/* ctor :22-39 (basicVariables is rebuilt from the tableau by :35, so it is not an argument).
 * final_tableau is rows x cols row-major with row 0 = Z row; cols >= rows. */
int lpr_sens_create(lpr_engine* e, const double* final_tableau, int32_t rows, int32_t cols,
                    const double* solution, int32_t nsol, double z, lpr_sens** out);
/* Program.cs:147-151: primalSolver.GetFinalTableau() / SolutionVector / FinalZ handed over device
 * to device from a solved primal tableau (n_decision = objective.Count). */
int lpr_sens_create_from_tableau(lpr_tableau* t, int32_t n_decision, lpr_sens** out);
int lpr_sens_destroy(lpr_sens* s);
/* numRows, numCols, solutionVector.Count, basicVars.Count, CurrentZ :728, pivots of the last edit */
int lpr_sens_shape(lpr_sens* s, int32_t* rows, int32_t* cols, int32_t* nsol, int32_t* nbasic,
                   double* z, int64_t* last_pivots);
/* CurrentTableau :727 (rows x cols, dense), basicVars, CurrentSolutionVector :729; any may be NULL */
int lpr_sens_read(lpr_sens* s, double* tableau, int32_t* basic, double* solution);
int lpr_sens_read_block(lpr_sens* s, int32_t row0, int32_t nrows, int32_t col0, int32_t ncols,
                        double* out);
int lpr_sens_basic_row(lpr_sens* s, int32_t col, int32_t* row);   /* GetBasicRow :69-77 */
/* (kind 0 dual / 1 primal, leaveRow, enterCol) of every pivot since creation; *count = total */
int lpr_sens_log_read(lpr_sens* s, int32_t* triples, int64_t cap, int64_t* count);
/* out[j] = (init ? init[j] : 0) + sum_{i<nw, in order} w[i] * tableau[i+1, j], j < ncols; nw must
 * be rows-1.  The order-faithful column sums of :636-645 and PerformDuality :690-694. */
int lpr_sens_column_fold(lpr_sens* s, const double* w, int32_t nw, const double* init,
                         int32_t ncols, double* out);
int lpr_sens_resolve_all(lpr_sens* s, int32_t* outcome);                       /* :203-208 */
/* ChangeNonBasicReducedCost :300-321 (index 0-based, new_cbar is the new Z-C entry) */
int lpr_sens_change_nonbasic_cbar(lpr_sens* s, int32_t index, double new_cbar, int32_t* outcome);
int lpr_sens_change_basic(lpr_sens* s, int32_t col, double delta, int32_t* outcome); /* :362-393 */
/* ChangeRHS :427-470 (k = constraint 1..rows-1, new_b replaces the CURRENT tableau RHS) */
int lpr_sens_change_rhs(lpr_sens* s, int32_t k, double new_b, int32_t* outcome);
int lpr_sens_change_nonbasic_column(lpr_sens* s, int32_t row, int32_t col, double new_val,
                                    int32_t* outcome);                          /* :502-531 */
int lpr_sens_add_activity(lpr_sens* s, double c_new, const double* a_new, int32_t na,
                          int32_t* outcome);                                    /* :534-584 */
/* AddNewConstraintNonInteractive :609-659 (tech has cols-1 entries, <= row) */
int lpr_sens_add_constraint(lpr_sens* s, const double* tech, int32_t ntech, double rhs,
                            int32_t* outcome);

/* The sensitivity report: what DisplayRangeNonBasic (:276-297), DisplayRangeBasic (:324-359),
 * DisplayRangeRHS (:396-424) and ShadowPrices (:212-222) compute, for every column and every
 * constraint of the analyzer's current state, from one read of the tableau on the device
 * (DESIGN.md section 18).  Max / Min are .NET Framework's Math.Max / Math.Min (a NaN sticks, of
 * equal values the later one in scan order is kept: +0 against -0), every quotient is IEEE
 * division.  What column j is: */
enum lpr_sens_range_kind {
    LPR_SENS_RANGE_NONBASIC_RANGE = 0,       /* cbar > EPS: "can DECREASE by at most" :291-292     */
    LPR_SENS_RANGE_NONBASIC_BOUNDARY = 1,    /* |cbar| <= EPS: "at boundary" :293-294              */
    LPR_SENS_RANGE_NONBASIC_NOT_OPTIMAL = 2, /* otherwise (negative or NaN cbar): "Warning" :295-296 */
    LPR_SENS_RANGE_BASIC = 3,                /* in basicVars, with a basic row :330-336            */
    LPR_SENS_RANGE_BASIC_ROW_NOT_FOUND = 4   /* in basicVars, GetBasicRow gives -1 :337            */
};
/* Per column j < cols - 1 (each array cols - 1 long):
 *   kind          an lpr_sens_range_kind; basicVars.Contains(j) decides basic (:282 :330)
 *   var_row       GetBasicRow(j) (:69-84) when j is in basicVars, else -1
 *   reduced_cost  tableau[0, j] (:288)
 *   cost_lo / hi  deltaLower / deltaUpper of :340-355 over row var_row for kind BASIC;
 *                 -inf / +inf for every other kind
 * Per constraint k = 1 .. rows - 1, at index k - 1 (each array rows - 1 long), slack column
 * s = n + k - 1 (:62-67):
 *   shadow        tableau[0, s] (:212-222, :404)
 *   rhs_lo / hi   deltaLower / deltaUpper of :406-418 down column s
 *   rhs_now       tableau[k, cols - 1] (:420)
 * Any output pointer may be NULL.  The call changes nothing of the analyzer: tableau, basicVars,
 * pivot log, solution vector and Z stay as they are.  A shape with n = cols - rows < 0 (the C#
 * would index out of range) is LPR_BAD_ARGUMENT and nothing is written. */
int lpr_sens_ranging(lpr_sens* s, int32_t* kind, int32_t* var_row, double* reduced_cost,
                     double* cost_lo, double* cost_hi, double* shadow, double* rhs_lo,
                     double* rhs_hi, double* rhs_now);
/* Device time in milliseconds of the two kernels of the last lpr_sens_ranging call on this handle
 * (the sweep over the tableau, the finish that folds the partials), from events; LPR_BAD_ARGUMENT
 * before the first call.  Either may be NULL. */
int lpr_sens_ranging_times(lpr_sens* s, double* sweep_ms, double* finish_ms);

/* ------------------------------------------------------------------------------------------
 * Knapsack, menu option 5 (Program.cs:430-470).  The reference calls two classes it never
 * defines (KnapsackBranchBoundSimplex; KnapsackBranchBoundSolver.cs is an empty class), so the
 * rules are fixed in DESIGN.md section 11 and restated in tests/ref_py_knapsack.py. */

/* KnapsackBranchBoundSolver.Solve(capacity, weights, values) (Program.cs:465): the 0/1 DP over an
 * int64 row initialised to 0, *best = dp[capacity].  capacity < 0 or a weight < 0:
 * LPR_BAD_ARGUMENT.  opts may be NULL; variant 0 = blocked LDS passes where the item weights fit
 * the halo, 1 = one streaming pass per item (benchmarks and tests only, same result). */
typedef struct lpr_knap_dp_opts {
    int32_t variant;
    int32_t reserved;
} lpr_knap_dp_opts;
int lpr_knap_dp(lpr_engine* e, int64_t capacity, const int32_t* weights, const int32_t* values,
                int32_t n, const lpr_knap_dp_opts* opts, int64_t* best);

typedef struct lpr_knap lpr_knap;
/* new KnapsackBranchBoundSimplex(capacity, weights, values) (Program.cs:443-447): integral
 * doubles, 1 <= w_i <= 2^31-1, 0 <= v_i <= 2^31-1, capacity >= 0, 1 <= n <= 8192; anything else
 * is LPR_BAD_ARGUMENT naming the offending index.  Ranks the items by v/w (exact cross products,
 * ties to the lower index) and uploads them in rank order. */
int lpr_knap_bb_create(lpr_engine* e, int64_t capacity, const double* weights,
                       const double* values, int32_t n, lpr_knap** out);
int lpr_knap_bb_destroy(lpr_knap* k);

typedef struct lpr_knap_bb_opts {
    int64_t node_cap;  /* evaluated nodes; <= 0: 2^22.  A level is evaluated only if the total
                          stays within it, else LPR_BB_NODE_CAP with the incumbent so far */
    int32_t narrate;   /* node records kept for lpr_knap_bb_nodes_read: 0 none, > 0 the first
                          `narrate` nodes, < 0 auto (4096 when n <= 64, else none) */
    int32_t reserved;
} lpr_knap_bb_opts;

typedef struct lpr_knap_bb_result {
    int32_t status;     /* LPR_OK_OPTIMAL or LPR_BB_NODE_CAP */
    int32_t found;      /* an incumbent exists (always, once the root was evaluated) */
    double z;           /* Z* (Solve(), Program.cs:449) */
    int64_t evaluated;  /* nodes evaluated */
    int64_t widest;     /* widest level evaluated */
    int32_t levels;     /* levels evaluated */
    int32_t reserved;
} lpr_knap_bb_result;

/* Solve() (Program.cs:449): the level-synchronous search on the device; opts may be NULL. */
int lpr_knap_bb_solve(lpr_knap* k, const lpr_knap_bb_opts* opts, lpr_knap_bb_result* res);
/* rank[p] = original index of the item at rank position p (n entries) */
int lpr_knap_bb_rank_read(lpr_knap* k, int32_t* rank);
/* GetSelectedItemsOriginal() (Program.cs:455): the incumbent's items, ascending original index;
 * ids holds n entries, *count is set */
int lpr_knap_bb_selected_read(lpr_knap* k, int32_t* ids, int32_t* count);
int lpr_knap_bb_stats(lpr_knap* k, int32_t* levels, int64_t* evaluated, int64_t* widest);
/* PrintIterations() (Program.cs:452): node records of the last solve in evaluation order (record
 * 0 = root): parent record (-1 root), branch (0: x_k = 0, 1: x_k = 1), status (0 fractional,
 * 1 fractional pruned, 2 integral, 3 infeasible), bound, k (ORIGINAL index of the critical item,
 * -1 when integral or infeasible), V.  *count = records kept (<= cap). */
int lpr_knap_bb_nodes_read(lpr_knap* k, int32_t* parent, int32_t* branch, int32_t* status,
                           double* bound, int32_t* kitem, int64_t* value, int64_t cap,
                           int64_t* count);

/* ------------------------------------------------------------------------------------------
 * Batched primal simplex.  One handle holds `count` independent LPs; one
 * solve call runs PrimalSimplexSolver's loop for every LP on the device, with its rules per LP
 * bit for bit: each LP ends with the bytes lpr_primal_solve (and the oracle) give for it alone.
 * Shapes up to 1024 rows x 2048 columns (form H); a larger LP is LPR_BAD_ARGUMENT, to be solved
 * alone with lpr_primal_solve.  The reference has no batch mode; every call cites the C# lines
 * it repeats per LP. */
typedef struct lpr_batch lpr_batch;

/* new PrimalSimplexSolver(objective, constraints, isMaximization) per LP
 * (Simplex/PrimalSimplexSolver.cs:27-87), built on the device with the bytes of
 * lpr_tableau_from_lp.  count LPs; n[k], m[k] >= 0 with n[k] + m[k] >= 1; objective packed by
 * n[k]; A packed as m[k] x n[k] row-major blocks; ncoef (NULL: full rows; else in [0, n[k]]),
 * relation (LPR_REL_LE/GE/EQ) and rhs packed by m[k]; is_max per LP.  log_cap: pivot-log pairs
 * kept per LP (0: 4 * (rows + cols), at most 4096). */
int lpr_batch_from_lps(lpr_engine* e, int32_t count, const int32_t* n, const int32_t* m,
                       const double* objective, const double* A, const int32_t* ncoef,
                       const int8_t* relation, const double* rhs, const int8_t* is_max,
                       int32_t log_cap, lpr_batch** out);
/* Ready tableaux (lpr_tableau_create per LP, BranchAndBoundAdapter.cs:31-46) packed as
 * rows[k] x cols[k] row-major blocks; basis packed by rows[k] - 1 (NULL: -1).  The decision
 * variables of LP k are its first max(0, cols[k] - rows[k]) columns ([A | I | b]). */
int lpr_batch_create(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                     const double* tableaux, const int32_t* basis, int32_t log_cap,
                     lpr_batch** out);
int lpr_batch_destroy(lpr_batch* b);

typedef struct lpr_batch_opts {
    int64_t max_pivots;  /* per LP, per call, as in lpr_primal_solve (<= 0: uncapped) */
    int32_t chunk;       /* pivots per LP per launch (0: by form) */
    int32_t variant;     /* 0 auto; 1 / 2 / 3 force form W / G / H on the LPs that fit it (tests
                            and tuning only, same bits) */
} lpr_batch_opts;

typedef struct lpr_batch_result {
    int32_t optimal, unbounded, limit;  /* LPs in each state after this call */
    int32_t launches;                   /* solve kernels launched by this call */
    int64_t pivots;                     /* pivots performed by this call, all LPs */
} lpr_batch_result;

/* PrimalSimplexSolver.Solve() (:102-150) for every LP not yet finished: FindEnteringVariable
 * (:152-167) -> FindLeavingVariable (:169-191) -> Pivot (:193-211) -> basicVariables[r-1] = e
 * (:142) until optimal / unbounded / max_pivots.  An LP at LPR_PIVOT_LIMIT resumes on the next
 * call; finished LPs stay finished.  Returns LPR_OK_OPTIMAL unless the call itself failed. */
int lpr_batch_solve(lpr_batch* b, const lpr_batch_opts* opts, lpr_batch_result* res);
/* Status, pivots so far (C# `iteration`, :138) and T[0, cols-1] (FinalZ, :113: the host mirror
 * keeps 0 on the unbounded exit) of every LP; count entries each, any may be NULL. */
int lpr_batch_status_read(lpr_batch* b, int32_t* status, int64_t* pivots, double* z);
/* ExtractSolution() (:213-252) of every LP, packed by n[k]; 0 for LPs that are not optimal. */
int lpr_batch_solution_read(lpr_batch* b, double* x);
/* basicVariables (:18-24) of every LP, packed by rows[k] - 1 (m[k]). */
int lpr_batch_basis_read(lpr_batch* b, int32_t* basis);
/* Pivot log of LP k, row 1-based as at :138: *count = min(pivots, log_cap, cap) pairs. */
int lpr_batch_log_read(lpr_batch* b, int32_t k, int32_t* rows, int32_t* cols, int64_t cap,
                       int64_t* count);
/* GetFinalTableau() (:269-278) of LP k: rows[k] x cols[k] row-major. */
int lpr_batch_tableau_read(lpr_batch* b, int32_t k, double* rowmajor);
/* rows, cols and decision variables n of LP k; any may be NULL. */
int lpr_batch_shape(lpr_batch* b, int32_t k, int32_t* rows, int32_t* cols, int32_t* n);

/* Traced batches: the solve also stores, per LP, the tableau after every
 * pivot in device memory -- the numbers of PrimalSimplexSolver's IterationSnapshots, "Initial
 * Tableau" (:86) and "Iteration i - After pivot" (:148); the host only formats.  Record i of an LP
 * is its state after i pivots, 2 + rows * cols doubles, indices stored as doubles:
 *   [0] leavingRow of pivot i (1-based, as logged at :138)  [1] enteringCol of pivot i
 *   T[rows x cols] row-major: the tableau after pivot i
 * Record 0 is the tableau as built or uploaded, its header -1, -1.  An LP has 1 + pivots records
 * and keeps the first min(., trace_cap); a record index >= trace_cap is counted, not written.
 * The C#'s list holds one more entry when the LP is optimal (:118-122) or unbounded (:133): that
 * one is formatted from lpr_batch_tableau_read, so it survives a small trace_cap.  PARITY: every
 * record is the bytes of the single-model path's tableau at that point, and everything else a
 * traced batch ends with is the bytes of the untraced batch.
 *
 * lpr_batch_trace_reserve makes the handle traced: it allocates trace_cap records per LP,
 * zero-filled, and writes record 0 of every LP.  Only before the handle's first solve:
 * LPR_BAD_ARGUMENT with a message afterwards, when called twice, or for trace_cap < 1.  A failed
 * allocation, or a slab beyond an int64 count of bytes, is LPR_OUT_OF_MEMORY and the message
 * names the buffer and its size; the handle stays usable and untraced.  opts and result of
 * lpr_batch_solve are unchanged. */
int lpr_batch_trace_reserve(lpr_batch* b, int32_t trace_cap);
/* Per LP (count entries each, any may be NULL): records, the exact number 1 + pivots (:137; may
 * exceed trace_cap, min(records, trace_cap) are kept); offset, where LP k's records start in the
 * trace slab, in doubles; stride, the doubles of one record. */
int lpr_batch_trace_info(lpr_batch* b, int64_t* records, int64_t* offset, int64_t* stride);
/* Records [first, first + n) of LP k (:86, :148) into out[n * stride]; a range beyond the kept
 * records is LPR_BAD_ARGUMENT. */
int lpr_batch_trace_read(lpr_batch* b, int32_t k, int64_t first, int64_t n, double* out);
/* The whole trace slab (trace_cap * sum of the strides doubles: every LP's :86 and :148 tableaux)
 * in one copy; cap_doubles is what `out` holds, LPR_BAD_ARGUMENT when it is too small.  Every
 * trace read on an untraced or orphaned handle is LPR_BAD_ARGUMENT with a message. */
int lpr_batch_trace_read_all(lpr_batch* b, double* out, int64_t cap_doubles);


/* ------------------------------------------------------- batched branch and bound */

/* Many independent integer programs per device call.  Every IP runs the
 * whole BranchAndBound.ExecuteBranchAndBound (IntegerProgramming/BranchBoundSimplexSolver.cs:
 * 1006-1233) on the device, with no host step per node, and gives the bits lpr_bb_run gives for
 * that root alone.  One IP per wave (form W) or per workgroup (G: its working pair in LDS, H: in
 * HBM), picked by the footprint of the child LP at full depth; the DFS stack stays in HBM.  The
 * reference has no batch mode; every call cites the C# lines it repeats per IP. */
typedef struct lpr_bb_batch lpr_bb_batch;

/* BranchAndBoundAdapter.SolveFromPrimal's set-up (BranchAndBoundAdapter.cs:9-24) per IP: root k is
 * the rows[k] x cols[k] row-major block of `tableaux` (packed), SetNumVars(nvars[k]) with nvars[k]
 * in [0, cols[k] - 1].  node_cap: the hard stop of :1038-1042 for every IP (<= 0: 20, at most 64);
 * each IP's shape at full depth, (rows + node_cap) x (cols + node_cap), must stay within 1024 x
 * 2048.  trace_cap: pivot-trace quads kept per IP (<= 0: 256; the count is always exact). */
int lpr_bb_batch_create(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                        const double* tableaux, const int32_t* nvars, int32_t node_cap,
                        int32_t trace_cap, lpr_bb_batch** out);
/* SolveFromPrimal (:9-24) for every LP of a solved lpr_batch, its FinalTableau copied device to
 * device: nvars = n[k] for an optimal LP (SolutionVector.Count), max(1, cols - 1) for an unbounded
 * one (InferNumVariables).  An LP without a FinalTableau (LPR_PIVOT_LIMIT, or never solved) makes
 * the call fail with LPR_BAD_ARGUMENT naming it.  The new handle does not depend on `lps`. */
int lpr_bb_batch_from_batch(lpr_batch* lps, int32_t node_cap, int32_t trace_cap,
                            lpr_bb_batch** out);
int lpr_bb_batch_destroy(lpr_bb_batch* b);

typedef struct lpr_bb_batch_opts {
    int32_t enable_pruning;   /* ShouldPrunebranch (:985-1004); Program.cs:389 passes false */
    int32_t chunk;            /* pops per IP per launch (0: by form) */
    int32_t variant;          /* 0 auto; 1 / 2 / 3 force form W / G / H on the IPs that fit it
                                 (tests and tuning only, same bits) */
    int32_t max_child_pivots; /* pivots one child LP may take before its IP ends with
                                 LPR_PIVOT_LIMIT (0: 65 536) */
} lpr_bb_batch_opts;

typedef struct lpr_bb_batch_result {
    int32_t done;        /* IPs whose stack emptied (LPR_OK_OPTIMAL) */
    int32_t node_cap;    /* IPs stopped by the node cap (LPR_BB_NODE_CAP) */
    int32_t pivot_limit; /* IPs ended by a child LP over max_child_pivots (LPR_PIVOT_LIMIT) */
    int32_t launches;    /* search kernels launched by this call */
    int64_t pops;        /* nodes popped (branchCount, :1045), all IPs */
    int64_t pivots;      /* pivot-trace entries, all IPs */
} lpr_bb_batch_result;

/* ExecuteBranchAndBound (:1006-1233) for every IP, from its root: RoundAllTableaux (:1021), DFS
 * stack, on each pop RoundAllTableaux (:1047), GetObjective (:892-897), ShouldPrunebranch,
 * UpdateOptimalSolution (:935-983), CreateBranches (:859-890); lower child then upper, each
 * AddConstraint (:694-803) + DoDualSimplex (:289-468); the solved ones rounded (:1124, :1187) and
 * pushed upper first (:1210-1213).  A second call starts again from the roots.  Returns
 * LPR_OK_OPTIMAL unless the call itself failed; each IP's status is in lpr_bb_batch_result_read. */
int lpr_bb_batch_run(lpr_bb_batch* b, const lpr_bb_batch_opts* opts, lpr_bb_batch_result* res);
/* lpr_bb_result's fields per IP, count entries each, any pointer may be NULL: status
 * (LPR_OK_OPTIMAL / LPR_BB_NODE_CAP / LPR_PIVOT_LIMIT), found, processed, best_node, z
 * (optimalValue, -inf if none), pivots, nodes_created. */
int lpr_bb_batch_result_read(lpr_bb_batch* b, int32_t* status, int32_t* found, int64_t* processed,
                             int32_t* best_node, double* z, int64_t* pivots,
                             int64_t* nodes_created);
/* The incumbent x of every IP (:1059-1066), packed by nvars[k]; 0 where none was found. */
int lpr_bb_batch_solution_read(lpr_bb_batch* b, double* x);
/* Node records of IP k, as lpr_bb_records_read (a child that hit max_child_pivots has status
 * LPR_PIVOT_LIMIT). */
int lpr_bb_batch_records_read(lpr_bb_batch* b, int32_t k, int32_t* parent, int32_t* kind,
                              int32_t* depth, int32_t* var, double* bound, int32_t* status,
                              double* z, int64_t cap, int64_t* count);
/* Record ids of IP k in the order they were popped, as lpr_bb_pop_order_read. */
int lpr_bb_batch_pop_order_read(lpr_bb_batch* b, int32_t k, int32_t* ids, int64_t cap,
                                int64_t* count);
/* Pivot trace of IP k, as lpr_bb_trace_read: *count = min(pivots, trace_cap, cap) quads. */
int lpr_bb_batch_trace_read(lpr_bb_batch* b, int32_t k, int32_t* quads, int64_t cap,
                            int64_t* count);

/* A NARRATED batch also keeps, per IP, the numbers behind everything
 * ExecuteBranchAndBound writes to the console (:1006-1233), written by the search kernel itself:
 *   - per child record, the list DoDualSimplex returns (:292, :341, :388): the tableau
 *     AddConstraint hands it, then one per pivot, each (rows + depth) x (cols + depth) doubles,
 *     row-major, unrounded, back to back and compact in the IP's slice of one slab; a last tableau
 *     dropped by :392-400 (trace phase 2) is dropped here too;
 *   - per pop, objVal (:892-897), the nvars decision values (:899-921) and a flag word: bit 0
 *     scored (not pruned, :985-1004), bit 1 every value integer, bit 2 became the incumbent;
 *   - the incumbent's tableau (bestTableau of UpdateOptimalSolution :935-983, printed at :1221).
 * Results, records, pop order, trace and solution are those of an un-narrated batch.
 *
 * lpr_bb_batch_narrate_reserve makes the handle narrated: cap_doubles[k] >= 0 is the doubles of
 * child tableaux IP k may keep.  A tableau that does not fit whole is counted and not written, and
 * so is every later one of that IP: what is kept is a prefix, and the totals stay exact.  It may
 * be called again between runs (read the exact needs with lpr_bb_batch_narrate_info, reserve
 * them, run again: a run is deterministic); the old slab is freed first.  LPR_BAD_ARGUMENT: NULL,
 * an entry below 0, an orphaned handle.  LPR_OUT_OF_MEMORY names the buffer and its size and
 * leaves the handle usable and un-narrated. */
int lpr_bb_batch_narrate_reserve(lpr_bb_batch* b, const int64_t* cap_doubles);
/* Per IP, count entries each, any pointer may be NULL: tableaux and doubles the child LPs of the
 * last run made (exact), doubles kept, and the start of the IP's slice in the slab. */
int lpr_bb_batch_narrate_info(lpr_bb_batch* b, int64_t* tableaux, int64_t* doubles_made,
                              int64_t* doubles_kept, int64_t* offset);
/* The pops of IP k in pop order (:1045-1076): *count = min(processed, cap); flags and z one per
 * pop, vals nvars per pop (undefined for a pruned pop); any of the three may be NULL. */
int lpr_bb_batch_narrate_pops_read(lpr_bb_batch* b, int32_t k, int32_t* flags, double* z,
                                   double* vals, int64_t cap, int64_t* count);
/* One entry per record of IP k: tab_off (doubles from the IP's slice start) and ntab, the
 * tableaux of its DoDualSimplex list (made; the kept ones are those below doubles_kept).  The
 * root has ntab 0. */
int lpr_bb_batch_narrate_children_read(lpr_bb_batch* b, int32_t k, int64_t* tab_off,
                                       int32_t* ntab, int64_t cap, int64_t* count);
/* Doubles [first_double, first_double + n) of IP k's slice, what DisplayTableau (:623-640) is
 * given; a range beyond what is kept is refused. */
int lpr_bb_batch_narrate_tableaux_read(lpr_bb_batch* b, int32_t k, int64_t first_double,
                                       int64_t n, double* out);
/* The whole slab (the sum of cap_doubles) in one copy; cap_doubles is what `out` holds. */
int lpr_bb_batch_narrate_read_all(lpr_bb_batch* b, double* out, int64_t cap_doubles);
/* The incumbent's tableau of IP k (:935-983, :1221), rows x cols; out may be NULL to ask for the
 * shape.  LPR_BAD_ARGUMENT if IP k has no incumbent. */
int lpr_bb_batch_narrate_best_read(lpr_bb_batch* b, int32_t k, double* out, int32_t* rows,
                                   int32_t* cols);


/* ------------------------------------------------------- sensitivity scenario batch */

/* One solved model, many what-if scripts per device call.  A scenario is a
 * private copy of a base analyzer's state -- the tableau, basicVars as stored, finalZ and
 * solutionVector (SensitivityAnalysis/SensitivityAnalyzer.cs:14-18) -- plus a script: an ordered
 * list of edits applied to that copy on the device, with no host step per edit or per pivot.
 * Scenario k ends with the state and the reports a fresh lpr_sens handle holding the base state
 * gives when the same edits are called on it one after another.  One 256-lane workgroup per
 * scenario, its tableau in LDS (form G) or in its slice of a global slab (form H, up to 1024 x
 * 2048).  The reference has no batch mode; every call cites the C# lines it repeats per scenario. */
typedef struct lpr_sens_batch lpr_sens_batch;

/* Ops 0..4 keep the tableau's shape and are what lpr_sens_batch_create takes.  AddNewActivity
 * (:534-584) and AddNewConstraint (:609-659) grow it: a batch from lpr_sens_batch_create_grow
 * takes them too, with the new column or row in that call's payload pool. */
enum lpr_sens_edit_op {
    LPR_SENS_EDIT_RESOLVE_ALL = 0,     /* ResolveAll :203-208; no arguments                       */
    LPR_SENS_EDIT_NONBASIC_CBAR = 1,   /* ChangeNonBasicReducedCost :300-321; a = index, v = new  */
    LPR_SENS_EDIT_BASIC = 2,           /* ChangeBasic :362-393; a = col, v = delta                */
    LPR_SENS_EDIT_RHS = 3,             /* ChangeRHS :427-470; a = k, v = new b                    */
    LPR_SENS_EDIT_NONBASIC_COLUMN = 4, /* ChangeNonBasicColumn :502-531; a = row, b = col, v = new */
    LPR_SENS_EDIT_ADD_ACTIVITY = 5,    /* AddNewActivity :534-584; v = c_new, the column a_new is
                                          payload[a .. a + b)                                      */
    LPR_SENS_EDIT_ADD_CONSTRAINT = 6   /* AddNewConstraint :609-659; v = rhs, tech is
                                          payload[a .. a + b), b = ntech                           */
};

typedef struct lpr_sens_edit {
    int32_t op, a, b, reserved;
    double v;
} lpr_sens_edit;

/* count scenarios on the state `base` holds now (:22-39 is not run again: basicVars is taken as
 * stored, stale entries included).  Script k is nedits[k] >= 0 entries of `edits`, packed; 0 edits
 * is the base state.  An unknown op, or one that changes the shape, is LPR_BAD_ARGUMENT; an index
 * out of range is not: that edit reports LPR_SENS_INVALID_INDEX and changes nothing.  The base
 * must be within 1024 x 2048.  log_cap: pivot-log triples kept per scenario (0: 4 * (rows +
 * cols), at most 4096; the count is always exact).  The base is only read, and may be destroyed
 * once this call has returned. */
int lpr_sens_batch_create(lpr_sens* base, int32_t count, const int32_t* nedits,
                          const lpr_sens_edit* edits, int32_t log_cap, lpr_sens_batch** out);
/* lpr_sens_batch_create plus ops 5 and 6, so a scenario's tableau can grow as its script runs.
 * `payload` (npayload doubles, copied; NULL only with npayload 0) holds the vectors those edits
 * point into.  LPR_BAD_ARGUMENT, naming the scenario and the edit: a payload range outside
 * [0, npayload), a negative b, npayload above 2^31 - 1, or a script whose largest possible shape
 * -- the base's rows plus its add-constraint edits, by the base's columns plus its add edits of
 * both kinds -- is past 1024 x 2048.  Every array of the batch is sized by the largest such
 * shape over all scripts, and that shape picks the form.
 *   ADD_ACTIVITY   with b != rows - 1 reports LPR_SENS_INVALID_INDEX and changes nothing (the
 *                  batch's one rule of its own: lpr_sens_add_activity refuses that call)
 *   ADD_CONSTRAINT with b != cols - 1 reports LPR_SENS_INVALID_INDEX (:616-617); with a stored
 *                  basicVars entry outside [0, b) LPR_SENS_INDEX_OUT_OF_RANGE; neither changes
 *                  anything.  aX (:647-651) reads solutionVector as stored, stale after an edit
 *                  that did not end OK.
 * The shape grows before the re-solve and stays grown whatever its outcome. */
int lpr_sens_batch_create_grow(lpr_sens* base, int32_t count, const int32_t* nedits,
                               const lpr_sens_edit* edits, const double* payload,
                               int64_t npayload, int32_t log_cap, lpr_sens_batch** out);
/* Many solved models, one script each: scenario k is a fresh analyzer on LP item[k] of a solved
 * lpr_batch -- new SensitivityAnalyzer(GetFinalTableau(), SolutionVector, FinalZ, BasicVariables)
 * (Program.cs:147-151, SensitivityAnalyzer.cs:22-39), run per scenario on the device -- followed by
 * script k (ops 0..6, payload rules as in lpr_sens_batch_create_grow).  The state it starts from:
 * the LP's final tableau; solutionVector = ExtractSolution() over the LP's n
 * (PrimalSimplexSolver.cs:213-249), so solutionVector.Count = n; finalZ = tableau[0, cols - 1];
 * basicVars from RebuildBasicsFromTableau (:35, :706-723: the first qualifying column per row, -1
 * where none), not the LP batch's stored basis.  item == NULL means item[k] = k, and count must
 * then be the LP batch's count; otherwise an index may repeat (several scripts on one model) and
 * the order is free.
 * The handle is an ordinary lpr_sens_batch whose scenarios have their own shapes, reported as in
 * a grow batch (lpr_sens_batch_shape_read; state_read packs basicVars by max_rows - 1).  Every
 * array is sized by the largest shape any scenario can reach, so one large LP sizes every slice
 * and picks the form: group mixed batches by size.  lpr_sens_batch_info's rows and cols report the
 * largest base shape over the chosen LPs.
 * LPR_BAD_ARGUMENT, naming the scenario and the item, with nothing allocated: a null or orphaned
 * LP batch, count < 1, an item outside the batch, an item whose status is not LPR_OK_OPTIMAL (an
 * unbounded LP has no SolutionVector, PrimalSimplexSolver.cs:129-135; a running or pivot-limited
 * one no final tableau), an item with cols < rows (as lpr_sens_create), a script that can grow its
 * own base past 1024 x 2048, and the payload and op errors of lpr_sens_batch_create_grow.
 * Synchronous: the LP batch (only read), the edits and the payload may go once it has returned. */
int lpr_sens_batch_from_batch(lpr_batch* lps, int32_t count, const int32_t* item,
                              const int32_t* nedits, const lpr_sens_edit* edits,
                              const double* payload, int64_t npayload, int32_t log_cap,
                              lpr_sens_batch** out);
/* Device time in milliseconds of the constructor kernel of the lpr_sens_batch_from_batch call that
 * made this handle, from events; LPR_BAD_ARGUMENT on a handle of another create. */
int lpr_sens_batch_from_batch_time(lpr_sens_batch* b, double* kernel_ms);
int lpr_sens_batch_destroy(lpr_sens_batch* b);

typedef struct lpr_sens_batch_opts {
    int64_t max_pivots;  /* per scenario, per call (<= 0: only the C#'s own 10 001 per loop) */
    int32_t chunk;       /* pivots per scenario per launch (0: by form) */
    int32_t variant;     /* 0 auto; 2 / 3 force form G / H where the base fits it (tests and tuning
                            only, same bits); ignored while scenarios are stopped inside an edit */
} lpr_sens_batch_opts;

typedef struct lpr_sens_batch_result {
    int32_t finished;  /* scenarios whose script has ended */
    int32_t running;   /* scenarios stopped by max_pivots; the next call resumes them */
    int32_t launches;  /* script kernels launched by this call */
    int32_t form;      /* the form this call ran: 1 G, 2 H */
    int64_t pivots;    /* pivots performed by this call, all scenarios */
} lpr_sens_batch_result;

/* Every script, edit after edit: the edit itself (:300-321, :362-393, :427-470 with its snapshot
 * and rollback, :502-531), RebuildBasicsFromTableau (:706-723), DualSimplexIfNeeded (:168-201),
 * ReOptimize (:121-166), Pivot (:98-119).  A script goes on after an edit that did not end OK.
 * A scenario stopped by max_pivots -- inside an edit, inside the dual phase -- resumes on the
 * next call; finished scenarios stay finished.  opts may be NULL.  Returns LPR_OK_OPTIMAL unless
 * the call itself failed. */
int lpr_sens_batch_run(lpr_sens_batch* b, const lpr_sens_batch_opts* opts,
                       lpr_sens_batch_result* res);
/* count, numRows, numCols, edits of all scripts together, the pivot-log capacity per scenario and
 * the form of the last run (0 before the first); any may be NULL.  rows x cols is the base's shape;
 * in a batch from lpr_sens_batch_from_batch the largest base shape over the chosen LPs. */
int lpr_sens_batch_info(lpr_sens_batch* b, int32_t* count, int32_t* rows, int32_t* cols,
                        int64_t* total_edits, int32_t* log_cap, int32_t* form);
/* rows[k] x cols[k]: the shape of scenario k as of the last run (the base's, where nothing has
 * grown it); max_rows x max_cols: the largest shape a script of this batch can reach, which the
 * strides of the bulk reads are sized by.  Any may be NULL. */
int lpr_sens_batch_shape_read(lpr_sens_batch* b, int32_t* rows, int32_t* cols, int32_t* max_rows,
                              int32_t* max_cols);
/* Per edit, packed as the scripts are: the lpr_sens_outcome (-100 for an edit that has not ended)
 * and its pivots (what lpr_sens_shape's last_pivots gives after that edit); either may be NULL. */
int lpr_sens_batch_outcomes_read(lpr_sens_batch* b, int32_t* outcome, int64_t* pivots);
/* CurrentZ :728 and solutionVector.Count per scenario, basicVars packed by rows - 1; any may be
 * NULL.  In a grow batch basicVars is packed by max_rows - 1 (lpr_sens_batch_shape_read), and the
 * entries past a scenario's own rows - 1 are INT32_MIN. */
int lpr_sens_batch_state_read(lpr_sens_batch* b, double* z, int32_t* nsol, int32_t* basic);
/* CurrentSolutionVector :729 of scenario k: *count entries, the first min(*count, cap) copied. */
int lpr_sens_batch_solution_read(lpr_sens_batch* b, int32_t k, double* x, int32_t cap,
                                 int32_t* count);
/* CurrentTableau :727 of scenario k: rows x cols row-major, at the scenario's own shape. */
int lpr_sens_batch_tableau_read(lpr_sens_batch* b, int32_t k, double* rowmajor);
/* (kind 0 dual / 1 primal, leaveRow, enterCol) of scenario k's pivots, as lpr_sens_log_read:
 * *count = all of them, the first min(*count, log_cap, cap) copied. */
int lpr_sens_batch_log_read(lpr_sens_batch* b, int32_t k, int32_t* triples, int64_t cap,
                            int64_t* count);
/* The sensitivity report of every scenario in one call: per scenario the
 * nine outputs of lpr_sens_ranging -- DisplayRangeNonBasic :276-297, DisplayRangeBasic :324-359,
 * DisplayRangeRHS :396-424, ShadowPrices :212-222, GetBasicRow / IsPivotColumn :69-84 -- on the
 * state the batch holds for it now: the tableau lpr_sens_batch_tableau_read gives, basicVars as
 * stored (lpr_sens_batch_state_read; stale entries are kept, nothing is rebuilt) and the
 * scenario's own shape.  Valid before the first run (every scenario is the base state), after a
 * run, and between two runs on scenarios stopped inside an edit (LPR_PIVOT_LIMIT).
 * kind, var_row, reduced_cost, cost_lo, cost_hi are count x (max_cols - 1), shadow, rhs_lo,
 * rhs_hi, rhs_now are count x (max_rows - 1), max_rows / max_cols those of
 * lpr_sens_batch_shape_read (the base's shape in a fixed-shape batch); scenario k owns row k of
 * each.  Entries past scenario k's own cols[k] - 1 or rows[k] - 1 are INT32_MIN in the int arrays
 * and a quiet NaN in the double arrays.  Any output pointer may be NULL.  The call changes nothing
 * of the batch: a following lpr_sens_batch_run resumes as if it had not been made. */
int lpr_sens_batch_ranging(lpr_sens_batch* b, int32_t* kind, int32_t* var_row,
                           double* reduced_cost, double* cost_lo, double* cost_hi, double* shadow,
                           double* rhs_lo, double* rhs_hi, double* rhs_now);
/* Device time in milliseconds of the kernel of the last lpr_sens_batch_ranging call on this
 * handle, from events; LPR_BAD_ARGUMENT before the first call. */
int lpr_sens_batch_ranging_time(lpr_sens_batch* b, double* kernel_ms);


/* ------------------------------------------------------------- cutting-plane batch */

/* Many option-4 tableaux per device call.  One handle holds `count`
 * independent tableaux (row 0 = objectiveRow, rows 1.. = constraintRows, what lpr_cutting_plane
 * takes); one run call takes every item through the whole CuttingPlaneSolution recursion
 * (IntegerProgramming/CuttingPlaneSolver.cs:64-229) on the device: the Gomory cut, the pivot on
 * it, the dual and primal clean-up solves and the decision to cut again, with no host step per
 * cut or per pivot.  Item k ends with the exit code, the cuts, the log and the grown tableau that
 * lpr_cutting_plane gives for it alone on a fresh lpr_tableau.  One 256-lane workgroup per item,
 * its tableau in LDS (form G) or in its slice of a global slab (form H), picked per item by the
 * tableau at full row capacity.  The reference has no batch mode; every call cites the C# lines
 * it repeats per item. */
typedef struct lpr_cut_batch lpr_cut_batch;

/* objectiveRow and constraintRows per item (:64-70): packed rows[k] x cols[k] row-major blocks.
 * max_cuts is the row capacity added per item over the handle's life (<= 0: 64, as in
 * lpr_cutting_plane).  rows[k] >= 2 (ArgumentException :68), cols[k] >= 2, rows[k] + max_cuts <=
 * 1024 and cols[k] <= 2048; anything else is LPR_BAD_ARGUMENT naming the item (a larger tableau
 * goes through lpr_cutting_plane).  log_cap: triples kept per item (0: 4 * (rows + max_cuts +
 * cols), at most 4096; the count is always exact). */
int lpr_cut_batch_create(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                         const double* tableaux, int32_t max_cuts, int32_t log_cap,
                         lpr_cut_batch** out);
/* The same from the FinalTableau of every LP of a solved lpr_batch (what option 4 cuts,
 * Program.cs:417-428), device to device.  An LP that was never solved or stopped at
 * LPR_PIVOT_LIMIT has none: LPR_BAD_ARGUMENT naming it.  The new handle does not depend on
 * `lps`. */
int lpr_cut_batch_from_batch(lpr_batch* lps, int32_t max_cuts, int32_t log_cap,
                             lpr_cut_batch** out);
/* After lpr_engine_close the handle is orphaned: every call but this one is LPR_BAD_ARGUMENT. */
int lpr_cut_batch_destroy(lpr_cut_batch* b);

typedef struct lpr_cut_batch_opts {
    int32_t mode;         /* 0 CuttingPlaneSolution :64-229; 1 DualSimplexSolver.Solve
                             (DualSimplex.cs:14-114); 2 PrimalSimplexSolver2.Solve
                             (PrimalSimplexSolver2.cs:46-97)                                     */
    int32_t max_cuts;     /* mode 0: cuts per item for this call (<= 0: all the capacity left)   */
    int64_t hard_cap;     /* extra pivot limit per inner solver run, as in the single calls
                             (<= 0: none)                                                        */
    int32_t max_iters;    /* modes 1, 2: maxIters (:108 / :90); mode 0 uses 10000 (:190, :200)   */
    int32_t print_steps;  /* modes 1, 2: `iter` advances only when set (:94 / :75); mode 0: set  */
    int32_t chunk;        /* pivots per item per launch (0: by form)       */
    int32_t variant;      /* 0 auto; 2 / 3 force form G / H on the items that fit (tests and
                             tuning only, same bits)                                             */
} lpr_cut_batch_opts;

typedef struct lpr_cut_batch_result {
    int32_t by_code[8];  /* items per exit code 0..7 (mode 0) or per lpr_status (modes 1, 2)     */
    int32_t launches;    /* kernels launched by this call                                        */
    int32_t items_g;     /* items this call ran in form G ...                                    */
    int32_t items_h;     /* ... and in form H                                                    */
    int32_t reserved;
    int64_t cuts;        /* cuts added by this call, all items                                   */
    int64_t pivots;      /* pivots performed by this call, all items and all three kinds         */
} lpr_cut_batch_result;

/* One call of lpr_cutting_plane (mode 0), lpr_dual_solve (mode 1) or lpr_primal2_solve (mode 2)
 * per item, on the tableau the last call left: logs append, rows stay grown, and a mode-0 call
 * adds at most min(opts.max_cuts, capacity left) cuts per item -- an item with none left ends
 * with exit 1 if all RHS are integral and with exit 6 otherwise, in that order.  opts may be NULL
 * (mode 0, every default).  Returns LPR_OK_OPTIMAL unless the call itself failed. */
int lpr_cut_batch_run(lpr_cut_batch* b, const lpr_cut_batch_opts* opts, lpr_cut_batch_result* res);
/* Per item: the exit code of lpr_cutting_plane (0..7, mode 0) or the lpr_status (modes 1, 2) of
 * the last call, its cuts, the rows now and the exact number of log triples; any may be NULL. */
int lpr_cut_batch_result_read(lpr_cut_batch* b, int32_t* code, int32_t* cuts, int32_t* rows,
                              int64_t* log_count);
/* Item k: rows now x cols, its row capacity and its log capacity; any may be NULL. */
int lpr_cut_batch_shape(lpr_cut_batch* b, int32_t k, int32_t* rows, int32_t* cols,
                        int32_t* row_cap, int32_t* log_cap);
/* Item k's own grown tableau: rows x cols row-major (lpr_cut_batch_shape). */
int lpr_cut_batch_tableau_read(lpr_cut_batch* b, int32_t k, double* rowmajor);
/* (kind 0 dual / 1 primal2 / 2 cut, row in the C#'s own numbering, column) of item k's pivots,
 * as lpr_cut_log_read: *count = all of them, the first min(*count, log_cap, cap) copied. */
int lpr_cut_batch_log_read(lpr_cut_batch* b, int32_t k, int32_t* triples, int64_t cap,
                           int64_t* count);
/* T[0, cols - 1] of every item (what lpr_solve_result.z is in lpr_dual_solve). */
int lpr_cut_batch_z_read(lpr_cut_batch* b, double* z);

/* Narration: the numbers behind the console text of
 * CuttingPlaneSolver.CuttingPlaneSolution (IntegerProgramming/CuttingPlaneSolver.cs:47-54, 64-229)
 * -- "Initial tableau:", "Before / After pivot on cut: row r, col c", every tableau both clean-up
 * solvers print under printSteps: true (Simplex/DualSimplex.cs:14-114, 193-207, 228-239;
 * Simplex/PrimalSimplexSolver2.cs:46-97, 184-189) and the closing lines -- kept on the device by
 * the kernel that makes them; the host only formats (cut_batch.py: format_cutting_plane).
 *
 * lpr_cut_batch_narrate_reserve makes the handle narrated: per item an event list of ev_cap
 * events of four int32 (kind, a, b, rows_now) and cap_doubles[k] >= 0 doubles of tableau data,
 * both appended over the handle's life as the log is.  Event kinds: 0 CALL (a mode, b
 * print_steps; start of every lpr_cut_batch_run), 1 LEVEL (one CuttingPlaneSolution call :64;
 * "Initial tableau:" :74 is the state at this point), 2 CUT (a the source row, 0-based among the
 * constraint rows :96; the row of :110 is the next data block), 3 SOLVE_BEGIN (a 0 dual :188-190,
 * 1 primal2 :198-200), 4 SOLVE_END (a the lpr_status of the inner solve -- DualSimplex.cs:42, :74,
 * :110; PrimalSimplexSolver2.cs:58, :65, :92; LPR_PIVOT_TOO_SMALL for :156 / :149 -- b 1 where
 * LPR_PIVOT_LIMIT came from opts.hard_cap and not from maxIters), 5 EXIT (a the code of
 * lpr_cut_batch_result_read), 8 + q PIVOT (q the log kind 0 dual / 1 primal2 / 2 cut; a, b the
 * row and column of the log triple; the whole rows_now x cols tableau after it is the next data
 * block).  Data: block 0 is the rows x cols tableau at reserve time, then one block per CUT
 * (cols doubles) and per PIVOT (rows_now x cols), back to back in event order.  A block that does
 * not fit whole is counted and not written, and so is every later one; the made counts are exact.
 * Allowed once and only before the first run: called twice, after a run, with NULL, with an entry
 * < 0 or with ev_cap < 1 it is LPR_BAD_ARGUMENT.  A failed allocation is LPR_OUT_OF_MEMORY naming
 * the buffer and its size, and leaves the handle usable and un-narrated.  Code, cuts, log and
 * tableau of a narrated handle are those of an un-narrated one. */
int lpr_cut_batch_narrate_reserve(lpr_cut_batch* b, const int64_t* cap_doubles, int32_t ev_cap);
/* Per item: events made, doubles made, doubles kept (a whole number of blocks) and the offset of
 * its slice in the data lpr_cut_batch_narrate_read_all copies; any may be NULL.  The reads below
 * are LPR_BAD_ARGUMENT on an un-narrated handle. */
int lpr_cut_batch_narrate_info(lpr_cut_batch* b, int64_t* events_made, int64_t* doubles_made,
                               int64_t* doubles_kept, int64_t* data_off);
/* Item k's events as quads: *count = all of them, the first min(*count, ev_cap, cap) copied. */
int lpr_cut_batch_narrate_events_read(lpr_cut_batch* b, int32_t k, int32_t* quads, int64_t cap,
                                      int64_t* count);
/* n doubles of item k's data from first_double; a range beyond what is kept is refused. */
int lpr_cut_batch_narrate_data_read(lpr_cut_batch* b, int32_t k, int64_t first_double, int64_t n,
                                    double* out);
/* Every item at once: the event buffer (count x ev_cap quads, item k at quad k * ev_cap) and the
 * data slab (the sum of cap_doubles, item k at its data_off); either pointer may be NULL, a
 * capacity below the size is LPR_BAD_ARGUMENT. */
int lpr_cut_batch_narrate_read_all(lpr_cut_batch* b, int32_t* quads, int64_t cap_quads,
                                   double* data, int64_t cap_doubles);


/* ------------------------------------------------------------------ knapsack batch */

/* Many option-5 instances per device call.  One handle holds `count`
 * independent 0/1 knapsack instances; one solve call runs the whole level-synchronous search of
 * section 11 for every instance on the device, with no host step per level, and one DP call runs
 * the 0/1 DP of every instance, which together are option 5's B&B-against-DP comparison
 * (Program.cs:430-470) for the whole batch.  PARITY: instance k ends with exactly what
 * lpr_knap_bb_solve gives for it alone AT THE SAME node_cap -- status, found, Z*, the selected
 * items, the rank, evaluated / levels / widest and every node record kept, the bound by bits.
 * The default cap differs (1024 here, 2^22 there), so pass the cap to both when comparing.
 * Forms, picked per instance by node_cap x (32 x ceil(n / 64) + 32) + 8 n bytes: W one wave per
 * instance (four per workgroup), G one workgroup with everything in LDS, H one workgroup with
 * the frontier in a global slab.  The reference has no batch mode. */
typedef struct lpr_knap_batch lpr_knap_batch;

/* capacity[count], n[count]; weights and values are doubles packed by n[k].  Per instance the
 * checks of lpr_knap_bb_create: integral doubles, 1 <= w <= 2^31-1, 0 <= v <= 2^31-1,
 * capacity >= 0, 1 <= n <= 8192; a violation is LPR_BAD_ARGUMENT and the message names the
 * instance and the index.  node_cap[count] (evaluated nodes per instance) or NULL; NULL or an
 * entry <= 0 means 1024, an entry over 2^22 is LPR_BAD_ARGUMENT.  narrate: node records kept per
 * instance (0: none; at most node_cap are ever written).  A failed device allocation is
 * LPR_OUT_OF_MEMORY and the message gives the footprint. */
int lpr_knap_batch_create(lpr_engine* e, int32_t count, const int64_t* capacity, const int32_t* n,
                          const double* weights, const double* values, const int64_t* node_cap,
                          int32_t narrate, lpr_knap_batch** out);
/* After lpr_engine_close the handle is orphaned: every call but this one is LPR_BAD_ARGUMENT. */
int lpr_knap_batch_destroy(lpr_knap_batch* b);

typedef struct lpr_knap_batch_opts {
    int32_t chunk;    /* nodes an instance may evaluate per launch, checked at level boundaries
                         (0: by form)                                      */
    int32_t variant;  /* 0 auto; 1 / 2 / 3 force form W / G / H on the instances that fit it
                         (tests and tuning only, same bits)                                      */
} lpr_knap_batch_opts;

typedef struct lpr_knap_batch_result {
    int32_t finished;  /* instances whose search ended (LPR_OK_OPTIMAL)                          */
    int32_t capped;    /* instances stopped by their node_cap (LPR_BB_NODE_CAP)                  */
    int32_t launches;  /* search kernels launched by this call                                   */
    int32_t items_w;   /* instances this call ran in form W ...                                  */
    int32_t items_g;   /* ... G ...                                                              */
    int32_t items_h;   /* ... and H                                                              */
    int64_t nodes;     /* nodes evaluated, all instances                                         */
} lpr_knap_batch_result;

/* The search of every instance, from the roots (a second call repeats the first).  opts may be
 * NULL.  Returns LPR_OK_OPTIMAL unless the call itself failed. */
int lpr_knap_batch_solve(lpr_knap_batch* b, const lpr_knap_batch_opts* opts,
                         lpr_knap_batch_result* res);
/* Per instance, as lpr_knap_bb_result: LPR_OK_OPTIMAL or LPR_BB_NODE_CAP, found, Z* (0 when not
 * found), evaluated, widest, levels; count entries each, any may be NULL. */
int lpr_knap_batch_result_read(lpr_knap_batch* b, int32_t* status, int32_t* found, double* z,
                               int64_t* evaluated, int64_t* widest, int32_t* levels);
/* rank[p] of every instance (lpr_knap_bb_rank_read), packed by n[k]. */
int lpr_knap_batch_rank_read(lpr_knap_batch* b, int32_t* rank);
/* The incumbents' items as ascending original indices, packed by n[k]: counts[k] entries of
 * instance k's block are valid, the rest of the block is -1. */
int lpr_knap_batch_selected_read(lpr_knap_batch* b, int32_t* ids, int32_t* counts);
/* Node records of instance k, as lpr_knap_bb_nodes_read: *count = records kept, the first
 * min(*count, cap) copied; kitem holds ORIGINAL indices. */
int lpr_knap_batch_nodes_read(lpr_knap_batch* b, int32_t k, int32_t* parent, int32_t* branch,
                              int32_t* status, double* bound, int32_t* kitem, int64_t* value,
                              int64_t cap, int64_t* count);
/* best[k] = dp[capacity[k]] of the 0/1 DP of lpr_knap_dp over an int64 row initialised to 0, for
 * every instance; which[count] or NULL: instances with 0 are skipped and get best[k] = -1.  An
 * instance that is not skipped and needs more than 2^22 cells (capacity + 1 > 4 194 304) makes
 * the call fail with LPR_BAD_ARGUMENT naming it: solve that one alone with lpr_knap_dp. */
int lpr_knap_batch_dp(lpr_knap_batch* b, const uint8_t* which, int64_t* best);

/* ------------------------------------------------------------------ revised simplex batch */

/* Many option-2 LPs per device call.  One handle holds `count` independent
 * LPs in (c, A, b) form; one solve call runs RevisedPrimalSimplexSolver.Solve() (:82-251) and
 * ExtractSolution (:277-287) for every LP on the device.  PARITY: LP k ends with exactly what
 * lpr_revised_solve gives for it alone at the same max_pivots -- status, iterations, the (row,
 * enter, leave) log, the basis, the bytes of B^-1 and of the last x_B, and x and Z on the optimal
 * exit.  Forms, picked per LP by the bytes it keeps resident (B^-1 and A with odd leading
 * dimensions, six vectors of m, c, the n + m staged candidates, the basis and the non-basic
 * flags): W one wave per LP (four per workgroup), G one workgroup with everything in LDS, H one
 * workgroup with B^-1 and A in a global slab.  IterationSnapshots are kept, as numbers, by a
 * batch made traced with lpr_rev_batch_trace_reserve (below); an untraced batch keeps none.  The
 * reference has no batch mode. */
typedef struct lpr_rev_batch lpr_rev_batch;

/* new RevisedPrimalSimplexSolver(objective, constraints, isMin) per LP (:41-80): c = -objective
 * when is_min (:51), B^-1 = I, basis[i] = n + i, c_B = 0 (:72-78); Relation is never read.
 * n[count], m[count]; objective packed by n[k], A as packed m[k] x n[k] row-major blocks, b
 * packed by m[k], is_min[count].  LPR_BAD_ARGUMENT with a message: count <= 0, a null array,
 * n[k] < 1 or m[k] < 1 (the two ArgumentExceptions of :43-44), log_cap < 0, or an LP beyond
 * m <= 1023 and n + m <= 2047 (what lpr_batch_from_lps takes; solve that one alone with
 * lpr_revised_solve).  log_cap: (row, enter, leave) triples kept per LP; 0 means
 * 4 * (n + 2 m), at most 4096.  A failed device allocation is LPR_OUT_OF_MEMORY and the message
 * names the buffer and its size. */
int lpr_rev_batch_create(lpr_engine* e, int32_t count, const int32_t* n, const int32_t* m,
                         const double* objective, const double* A, const double* b,
                         const int8_t* is_min, int32_t log_cap, lpr_rev_batch** out);
/* After lpr_engine_close the handle is orphaned: every call but this one is LPR_BAD_ARGUMENT. */
int lpr_rev_batch_destroy(lpr_rev_batch* b);

typedef struct lpr_rev_batch_opts {
    int64_t max_pivots;  /* iterations per LP per call, tested where lpr_revised_solve tests it:
                            after the entering choice (0: no limit)                              */
    int32_t chunk;       /* passes of the loop (:87) per LP per launch (0: by form, section 17)  */
    int32_t variant;     /* 0 auto; 1 / 2 / 3 force form W / G / H on the LPs that fit it (tests
                            and tuning only, same bits)                                          */
} lpr_rev_batch_opts;

typedef struct lpr_rev_batch_result {
    int32_t optimal;     /* LPs in each state after this call: LPR_OK_OPTIMAL (:124-146) ...     */
    int32_t unbounded;   /* ... LPR_UNBOUNDED (:178-179) ...                                     */
    int32_t infeasible;  /* ... LPR_INFEASIBLE_BASIS (:90-91) ...                                */
    int32_t other;       /* ... LPR_ENTERING_ALREADY_BASIC (:182-183), LPR_PIVOT_TOO_SMALL (:267) */
    int32_t limit;       /* ... and LPR_PIVOT_LIMIT (no C# counterpart)                          */
    int32_t launches;    /* solve kernels launched by this call                                  */
    int64_t iterations;  /* iterations (:249) performed by this call, all LPs                    */
} lpr_rev_batch_result;

/* Solve() (:82-251) for every LP that is not finished: an LP at LPR_PIVOT_LIMIT resumes with the
 * bits an uninterrupted solve has, a finished one stays as it is.  opts may be NULL.  Returns
 * LPR_OK_OPTIMAL unless the call itself failed (a bad variant or a negative chunk is
 * LPR_BAD_ARGUMENT). */
int lpr_rev_batch_solve(lpr_rev_batch* b, const lpr_rev_batch_opts* opts,
                        lpr_rev_batch_result* res);
/* Per LP: status, iterations (:249) and FinalZ = Dot(cOrig, x) (:284; 0 unless optimal); count
 * entries each, any may be NULL. */
int lpr_rev_batch_status_read(lpr_rev_batch* b, int32_t* status, int64_t* iterations, double* z);
/* SolutionVector (:277-283) of every LP, packed by n[k]; 0 unless optimal. */
int lpr_rev_batch_solution_read(lpr_rev_batch* b, double* x);
/* basicVariables (:28, :195) of every LP, packed by m[k]. */
int lpr_rev_batch_basis_read(lpr_rev_batch* b, int32_t* basis);
/* The log of LP k: leavingRow (:177, 0-based), enteringIdx (:122), leavingVar (:181) of the first
 * min(iterations, log_cap) iterations; *count = triples kept, the first min(*count, cap) copied. */
int lpr_rev_batch_log_read(lpr_rev_batch* b, int32_t k, int32_t* row, int32_t* enter,
                           int32_t* leave, int64_t cap, int64_t* count);
/* BInverse (:29, :274) of LP k, m x m row-major. */
int lpr_rev_batch_binv_read(lpr_rev_batch* b, int32_t k, double* out);
/* The last x_B = BInverse b (:89) of LP k, m entries. */
int lpr_rev_batch_xb_read(lpr_rev_batch* b, int32_t k, double* out);
/* n (:45) and m (:46) of LP k; either may be NULL. */
int lpr_rev_batch_shape(lpr_rev_batch* b, int32_t k, int32_t* n, int32_t* m);

/* Traced batches: the solve also records, per LP, every snapshot
 * CaptureSnapshot (:294-387) would have appended to IterationSnapshots -- one after each pivot
 * (:232-247) and the "Optimal" one (:124-146) -- as numbers in device memory; the host only
 * formats.  One record is 6 + 7 m + n + m n + m m doubles, indices stored as doubles:
 *   [0] enteringIdx  [1] leavingRow  [2] leavingVarIndex_Pre  [3] enteringRC_pre  [4] zWorking
 *   [5] zOriginal, then y[m], rcX[n], rcS[m], u_pre[m], ratios_pre[m] (+inf where u_i <= EPS),
 *   basisForRatios_Pre[m], basicVariables after the pivot [m], xB[m], BInvA[m x n]
 *   (MultiplyMatrices(BInverse, A) in the C#'s order, :360), BInv[m x m].
 * The "Optimal" record has -1, -1, -1, rc 0.0, u_pre +0.0, ratios_pre +inf and the current basis
 * twice.  An LP has iterations + (status == LPR_OK_OPTIMAL) records: LPR_UNBOUNDED,
 * LPR_ENTERING_ALREADY_BASIC and LPR_PIVOT_TOO_SMALL add none for the failing pass, and an LP
 * that ends LPR_INFEASIBLE_BASIS after k pivots has k complete ones.  PARITY: every record is the
 * bytes of the single-model path's numbers for that snapshot, and everything else a traced batch
 * ends with is the bytes of the untraced batch.
 *
 * lpr_rev_batch_trace_reserve makes the handle traced and allocates trace_cap records per LP,
 * zero-filled; a record index >= trace_cap is counted, not written.  Only before the handle's
 * first solve: LPR_BAD_ARGUMENT with a message afterwards, when called twice, or for
 * trace_cap < 1.  A failed allocation is LPR_OUT_OF_MEMORY and the message names the buffer and
 * its size; the handle stays untraced.  opts and result of lpr_rev_batch_solve are unchanged. */
int lpr_rev_batch_trace_reserve(lpr_rev_batch* b, int32_t trace_cap);
/* Per LP (count entries each, any may be NULL): snapshots, the exact number of records (may
 * exceed trace_cap; min(snapshots, trace_cap) are kept); offset, where LP k's records start in
 * the trace slab, in doubles; stride, the doubles of one record. */
int lpr_rev_batch_trace_info(lpr_rev_batch* b, int64_t* snapshots, int64_t* offset,
                             int64_t* stride);
/* Records [first, first + n) of LP k into out[n * stride]; a range beyond the kept records is
 * LPR_BAD_ARGUMENT. */
int lpr_rev_batch_trace_read(lpr_rev_batch* b, int32_t k, int64_t first, int64_t n, double* out);
/* The whole trace slab (trace_cap * sum of the strides doubles) in one copy; cap_doubles is what
 * `out` holds, LPR_BAD_ARGUMENT when it is too small.  Every trace read on an untraced or
 * orphaned handle is LPR_BAD_ARGUMENT with a message. */
int lpr_rev_batch_trace_read_all(lpr_rev_batch* b, double* out, int64_t cap_doubles);

/* Device text: the bytes of TableIterationFormater.Format
 * (Utilities/TableIterationFormater.cs:22-48) written on the device.  A block is Format(tab,
 * numOriginalVars, title) without its first line ("\n" + title + ":" + CRLF, which stays with the
 * caller: one tableau is printed under several titles):
 *   "-" x 80 CRLF
 *   "Table\t" "x1\t" .. "x{nvars}\t" "t1\t" .. "t{cols-1-nvars}\t" "RHS" CRLF        (:27-35)
 *   "Z\t" F3(T[0,0]) "\t" .. F3(T[0,cols-1]) "\t" CRLF                                (:36-40)
 *   "{i}\t" F3(T[i,0]) "\t" .. "\t" CRLF  for i = 1 .. rows-1                         (:41-47)
 * with {v:F3} of .NET Framework: the 15-significant-digit image of v (ties to even) rounded half
 * away from zero at three decimals, no sign on an all-zero result, NaN / Infinity / -Infinity as
 * words.  PARITY: byte for byte what table_iteration_formater.Format gives after its title line.
 * An lpr_text holds the blocks in device memory, independent of what they were formatted from. */
typedef struct lpr_text lpr_text;

/* Format (:22-48) of a ragged list of tableaux from the host: count blocks, block k is
 * rows[k] x cols[k] row-major in `tableaux`, one after the other, with nvars[k] original
 * variables (the x loop of :32 runs to nvars whatever cols is; the t loop of :33 is empty when
 * nvars >= cols - 1).  LPR_BAD_ARGUMENT with a message naming the call and the index for a NULL
 * argument, count < 1, rows < 1, cols < 1 or nvars < 0; a failed allocation is LPR_OUT_OF_MEMORY
 * naming the buffer and its size. */
int lpr_text_format_tableaux(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                             const int32_t* nvars, const double* tableaux, lpr_text** out);
/* Format (:22-48) of every kept record of every LP of a traced batch, read where the trace slab
 * keeps it, in record order, followed per LP by one block of its tableau in the batch when the LP
 * is LPR_OK_OPTIMAL or LPR_UNBOUNDED (PrimalSimplexSolver.cs:118-122, :133).  first_block[count +
 * 1] (may be NULL): where LP k's blocks start.  Reads the batch only.  An untraced or orphaned
 * batch is LPR_BAD_ARGUMENT; after LPR_OUT_OF_MEMORY the batch stays usable. */
int lpr_batch_trace_text(lpr_batch* b, int64_t* first_block, lpr_text** out);
/* DisplayTableau (IntegerProgramming/BranchBoundSimplexSolver.cs:623-640) of a ragged list of
 * tableaux from the host: as lpr_text_format_tableaux, but block k is
 * Format (:22-48) of the tableau after round4[k] applications of Math.Round(v, 4) to every cell
 * (RoundTableau; 0 leaves the cells as they are, 2 is RoundAllTableaux followed by
 * DisplayTableau).  An entry of round4 outside 0..2, or a NULL round4, is LPR_BAD_ARGUMENT naming
 * the index. */
int lpr_text_format_tableaux_rounded(lpr_engine* e, int32_t count, const int32_t* rows,
                                     const int32_t* cols, const int32_t* nvars,
                                     const int32_t* round4, const double* tableaux,
                                     lpr_text** out);
/* DisplayTableau (BranchBoundSimplexSolver.cs:623-640) of everything a narrated B&B batch keeps
 * (DESIGN.md sections 23 and 26), read where the batch keeps it.  Per IP: one block per kept child
 * tableau in the order of its slice -- record-id order, list order within a record; a record keeps
 * min(ntab, (doubles_kept - tab_off) / (rows * cols)) tableaux, never below 0 -- each
 * (R0 + depth) x (C0 + depth) with the IP's nvars, then one block of the incumbent's tableau when
 * the IP has one.  Cells are rounded as ExecuteBranchAndBound rounds what it shows: twice for a
 * tableau of a solved child (RoundAllTableaux :1124 / :1187, then DisplayTableau), once for one of
 * an infeasible or failed child, once for the incumbent's (stored rounded by :1047).
 * first_block[count + 1] (may be NULL): where IP k's blocks start.  Reads the batch only; the text
 * owns its bytes and outlives a later run, reserve or destroy of the batch.  LPR_BAD_ARGUMENT, with
 * a message saying which, for an un-narrated batch, no run since the last reserve, an orphaned
 * handle, a NULL out, or nothing to format (no kept tableau and no incumbent in the whole batch);
 * after LPR_OUT_OF_MEMORY the batch stays usable. */
int lpr_bb_batch_narrate_text(lpr_bb_batch* b, int64_t* first_block, lpr_text** out);
/* Blocks, bytes of all blocks (:22-48, title lines excluded) and the milliseconds the kernels
 * took; any may be NULL. */
int lpr_text_info(lpr_text* t, int64_t* blocks, int64_t* bytes, double* kernel_ms);
/* Where each block (:22-48) starts: blocks + 1 entries, the last one `bytes`. */
int lpr_text_offsets_read(lpr_text* t, int64_t* offsets);
/* Bytes [first_byte, first_byte + n) of the text (:22-48); a range beyond `bytes` is
 * LPR_BAD_ARGUMENT. */
int lpr_text_read(lpr_text* t, int64_t first_byte, int64_t n, uint8_t* out);
/* Releases the blocks (:22-48).  After lpr_engine_close the handle is orphaned: every call but
 * this one is LPR_BAD_ARGUMENT. */
int lpr_text_destroy(lpr_text* t);

#ifdef __cplusplus
}
#endif
#endif /* LPR_ENGINE_H */
