// cut_kernels.hip -- gfx950 kernels + C ABI of the cutting-plane side path ("next" row f3):
//   DualSimplexSolver.Solve        LPR_381_Group_V22/Simplex/DualSimplex.cs:14-114
//   PrimalSimplexSolver2.Solve     LPR_381_Group_V22/Simplex/PrimalSimplexSolver2.cs:46-97
//   CuttingPlaneSolver             LPR_381_Group_V22/IntegerProgramming/CuttingPlaneSolver.cs:64-229
// They work on the same device tableau as the primal path (row 0 = objectiveRow, rows 1.. =
// constraintRows).  Same pivot shape as PrimalSimplexSolver with two differences: rows whose
// factor is within 1e-9 of zero are left untouched (DualSimplex.cs:166, PrimalSimplexSolver2.cs:160)
// and every selection is an EPS-band sequential fold ("better by more than EPS"), replayed exactly
// and in one pass by eps_fold (fold_common.hpp), as in the sensitivity re-solve.  Not pipelined:
// this path is dead code in the reference's menu (Program.cs:417-428); parity is the bar here, not
// the roofline.
#include "cut_common.hpp"
#include "select_common.hpp"

#include <new>

#pragma clang fp contract(off)

namespace lpr {

constexpr int kCutK = 16;  // eps_fold candidates cached per lane: 16 384 rows / columns in one pass

struct CutState {
    int32_t status;      // kRunning or an lpr_status
    int32_t pr, pc;      // pivot (tableau row, column) of the pending update
    int32_t print_steps; // `iter` only advances when printSteps is set (DualSimplex.cs:94)
    int32_t pending;     // a pivot has been staged/applied and not yet counted
    int32_t nan_updates; // the staged pivot is PrimalSimplexSolver2's: it skips a row on `|f| <= EPS`
                         // (:160), so a NaN factor updates its row; the other two pivots update on
                         // `|f| > EPS` (DualSimplex.cs:166, CuttingPlaneSolver.cs:161), so it does not
    int64_t iter;        // the C# `iter`
    int64_t done;        // pivots performed
    int64_t max_iters;   // maxIters (:108 / :90)
    int64_t hard_cap;    // extra stop (no C# counterpart), <= 0: none
    int64_t log_n, log_cap;
    int32_t scratch[8];  // cutting-plane step results
};

// |num / a| over the negative entries of row `prow` with a non-zero objective entry; NaN = skip
__device__ __forceinline__ double dual_ratio(const double* __restrict__ T, int ld, int prow,
                                             int j) {
    const double a = T[(size_t)prow * ld + j];
    if (!(a < -kCutEps)) return NAN;
    const double num = T[j];
    if (!(fabs(num) > kCutEps)) return NAN;
    return fabs(ieee_div(num, a));
}

// Pivot column of the dual ratio test on row `prow` (DualSimplex.cs:53-70,
// CuttingPlaneSolver.cs:116-132): `ratio < best - EPS || (|ratio - best| <= EPS && (pc == -1 ||
// j < pc))` over j ascending.  The tie clause never fires: j ascends, so `j < pc` is false once a
// column has been taken; before that best is +inf and |ratio - inf| is inf (NaN for ratio = inf),
// never <= EPS.  What is left is eps_fold's "better by more than EPS".
__device__ __forceinline__ int fold_dual_column(const double* __restrict__ T, int ld, int C,
                                                int prow, int* lds, double* lds_v) {
    return eps_fold<kCutK>(
        0, C - 1, INFINITY, [&](int j) { return dual_ratio(T, ld, prow, j); }, lds, lds_v);
}

// One loop head of DualSimplexSolver.Solve (:24-112) or PrimalSimplexSolver2.Solve (:49-96).
__global__ __launch_bounds__(1024) void k_cut_select(double* __restrict__ T, int ld, int R, int C,
                                                     double* __restrict__ rowbuf,
                                                     double* __restrict__ colbuf,
                                                     int32_t* __restrict__ log, CutState* st,
                                                     int mode) {
    __shared__ int lds[32];
    __shared__ double lds_v[32];
    if (st->status != kRunning) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int rhs = C - 1;
    int pr = -1, pc = -1;

    // Close the previous pivot first: `if (iter >= maxIters) return false` comes AFTER the pivot in
    // the C# (:108 / :90).  It is done here, not in k_cut_update, so that no update workgroup can
    // see the status change while others of the same launch are still running.
    int64_t done_now;
    {
        const int pending = st->pending;
        const int64_t it = st->iter, mx = st->max_iters;
        done_now = st->done + (pending ? 1 : 0);
        __syncthreads();
        if (pending) {
            if (tid == 0) {
                st->pending = 0;
                st->done += 1;
            }
            if (it >= mx) {
                if (tid == 0) st->status = LPR_PIVOT_LIMIT;
                return;
            }
        }
    }

    // Each selection below is a sequential fold over ascending indices whose C# condition also
    // has a tie clause on `index < current choice`.  An ascending scan only meets indices above
    // its current choice, so those clauses are dead and eps_fold replays what is left.
    if (mode == kCutDual) {
        // pivot row: `rhs < mostNeg - EPS || (|rhs - mostNeg| <= EPS && pivotRow != -1 &&
        // r < pivotRow)` over constraint rows r ascending, mostNeg = 0 at the start (:29-37);
        // r > pivotRow whenever pivotRow != -1
        const int prow = eps_fold<kCutK>(
            0, R - 1, 0.0, [&](int r) { return T[(size_t)(r + 1) * ld + rhs]; }, lds, lds_v);
        if (prow < 0) {
            if (tid == 0) st->status = LPR_OK_OPTIMAL;  // "Dual phase complete" :40-44
            return;
        }
        pr = prow + 1;
        pc = fold_dual_column(T, ld, C, pr, lds, lds_v);
        if (pc < 0) {
            if (tid == 0) st->status = LPR_INFEASIBLE_BASIS;  // return false :72-76
            return;
        }
    } else {
        // entering column: `c < mostNeg - EPS || (|c - mostNeg| <= EPS && pc != -1 && j < pc)`,
        // mostNeg = 0 at the start (:102-117); j > pc whenever pc != -1
        pc = eps_fold<kCutK>(0, rhs, 0.0, [&](int j) { return T[j]; }, lds, lds_v);
        if (pc < 0) {
            if (tid == 0) st->status = LPR_OK_OPTIMAL;  // :54-60
            return;
        }
        // leaving row over the rows with a > EPS (:120-141), with the C#'s operator precedence:
        // (ratio > EPS && ratio < best - EPS) || ((|ratio - best| <= EPS && bestRow == -1) ? true
        //                                                                           : i < bestRow)
        // The second operand is never true: with bestRow == -1 best is +inf, so the ternary's
        // condition is false and `i < -1` is false; afterwards i > bestRow.
        pr = eps_fold<kCutK>(
            1, R, INFINITY,
            [&](int i) -> double {
                const double a = T[(size_t)i * ld + pc];
                if (!(a > kCutEps)) return NAN;
                const double ratio = ieee_div(T[(size_t)i * ld + rhs], a);
                return (ratio > kCutEps) ? ratio : NAN;
            },
            lds, lds_v);
        if (pr < 0) {
            if (tid == 0) st->status = LPR_UNBOUNDED;  // return false :63-68
            return;
        }
    }

    if (st->hard_cap > 0 && done_now >= st->hard_cap) {
        if (tid == 0) st->status = LPR_PIVOT_LIMIT;
        return;
    }
    const double piv = T[(size_t)pr * ld + pc];
    if (fabs(piv) <= kCutEps) {
        if (tid == 0) st->status = LPR_PIVOT_TOO_SMALL;  // InvalidOperationException :155 / :148
        return;
    }
    for (int j = tid; j < ld; j += nt) rowbuf[j] = (j < C) ? ieee_div(T[(size_t)pr * ld + j], piv) : 0.0;
    for (int i = tid; i < R; i += nt) colbuf[i] = T[(size_t)i * ld + pc];
    if (tid == 0) {
        st->pr = pr;
        st->pc = pc;
        st->nan_updates = (mode == kCutPrimal2);
        st->pending = 1;  // closed by the next k_cut_select
        if (st->print_steps) st->iter += 1;  // ++iter inside `if (printSteps)` (:94 / :75)
        if (st->log_n < st->log_cap) {
            int32_t* e = log + 3 * st->log_n;
            e[0] = mode;
            e[1] = (mode == kCutDual) ? pr - 1 : pr;  // the C#'s own row numbering
            e[2] = pc;
        }
        st->log_n += 1;
    }
}

// Pivot with the row skip (DualSimplex.cs:150-178, PrimalSimplexSolver2.cs:145-164): row i is
// rewritten only if |f_i| > EPS; a NaN f_i rewrites its row in PrimalSimplexSolver2's form alone
// (`if (|f| <= EPS) continue`), st->nan_updates.  No state is written here: the bookkeeping lives in k_cut_select.
template <int TR>
__global__ __launch_bounds__(256) void k_cut_update(double* __restrict__ T, int ld, int R,
                                                    const double* __restrict__ rowbuf,
                                                    const double* __restrict__ colbuf,
                                                    CutState* st, int check_status) {
    if (check_status && st->status != kRunning) return;
    const int ld2 = ld >> 1;
    const int c2 = blockIdx.x * blockDim.x + threadIdx.x;
    const int i0 = blockIdx.y * TR;
    const int r = st->pr;
    const bool nan_updates = st->nan_updates != 0;
    if (c2 >= ld2) return;
    const double2 pr2 = reinterpret_cast<const double2*>(rowbuf)[c2];
    double2* __restrict__ T2 = reinterpret_cast<double2*>(T);
#pragma unroll
    for (int k = 0; k < TR; ++k) {
        const int i = i0 + k;
        if (i >= R) break;
        if (i == r) {
            T2[(size_t)i * ld2 + c2] = pr2;
            continue;
        }
        const double f = colbuf[i];
        if (nan_updates ? (fabs(f) <= kCutEps) : !(fabs(f) > kCutEps)) continue;  // not touched
        double2 x = T2[(size_t)i * ld2 + c2];
        const double px = f * pr2.x;
        const double py = f * pr2.y;
        x.x = x.x - px;
        x.y = x.y - py;
        T2[(size_t)i * ld2 + c2] = x;
    }
}

// CuttingPlaneSolution steps 1-6 (:76-138): choose the constraint whose fractional RHS is closest
// to 0.5 (first in index order among equals -- see oracle/oracle_cut.c on List.Sort), append
// cut = -frac(row) as tableau row R, pick the pivot column on it.  scratch[0] = chosen constraint
// (-1: all RHS integral), scratch[1] = pivot column (-1: none).  Also stages rowbuf / colbuf for
// the pivot on the cut.
__global__ __launch_bounds__(1024) void k_cut_add(double* __restrict__ T, int ld, int R, int C,
                                                  double* __restrict__ rowbuf,
                                                  double* __restrict__ colbuf,
                                                  int32_t* __restrict__ log, CutState* st) {
    __shared__ int lds[32];
    __shared__ double lds_v[32];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int rhs = C - 1;
    // lexicographic min of (|frac - 0.5|, index) over rows with frac > EPS
    Cand best;
    best.v = INFINITY;
    best.i = -1;
    for (int i = tid; i < R - 1; i += nt) {
        const double fr = cut_frac(T[(size_t)(i + 1) * ld + rhs]);
        if (fr > kCutEps) {
            const double key = fabs(fr - 0.5);
            if (best.i < 0 || key < best.v) {  // ascending i per thread: strict < keeps the first
                best.v = key;
                best.i = i;
            }
        }
    }
    best = block_cand_min(best, lds_v, lds);
    if (best.i < 0) {
        if (tid == 0) {
            st->scratch[0] = -1;
            st->scratch[1] = -1;
        }
        return;
    }
    const int chosen = best.i;
    for (int j = tid; j < ld; j += nt)  // cut row (:99-110), padding stays 0
        T[(size_t)R * ld + j] = (j < C) ? -cut_frac(T[(size_t)(chosen + 1) * ld + j]) : 0.0;
    __syncthreads();  // the fold reads the row this workgroup has just written
    __threadfence_block();
    const int pc = fold_dual_column(T, ld, C, R, lds, lds_v);  // :113-132 on the new row
    if (tid == 0) {
        st->scratch[0] = chosen;
        st->scratch[1] = pc;
    }
    if (pc < 0) return;
    const double piv = T[(size_t)R * ld + pc];
    if (fabs(piv) <= kCutEps) {  // :145-150
        if (tid == 0) st->scratch[1] = -2;
        return;
    }
    for (int j = tid; j < ld; j += nt) rowbuf[j] = (j < C) ? ieee_div(T[(size_t)R * ld + j], piv) : 0.0;
    for (int i = tid; i < R + 1; i += nt) colbuf[i] = T[(size_t)i * ld + pc];
    if (tid == 0) {
        st->pr = R;
        st->nan_updates = 0;
        st->pc = pc;
        if (st->log_n < st->log_cap) {
            int32_t* e = log + 3 * st->log_n;
            e[0] = 2;
            e[1] = R - 1;  // cutRowIdx (constraint index)
            e[2] = pc;
        }
        st->log_n += 1;
    }
}

// needDual / needPrimal / anyFractional (:183-184, :215-217) -> scratch[2..4]
__global__ __launch_bounds__(1024) void k_cut_flags(const double* __restrict__ T, int ld, int R,
                                                    int C, CutState* st) {
    const int tid = threadIdx.x, nt = blockDim.x;
    int neg = 0, nonopt = 0, frac = 0;
    for (int i = 1 + tid; i < R; i += nt) {
        const double v = T[(size_t)i * ld + (C - 1)];
        if (v < -kCutEps) neg = 1;
        if (cut_frac(v) > kCutEps) frac = 1;
    }
    for (int j = tid; j < C - 1; j += nt)
        if (T[j] < -kCutEps) nonopt = 1;
    neg = __syncthreads_or(neg);
    nonopt = __syncthreads_or(nonopt);
    frac = __syncthreads_or(frac);
    if (tid == 0) {
        st->scratch[2] = neg;
        st->scratch[3] = nonopt;
        st->scratch[4] = frac;
    }
}

}  // namespace lpr

// ---------------------------------------------------------------------------------------------
// host side

struct lpr_cut_ctx {  // per-tableau scratch of this path, hung off the tableau lazily
    lpr::CutState* state = nullptr;
    lpr::CutState* h_state = nullptr;
    int32_t* log = nullptr;
    int64_t log_cap = 0;
};

using namespace lpr;

namespace {

int cut_ensure(lpr_tableau* t) {
    if (t->cut) return LPR_OK_OPTIMAL;
    lpr_cut_ctx* c = new (std::nothrow) lpr_cut_ctx();
    if (!c) return LPR_OUT_OF_MEMORY;
    c->log_cap = 1 << 16;
    hipError_t err = hipMalloc(&c->state, sizeof(CutState));
    if (err == hipSuccess) err = hipHostMalloc(&c->h_state, sizeof(CutState));
    if (err == hipSuccess) err = hipMalloc(&c->log, (size_t)c->log_cap * 3 * sizeof(int32_t));
    if (err != hipSuccess) {
        set_error("cut-path scratch allocation failed: %s", hipGetErrorString(err));
        hipFree(c->state);
        hipFree(c->log);
        if (c->h_state) hipHostFree(c->h_state);
        delete c;
        return LPR_DEVICE_ERROR;
    }
    std::memset(c->h_state, 0, sizeof(CutState));
    c->h_state->log_cap = c->log_cap;
    t->cut = c;
    return LPR_OK_OPTIMAL;
}

void cut_launch_update(lpr_tableau* t, int check_status) {
    lpr_cut_ctx* c = static_cast<lpr_cut_ctx*>(t->cut);
    constexpr int TR = 8;
    dim3 grid((t->ld / 2 + 255) / 256, (t->rows + TR - 1) / TR);
    hipLaunchKernelGGL((k_cut_update<TR>), grid, dim3(256), 0, t->eng->stream, t->T, t->ld, t->rows,
                       t->rowbuf, t->colbuf, c->state, check_status);
}

// DualSimplexSolver.Solve / PrimalSimplexSolver2.Solve driver; returns the lpr_status
int cut_run_solver(lpr_tableau* t, int mode, int max_iters, int print_steps, int64_t hard_cap,
                   int64_t* pivots) {
    lpr_cut_ctx* c = static_cast<lpr_cut_ctx*>(t->cut);
    hipStream_t s = t->eng->stream;
    CutState* hs = c->h_state;
    const int64_t log_n = hs->log_n;
    std::memset(hs, 0, sizeof(CutState));
    hs->status = kRunning;
    hs->print_steps = print_steps ? 1 : 0;
    hs->max_iters = max_iters;
    hs->hard_cap = hard_cap;
    hs->log_n = log_n;
    hs->log_cap = c->log_cap;
    LPR_HIP(hipMemcpyAsync(c->state, hs, sizeof(CutState), hipMemcpyHostToDevice, s));
    const int batch = 16;
    for (;;) {
        for (int k = 0; k < batch; ++k) {
            hipLaunchKernelGGL(k_cut_select, dim3(1), dim3(1024), 0, s, t->T, t->ld, t->rows,
                               t->cols, t->rowbuf, t->colbuf, c->log, c->state, mode);
            cut_launch_update(t, 1);
        }
        LPR_HIP(hipGetLastError());
        LPR_HIP(hipMemcpyAsync(hs, c->state, sizeof(CutState), hipMemcpyDeviceToHost, s));
        LPR_HIP(hipStreamSynchronize(s));
        if (hs->status != kRunning) break;
    }
    if (pivots) *pivots = hs->done;
    return hs->status;
}

// needDual / needPrimal / anyFractional of the tableau as it stands -> h_state->scratch[2..4]
int cut_read_flags(lpr_tableau* t) {
    lpr_cut_ctx* c = static_cast<lpr_cut_ctx*>(t->cut);
    hipStream_t s = t->eng->stream;
    hipLaunchKernelGGL(k_cut_flags, dim3(1), dim3(1024), 0, s, t->T, t->ld, t->rows, t->cols,
                       c->state);
    LPR_HIP(hipGetLastError());
    LPR_HIP(hipMemcpyAsync(c->h_state, c->state, sizeof(CutState), hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    return LPR_OK_OPTIMAL;
}

// lpr_dual_solve / lpr_primal2_solve after their argument checks
int cut_solve_entry(lpr_tableau* t, int mode, int max_iters, int print_steps, int64_t hard_cap,
                    lpr_solve_result* res) {
    LPR_HIP(hipSetDevice(t->eng->device));
    int rc = cut_ensure(t);
    if (rc != LPR_OK_OPTIMAL) return rc;
    int64_t piv = 0;
    const int st = cut_run_solver(t, mode, max_iters, print_steps, hard_cap, &piv);
    if (st < 0) return st;
    res->status = st;
    res->block = 1;
    res->pivots = piv;
    res->total_pivots = piv;
    res->z = 0.0;
    LPR_HIP(hipMemcpy(&res->z, t->T + (t->cols - 1), sizeof(double), hipMemcpyDeviceToHost));
    return st;
}

}  // namespace

void lpr_cut_release(lpr_tableau* t) {  // called from release_device (lpr_engine.hip)
    lpr_cut_ctx* c = static_cast<lpr_cut_ctx*>(t->cut);
    if (!c) return;
    hipFree(c->state);
    hipFree(c->log);
    if (c->h_state) hipHostFree(c->h_state);
    delete c;
    t->cut = nullptr;
}

#define LPR_LIVE_T(t)                                                            \
    do {                                                                         \
        if (!(t) || !(t)->eng) {                                                 \
            set_error("tableau handle is null or its engine has been closed");   \
            return LPR_BAD_ARGUMENT;                                             \
        }                                                                        \
    } while (0)

extern "C" {

int lpr_dual_solve(lpr_tableau* t, int max_iters, int print_steps, int64_t hard_cap,
                   lpr_solve_result* res) {
    LPR_LIVE_T(t);
    if (!res || t->rows < 2) {
        set_error("lpr_dual_solve: no constraint rows");  // ArgumentException :17
        return LPR_BAD_ARGUMENT;
    }
    return cut_solve_entry(t, kCutDual, max_iters, print_steps, hard_cap, res);
}

int lpr_primal2_solve(lpr_tableau* t, int max_iters, int print_steps, int64_t hard_cap,
                      lpr_solve_result* res) {
    LPR_LIVE_T(t);
    if (!res || t->rows < 2) {
        set_error("lpr_primal2_solve: no constraint rows");  // ArgumentException :27
        return LPR_BAD_ARGUMENT;
    }
    return cut_solve_entry(t, kCutPrimal2, max_iters, print_steps, hard_cap, res);
}

int lpr_cutting_plane(lpr_tableau* t, int max_cuts, int64_t hard_cap, int32_t* exit_code,
                      int32_t* cuts) {
    LPR_LIVE_T(t);
    if (!exit_code || t->rows < 2) {
        set_error("lpr_cutting_plane: no constraint rows");  // ArgumentException :68
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipSetDevice(t->eng->device));
    int rc = cut_ensure(t);
    if (rc != LPR_OK_OPTIMAL) return rc;
    if (max_cuts <= 0) max_cuts = 64;
    lpr_cut_ctx* c = static_cast<lpr_cut_ctx*>(t->cut);
    hipStream_t s = t->eng->stream;
    CutState* hs = c->h_state;
    int ncuts = 0, ex = 5;
    for (;;) {
        if (ncuts >= max_cuts) {
            // do not add a cut we are not allowed to; but "all integral" still wins (exit 1)
            rc = cut_read_flags(t);
            if (rc != LPR_OK_OPTIMAL) return rc;
            ex = hs->scratch[4] ? 6 : 1;
            break;
        }
        rc = tableau_reserve_rows(t, t->rows + 1);  // the cut appends one row
        if (rc != LPR_OK_OPTIMAL) return rc;
        // steps 1-6 (+ staging of the pivot on the cut)
        hs->status = LPR_OK_OPTIMAL;
        LPR_HIP(hipMemcpyAsync(&c->state->log_n, &hs->log_n, 2 * sizeof(int64_t),
                               hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_cut_add, dim3(1), dim3(1024), 0, s, t->T, t->ld, t->rows, t->cols,
                           t->rowbuf, t->colbuf, c->log, c->state);
        LPR_HIP(hipGetLastError());
        LPR_HIP(hipMemcpyAsync(hs, c->state, sizeof(CutState), hipMemcpyDeviceToHost, s));
        LPR_HIP(hipStreamSynchronize(s));
        if (hs->scratch[0] < 0) { ex = 1; break; }  // "All RHS are integers" :87-91
        t->rows += 1;                                // the cut row is part of the tableau now
        ncuts += 1;
        if (hs->scratch[1] == -1) { ex = 2; break; }  // no valid pivot column :134-138
        if (hs->scratch[1] == -2) { ex = 3; break; }  // pivot too small :146-150
        cut_launch_update(t, 0);                      // step 7
        rc = cut_read_flags(t);
        if (rc != LPR_OK_OPTIMAL) return rc;
        bool needDual = hs->scratch[2] != 0, needPrimal = hs->scratch[3] != 0;
        if (needDual) {  // :186-194, printSteps: true
            const int st = cut_run_solver(t, kCutDual, 10000, 1, hard_cap, nullptr);
            if (st < 0) return st;
            if (st == LPR_PIVOT_TOO_SMALL) { ex = 7; break; }
            if (st != LPR_OK_OPTIMAL) { ex = 4; break; }
            rc = cut_read_flags(t);
            if (rc != LPR_OK_OPTIMAL) return rc;
            needPrimal = hs->scratch[3] != 0;
        }
        if (needPrimal) {  // :196-212; the result of Solve is ignored by the C#
            const int st = cut_run_solver(t, kCutPrimal2, 10000, 1, hard_cap, nullptr);
            if (st < 0) return st;
            if (st == LPR_PIVOT_TOO_SMALL) { ex = 7; break; }
        }
        rc = cut_read_flags(t);
        if (rc != LPR_OK_OPTIMAL) return rc;
        if (!hs->scratch[3] && !hs->scratch[2]) {  // :215
            if (hs->scratch[4]) continue;           // another Gomory cut (:217-222)
            ex = 0;                                 // "Displayed the Optimal Tableau" :224
            break;
        }
        ex = 5;  // "Cutting-plane step finished" :228
        break;
    }
    *exit_code = ex;
    if (cuts) *cuts = ncuts;
    return LPR_OK_OPTIMAL;
}

int lpr_cut_log_read(lpr_tableau* t, int32_t* triples, int64_t cap, int64_t* count) {
    LPR_LIVE_T(t);
    if (!count || cap < 0) return LPR_BAD_ARGUMENT;
    lpr_cut_ctx* c = static_cast<lpr_cut_ctx*>(t->cut);
    int64_t k = c ? c->h_state->log_n : 0;
    if (c && k > c->log_cap) k = c->log_cap;
    if (k > cap) k = cap;
    *count = k;
    if (k == 0 || !triples) return LPR_OK_OPTIMAL;
    LPR_HIP(hipSetDevice(t->eng->device));
    LPR_HIP(hipMemcpy(triples, c->log, (size_t)k * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return LPR_OK_OPTIMAL;
}

}  // extern "C"
