// cut_batch_kernels.hip -- the batched cutting plane: many option-4
// tableaux per launch, each taken through the whole recursion of
//   CuttingPlaneSolver.CuttingPlaneSolution  IntegerProgramming/CuttingPlaneSolver.cs:64-229
//   DualSimplexSolver.Solve                  Simplex/DualSimplex.cs:14-114
//   PrimalSimplexSolver2.Solve               Simplex/PrimalSimplexSolver2.cs:46-97
// with the rules of cut_kernels.hip (k_cut_select, k_cut_add, k_cut_update, k_cut_flags and the
// host loop of lpr_cutting_plane): the same bits as that call gives on a fresh lpr_tableau.
//
//   k_cut_batch<kLds>   one 256-lane workgroup per item runs it as a resumable state machine; at
//                       most `chunk` pivots per launch; the tableau in LDS (form G) or in the
//                       item's slice of the global slab (form H).  A cut appends one row to the
//                       compact tableau (:104-110): a write past its end, no restride.
//   k_cut_batch_load    the tableaux into their slices (lpr_cut_batch_create / _from_batch)
#include "batch_device.hpp"
#include "cut_batch_common.hpp"

#pragma clang fp contract(off)

namespace lpr {

// needDual / needPrimal / anyFractional (:183-184, :215-217), as k_cut_flags scans them
__device__ __forceinline__ void cut_scan_flags(const double* T, int R, int C, bool want_frac,
                                               int* neg_out, int* nonopt_out, int* frac_out) {
    int neg = 0, nonopt = 0, frac = 0;
    for (int i = 1 + (int)threadIdx.x; i < R; i += 256) {
        const double v = T[(size_t)i * C + (C - 1)];
        if (v < -kCutEps) neg = 1;
        if (want_frac && cut_frac(v) > kCutEps) frac = 1;
    }
    for (int j = threadIdx.x; j < C - 1; j += 256)
        if (T[j] < -kCutEps) nonopt = 1;
    *neg_out = __syncthreads_or(neg);
    *nonopt_out = __syncthreads_or(nonopt);
    *frac_out = __syncthreads_or(frac);
}

// |z_j / a_j| over `a_j < -EPS`, `|z_j| > EPS` of row `row`, staged for the dual ratio fold
// (DualSimplex.cs:53-70, CuttingPlaneSolver.cs:116-132); NaN = not a candidate
__device__ __forceinline__ void cut_stage_dual_ratios(const double* T, int C, int row,
                                                      double* stage) {
    const double* a_row = T + (size_t)row * C;
    for (int j = threadIdx.x; j < C - 1; j += 256) {
        const double a = a_row[j];
        double v = NAN;
        if (a < -kCutEps) {
            const double num = T[j];
            if (fabs(num) > kCutEps) v = fabs(ieee_div(num, a));
        }
        stage[j] = v;
    }
    __syncthreads();
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_cut_batch(CutBatchDesc* __restrict__ desc,
                                                   double* __restrict__ slab,
                                                   int32_t* __restrict__ logs, CutBatchCall call,
                                                   const int32_t* __restrict__ idx_in, int n_in,
                                                   int32_t* __restrict__ idx_out,
                                                   int32_t* __restrict__ n_out) {
    extern __shared__ double smem[];
    __shared__ double red_v[8];
    __shared__ int red_i[8];
    __shared__ int slot[8];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_in) return;
    const int k = idx_in[blockIdx.x];
    CutBatchDesc* const d = desc + k;
    const int C = d->cols, rcap = d->rcap, rhs = C - 1;
    int R = d->rows;
    double* const slice = slab + d->t_off;
    int32_t* const g_log = logs + 3 * d->log_off;

    // LDS: [tableau at capacity (G)] factor column (rcap), pivot row (cols).  Both vectors are
    // idle during selection: row-indexed candidates stage in the factor column, column-indexed
    // ones in the pivot row.
    double* T;
    double* fcol;
    if constexpr (kLds) {
        T = smem;
        fcol = smem + (size_t)rcap * C;
    } else {
        T = slice;
        fcol = smem;
    }
    double* const prow = fcol + rcap;

    // the descriptor, uniform over the workgroup
    const int log_cap = d->log_cap, cut_limit = d->cut_limit;
    int64_t log_n = d->log_n, iter = d->iter, done = d->done, pivots = d->pivots;
    int phase = d->phase, cuts = d->cuts;
    if constexpr (kLds) {
        const int RC = R * C;
        for (int x = tid; x < RC; x += 256) T[x] = slice[x];
    }
    __syncthreads();

    int code = kRunning;
    int used = 0;  // pivots of this launch
    while (code == kRunning) {
        int pr = -1, pc = -1, kind = -1;  // the pivot this pass has selected, if any
        int ended = kRunning;             // lpr_status of an inner solve that ends in this pass

        if (phase == kCutPhaseAdd) {
            // steps 1-2 (:76-96): the lexicographic (|frac(rhs) - 0.5|, index) minimum over the
            // rows with Frac(rhs) > EPS.  Strict, no EPS band: a candidate minimum, not a fold.
            Cand best;
            best.v = INFINITY;
            best.i = -1;
            for (int i = tid; i < R - 1; i += 256) {
                const double fr = cut_frac(T[(size_t)(i + 1) * C + rhs]);
                if (fr > kCutEps) {
                    const double key = fabs(fr - 0.5);
                    if (best.i < 0 || key < best.v) {  // ascending i per lane: the first stays
                        best.v = key;
                        best.i = i;
                    }
                }
            }
            best = group_cand_min<256>(best, red_v, red_i);
            if (best.i < 0) {  // "All RHS are integers" :87-91; wins over the cut limit, as in
                code = kCutExitIntegral;  // lpr_cutting_plane and the oracle
                break;
            }
            if (cuts >= cut_limit) {
                code = kCutExitMaxCuts;
                break;
            }
            // steps 3-5 (:99-110): -Frac of every entry, RHS included, appended as row R
            const double* src = T + (size_t)(best.i + 1) * C;
            double* cut = T + (size_t)R * C;
            for (int j = tid; j < C; j += 256) cut[j] = -cut_frac(src[j]);
            R += 1;
            cuts += 1;
            phase = kCutPhaseCutPivot;
            __syncthreads();
        }

        if (phase == kCutPhaseCutPivot) {
            // step 6 (:113-132): the dual ratio fold on the new row.  Its tie clause is dead for
            // the reason given at fold_dual_column (cut_kernels.hip): j ascends, and before the
            // first take best is +inf.
            pr = R - 1;
            cut_stage_dual_ratios(T, C, pr, prow);
            pc = staged_eps_fold(prow, 0, rhs, INFINITY, slot);
            if (pc < 0) {
                code = kCutExitNoColumn;  // :134-138
                break;
            }
            kind = kCutKindCut;
        } else if (phase == kCutPhaseDual) {
            // pivot row: `rhs < mostNeg - EPS`, mostNeg = 0.0 at the start, constraint rows
            // ascending (:29-37); tie clause dead, see k_cut_select
            for (int i = tid; i < R; i += 256) fcol[i] = T[(size_t)i * C + rhs];
            __syncthreads();
            pr = staged_eps_fold(fcol, 1, R, 0.0, slot);
            if (pr < 0) {
                ended = LPR_OK_OPTIMAL;  // "Dual phase complete" :40-44
            } else {
                cut_stage_dual_ratios(T, C, pr, prow);  // :53-70
                pc = staged_eps_fold(prow, 0, rhs, INFINITY, slot);
                if (pc < 0)
                    ended = LPR_INFEASIBLE_BASIS;  // return false :72-76
                else
                    kind = kCutDual;
            }
        } else if (phase == kCutPhasePrimal2) {
            // entering column: `c < mostNeg - EPS`, mostNeg = 0.0 at the start, columns ascending
            // (:102-117); tie clause dead, see k_cut_select
            for (int j = tid; j < rhs; j += 256) prow[j] = T[j];
            __syncthreads();
            pc = staged_eps_fold(prow, 0, rhs, 0.0, slot);
            if (pc < 0) {
                ended = LPR_OK_OPTIMAL;  // :54-60
            } else {
                // leaving row: `a > EPS`, `ratio > EPS && ratio < best - EPS`, rows ascending
                // (:120-141); the second operand of the C#'s `||` is never true, see k_cut_select
                for (int i = tid; i < R; i += 256) {
                    const double a = T[(size_t)i * C + pc];
                    double v = NAN;
                    if (a > kCutEps) {
                        const double ratio = ieee_div(T[(size_t)i * C + rhs], a);
                        if (ratio > kCutEps) v = ratio;
                    }
                    fcol[i] = v;
                }
                __syncthreads();
                pr = staged_eps_fold(fcol, 1, R, INFINITY, slot);
                if (pr < 0)
                    ended = LPR_UNBOUNDED;  // return false :63-68
                else
                    kind = kCutPrimal2;
            }
        }

        if (kind >= 0) {
            // The launch bound: an item stops only here, in front of a pivot, and selects it
            // again when it resumes.
            if (used >= call.chunk) break;
            const bool solver = kind != kCutKindCut;
            if (solver && call.hard_cap > 0 && done >= call.hard_cap) ended = LPR_PIVOT_LIMIT;
            const double piv = T[(size_t)pr * C + pc];
            if (ended == kRunning && fabs(piv) <= kCutEps) {
                if (!solver) {
                    // :145-150.  Not reachable: the fold only takes columns with a < -EPS.  Kept
                    // because the C# and lpr_cutting_plane keep it.
                    code = kCutExitSmallPivot;
                    break;
                }
                ended = LPR_PIVOT_TOO_SMALL;  // InvalidOperationException :155 / :148
            }
            if (ended == kRunning) {
                if (solver && call.print_steps) ++iter;  // ++iter inside `if (printSteps)` :94 / :75
                if (tid == 0 && log_n < log_cap) {
                    int32_t* e = g_log + 3 * log_n;
                    e[0] = kind;
                    e[1] = (kind == kCutPrimal2) ? pr : pr - 1;  // the C#'s own row numbering
                    e[2] = pc;
                }
                ++log_n;
                // ---- the pivot (DualSimplex.cs:150-178, PrimalSimplexSolver2.cs:145-164,
                // CuttingPlaneSolver.cs:145-176): the factor column first, the pivot row divided
                // by the saved element, every other row x - (f * p_j) with the product rounded
                __syncthreads();  // the staged candidates have been read
                for (int i = tid; i < R; i += 256) fcol[i] = T[(size_t)i * C + pc];
                for (int j = tid; j < C; j += 256) prow[j] = ieee_div(T[(size_t)pr * C + j], piv);
                __syncthreads();
                // The dual and cut pivots update a row on `|f| > EPS` (DualSimplex.cs:166,
                // CuttingPlaneSolver.cs:161): a NaN factor leaves its row.  PrimalSimplexSolver2
                // skips on `|f| <= EPS` (:160): a NaN factor updates it (CutState::nan_updates).
                const bool nan_updates = kind == kCutPrimal2;
                {
                    // element-parallel over the flattened tableau, four elements in flight
                    constexpr int U = 4;
                    const int RC = R * C;
                    const int di = 256 / C, dj = 256 - (256 / C) * C;
                    int i = tid / C, j = tid - (tid / C) * C;
                    for (int base = 0; base < RC; base += U * 256) {
                        double v[U];
                        int ii[U], jj[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int x = base + u * 256 + tid;
                            ii[u] = i;
                            jj[u] = j;
                            v[u] = (x < RC) ? T[x] : 0.0;
                            i += di;
                            j += dj;
                            if (j >= C) {
                                j -= C;
                                ++i;
                            }
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int x = base + u * 256 + tid;
                            if (x < RC) {
                                if (ii[u] == pr) {
                                    T[x] = prow[jj[u]];
                                } else {
                                    const double f = fcol[ii[u]];
                                    const bool skip = nan_updates ? (fabs(f) <= kCutEps)
                                                                  : !(fabs(f) > kCutEps);
                                    if (!skip) {
                                        const double prod = f * prow[jj[u]];  // rounded: no FMA
                                        T[x] = v[u] - prod;
                                    }
                                }
                            }
                        }
                    }
                }
                ++pivots;
                ++used;
                __syncthreads();
                if (!solver) {
                    // step 8 (:183-212): which clean-up solves the pivot on the cut calls for
                    int neg, nonopt, frac;
                    cut_scan_flags(T, R, C, false, &neg, &nonopt, &frac);
                    phase = neg ? kCutPhaseDual : (nonopt ? kCutPhasePrimal2 : kCutPhaseClosing);
                    iter = 0;
                    done = 0;
                } else {
                    ++done;
                    // `if (iter >= maxIters) return false` comes after the pivot (:108 / :90)
                    if (iter >= call.max_iters) ended = LPR_PIVOT_LIMIT;
                }
            }
        }

        if (ended != kRunning) {  // an inner solve has returned
            if (call.mode != kCutModeCuttingPlane) {
                code = ended;
                break;
            }
            if (ended == LPR_PIVOT_TOO_SMALL) {
                code = kCutExitException;
                break;
            }
            if (phase == kCutPhaseDual) {
                if (ended != LPR_OK_OPTIMAL) {
                    code = kCutExitDualFailed;  // :191
                    break;
                }
                int neg, nonopt, frac;  // needPrimal is read again after the dual (:196)
                cut_scan_flags(T, R, C, false, &neg, &nonopt, &frac);
                phase = nonopt ? kCutPhasePrimal2 : kCutPhaseClosing;
                iter = 0;
                done = 0;
            } else {
                phase = kCutPhaseClosing;  // the result of Solve is ignored (:200)
            }
        }

        if (phase == kCutPhaseClosing) {  // step 9 (:215-228)
            int neg, nonopt, frac;
            cut_scan_flags(T, R, C, true, &neg, &nonopt, &frac);
            if (!nonopt && !neg) {
                if (frac) {
                    phase = kCutPhaseAdd;  // another Gomory cut (:217-222)
                } else {
                    code = kCutExitOptimal;  // :224
                    break;
                }
            } else {
                code = kCutExitStepDone;  // :228
                break;
            }
        }
    }

    // ---- write the item back ----
    __syncthreads();
    if constexpr (kLds) {
        const int RC = R * C;
        for (int x = tid; x < RC; x += 256) slice[x] = T[x];
    }
    if (tid == 0) {
        d->log_n = log_n;
        d->iter = iter;
        d->done = done;
        d->pivots = pivots;
        d->z = T[rhs];
        d->rows = R;
        d->phase = phase;
        d->cuts = cuts;
        d->code = code;
        if (code == kRunning) idx_out[atomicAdd(n_out, 1)] = k;
    }
}

template __global__ void k_cut_batch<true>(CutBatchDesc*, double*, int32_t*, CutBatchCall,
                                           const int32_t*, int, int32_t*, int32_t*);
template __global__ void k_cut_batch<false>(CutBatchDesc*, double*, int32_t*, CutBatchCall,
                                            const int32_t*, int, int32_t*, int32_t*);

// Tableau k (rows x cols, compact, at src + src_off[k]) into the front of its slice; z of the
// descriptor with it.
__global__ __launch_bounds__(256) void k_cut_batch_load(CutBatchDesc* __restrict__ desc, int count,
                                                        const double* __restrict__ src,
                                                        const int64_t* __restrict__ src_off,
                                                        double* __restrict__ slab) {
    const int k = blockIdx.x;
    if (k >= count) return;
    CutBatchDesc* const d = desc + k;
    const int n = d->rows * d->cols;
    const double* from = src + src_off[k];
    double* to = slab + d->t_off;
    for (int x = threadIdx.x; x < n; x += 256) to[x] = from[x];
    if (threadIdx.x == 0) d->z = from[d->cols - 1];
}

// ------------------------------------------------------------------------------------------
// Launchers (cut_batch_engine.hip).  lds: the largest dynamic LDS an item of this list needs.
int cut_batch_launch(int form, hipStream_t s, CutBatchDesc* desc, double* slab, int32_t* logs,
                     const CutBatchCall& call, size_t lds, const int32_t* idx_in, int n_in,
                     int32_t* idx_out, int32_t* n_out) {
    static unsigned long long g_mask = 0;  // per device bit: the G attribute is set
    if (n_in <= 0) return LPR_OK_OPTIMAL;
    if (form == kFormG) {
        if (lds > kBatchMaxLdsG) {
            set_error("k_cut_batch: %zu bytes of LDS asked for in form G", lds);
            return LPR_BAD_ARGUMENT;
        }
        if (lds > ((size_t)64 << 10)) {
            const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&k_cut_batch<true>),
                                             kBatchMaxLdsG, &g_mask);
            if (rc != LPR_OK_OPTIMAL) return rc;
        }
        hipLaunchKernelGGL(k_cut_batch<true>, dim3(n_in), dim3(256), lds, s, desc, slab, logs,
                           call, idx_in, n_in, idx_out, n_out);
    } else {
        hipLaunchKernelGGL(k_cut_batch<false>, dim3(n_in), dim3(256), lds, s, desc, slab, logs,
                           call, idx_in, n_in, idx_out, n_out);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        set_error("k_cut_batch (form %d, %d items) failed to launch: %s", form, n_in,
                  hipGetErrorString(err));
        return LPR_DEVICE_ERROR;
    }
    return LPR_OK_OPTIMAL;
}

int cut_batch_launch_load(hipStream_t s, CutBatchDesc* desc, int count, const double* src,
                          const int64_t* src_off, double* slab) {
    hipLaunchKernelGGL(k_cut_batch_load, dim3(count), dim3(256), 0, s, desc, count, src, src_off,
                       slab);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        set_error("k_cut_batch_load failed to launch: %s", hipGetErrorString(err));
        return LPR_DEVICE_ERROR;
    }
    return LPR_OK_OPTIMAL;
}

}  // namespace lpr
