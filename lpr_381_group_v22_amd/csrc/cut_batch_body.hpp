// cut_batch_body.hpp -- the one text of the batched cutting plane's state machine (DESIGN.md
// sections 15 and 24), behind template <bool kLds, bool kNarr>: cut_batch_kernels.hip expands it
// with kNarr = false (k_cut_batch) and cut_batch_narr_kernels.hip with kNarr = true
// (k_cut_batch_narr).  Included once at file scope it gives the helpers; included again inside a
// kernel with LPR_CUT_BATCH_BODY_TEXT defined it gives the kernel's text.  Every item is taken through
//   CuttingPlaneSolver.CuttingPlaneSolution  IntegerProgramming/CuttingPlaneSolver.cs:64-229
//   DualSimplexSolver.Solve                  Simplex/DualSimplex.cs:14-114
//   PrimalSimplexSolver2.Solve               Simplex/PrimalSimplexSolver2.cs:46-97
// with the rules of cut_kernels.hip (k_cut_select, k_cut_add, k_cut_update, k_cut_flags and the
// host loop of lpr_cutting_plane): the same bits as that call gives on a fresh lpr_tableau.
//
// Under kNarr the body also keeps what the console text of those three sources needs, in the
// layout of cut_narr_layout.hpp: lane 0 pushes an event on every branch the text depends on, and
// the lane that gives a tableau element its final value also stores it to the item's record -- a
// second store, not a second pass.  No lane reads a record; narration adds no fence and no
// barrier.  With kNarr = false every narration step is compiled out.
#ifndef LPR_CUT_BATCH_BODY_HPP
#define LPR_CUT_BATCH_BODY_HPP

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

// One event of item `c` (cut_narr_layout.hpp): every lane advances the cursor, lane 0 stores.
__device__ __forceinline__ void cut_narr_emit(CutNarrDesc& c, int32_t* __restrict__ ev, int kind,
                                              int a, int b, int rows_now) {
    const int64_t at = cut_narr_event(c);
    if (threadIdx.x == 0 && at >= 0) {
        int32_t* e = ev + 4 * (c.ev_off + at);
        e[0] = kind;
        e[1] = a;
        e[2] = b;
        e[3] = rows_now;
    }
}

// The cursors of one item into registers and back, field by field; the offsets and capacities
// are the host's and are not written.
__device__ __forceinline__ CutNarrDesc cut_narr_load(const CutNarrDesc* __restrict__ p) {
    CutNarrDesc c;
    c.ev_off = p->ev_off;
    c.ev_n = p->ev_n;
    c.data_off = p->data_off;
    c.kp.cap = p->kp.cap;
    c.kp.cur = p->kp.cur;
    c.kp.made_d = p->kp.made_d;
    c.kp.made_n = p->kp.made_n;
    c.kp.kept_n = p->kp.kept_n;
    c.ev_cap = p->ev_cap;
    c.pad = 0;
    return c;
}
__device__ __forceinline__ void cut_narr_store(CutNarrDesc* __restrict__ p, const CutNarrDesc& c) {
    p->ev_n = c.ev_n;
    p->kp.cur = c.kp.cur;
    p->kp.made_d = c.kp.made_d;
    p->kp.made_n = c.kp.made_n;
    p->kp.kept_n = c.kp.kept_n;
}

// One more block of n doubles of item `c`: where the lanes store it, or nullptr where it is only
// counted.
__device__ __forceinline__ double* cut_narr_block(CutNarrDesc& c, double* __restrict__ data,
                                                  int64_t n) {
    const int64_t at = kept_push(c.kp, n);
    return at >= 0 ? data + c.data_off + at : nullptr;
}

}  // namespace lpr

#endif  // LPR_CUT_BATCH_BODY_HPP

#ifdef LPR_CUT_BATCH_BODY_TEXT
// ---- the text of the kernel: template <bool kLds, bool kNarr> ------------------------------------
// One item, by the 256 lanes of its workgroup: a resumable state machine; at most `call.chunk`
// pivots per launch; the tableau in LDS (kLds, form G) or in the item's slice of the global slab
// (form H).  A cut appends one row to the compact tableau (:104-110): a write past its end, no
// restride.
//
// This part is expanded INSIDE the two __global__ templates (k_cut_batch, k_cut_batch_narr), not
// called: `desc`, `slab`, `logs`, `call`, `idx_in`, `n_in`, `idx_out`, `n_out` are the kernel's own
// __restrict__ arguments, `kLds` its template parameter, and `kNarr` / `narr` what the kernel
// declares in front of the #include (false and an empty CutNarr in the un-narrated one).  As an
// inlined function the same text gave the un-narrated kernels another instruction stream (the
// no-alias attributes of the kernel arguments did not reach it); expanded here, k_cut_batch
// compiles to the stream it had before the text moved.
{
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
    // the narration cursors, uniform too: every lane advances its copy, lane 0 stores it back
    CutNarrDesc nc;
    if constexpr (kNarr) nc = cut_narr_load(narr.desc + k);
    int exit_b = 0;  // the column of an exit-3 event
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
        int ended_hard = 0;               // ... by call.hard_cap

        if (phase == kCutPhaseAdd) {
            // "Initial tableau:" (:74) is printed from the state as it stands here
            if constexpr (kNarr) cut_narr_emit(nc, narr.ev, kCutEvLevel, 0, 0, R);
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
            if constexpr (kNarr) {
                cut_narr_emit(nc, narr.ev, kCutEvCut, best.i, 0, R + 1);
                double* const rec = cut_narr_block(nc, narr.data, C);
                for (int j = tid; j < C; j += 256) {
                    const double v = -cut_frac(src[j]);
                    cut[j] = v;
                    if (rec) rec[j] = v;
                }
            } else {
                for (int j = tid; j < C; j += 256) cut[j] = -cut_frac(src[j]);
            }
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
            // again when it resumes.  Nothing of this pivot has been pushed yet.
            if (used >= call.chunk) break;
            const bool solver = kind != kCutKindCut;
            if (solver && call.hard_cap > 0 && done >= call.hard_cap) {
                ended = LPR_PIVOT_LIMIT;
                ended_hard = 1;
            }
            const double piv = T[(size_t)pr * C + pc];
            if (ended == kRunning && fabs(piv) <= kCutEps) {
                if (!solver) {
                    // :145-150.  Not reachable: the fold only takes columns with a < -EPS.  Kept
                    // because the C# and lpr_cutting_plane keep it.
                    code = kCutExitSmallPivot;
                    exit_b = pc;
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
                double* rec = nullptr;  // the block of the tableau after this pivot
                if constexpr (kNarr) {
                    cut_narr_emit(nc, narr.ev, kCutEvPivot + kind,
                                  (kind == kCutPrimal2) ? pr : pr - 1, pc, R);
                    rec = cut_narr_block(nc, narr.data, (int64_t)R * C);
                }
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
                                // One computation.  Under kNarr the lane also stores the
                                // element's final value to the record: the pivot row's, the new
                                // value, or the value it loaded where the row is left as it is.
                                if (ii[u] == pr) {
                                    const double out = prow[jj[u]];
                                    T[x] = out;
                                    if constexpr (kNarr) {
                                        if (rec) rec[x] = out;
                                    }
                                } else {
                                    const double f = fcol[ii[u]];
                                    const bool skip = nan_updates ? (fabs(f) <= kCutEps)
                                                                  : !(fabs(f) > kCutEps);
                                    if (!skip) {
                                        const double prod = f * prow[jj[u]];  // rounded: no FMA
                                        const double out = v[u] - prod;
                                        T[x] = out;
                                        if constexpr (kNarr) {
                                            if (rec) rec[x] = out;
                                        }
                                    } else {
                                        if constexpr (kNarr) {
                                            if (rec) rec[x] = v[u];
                                        }
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
                    if constexpr (kNarr) {
                        if (phase != kCutPhaseClosing)
                            cut_narr_emit(nc, narr.ev, kCutEvSolveBegin,
                                          phase == kCutPhaseDual ? kCutDual : kCutPrimal2, 0, R);
                    }
                } else {
                    ++done;
                    // `if (iter >= maxIters) return false` comes after the pivot (:108 / :90)
                    if (iter >= call.max_iters) ended = LPR_PIVOT_LIMIT;
                }
            }
        }

        if (ended != kRunning) {  // an inner solve has returned
            if constexpr (kNarr) cut_narr_emit(nc, narr.ev, kCutEvSolveEnd, ended, ended_hard, R);
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
                if constexpr (kNarr) {
                    if (phase == kCutPhasePrimal2)
                        cut_narr_emit(nc, narr.ev, kCutEvSolveBegin, kCutPrimal2, 0, R);
                }
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
    if constexpr (kNarr) {
        if (code != kRunning) cut_narr_emit(nc, narr.ev, kCutEvExit, code, exit_b, R);
        if (tid == 0) cut_narr_store(narr.desc + k, nc);
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
#endif  // LPR_CUT_BATCH_BODY_TEXT
