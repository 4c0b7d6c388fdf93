// sens_batch_kernels.hip -- the sensitivity scenario batch: many what-if
// scripts over one solved model per launch, each applied with the rules of SensitivityAnalyzer
// (SensitivityAnalysis/SensitivityAnalyzer.cs), the same bits as lpr_sens_* calls on a fresh
// handle and the oracle give for that script alone.
//
//   k_sens_batch<kLds, kGrow>
//                        one 256-lane workgroup per scenario runs its script as a resumable state
//                        machine: the edits (:300-321 :362-393 :427-470 :502-531),
//                        RebuildBasicsFromTableau (:706-723), DualSimplexIfNeeded (:168-201),
//                        ReOptimize (:121-166), Pivot (:98-119); at most `chunk` pivots per
//                        launch; the tableau in LDS (form G) or in the global slab (form H).
//                        kGrow (lpr_sens_batch_create_grow): the shape is the scenario's own, and
//                        AddNewActivity (:534-584) / AddNewConstraint (:609-659) grow it in place
//   k_sens_batch_init    the base state copied into every scenario
//   k_sens_batch_from_models
//                        lpr_sens_batch_from_batch: the analyzer's constructor (:22-39) per
//                        scenario on the final tableau of an LP of a solved LP batch
#include "batch_device.hpp"
#include "sens_batch_common.hpp"
#include "sens_rules.hpp"

#pragma clang fp contract(off)

namespace lpr {

// GetBasicRow (:69-84) of column j by one lane (the column scans of :706-723 and :160-165)
__device__ __forceinline__ int column_basic_row(const double* T, int R, int C, int j) {
    int c = 0, rs = 0;
    for (int i = 1; i < R; ++i) basic_row_step(above_eps(T[(size_t)i * C + j]), i, c, rs);
    return basic_row_verdict(c, rs, T + j, C);
}

// The membership counts that shadow basicVars, counted again from its m entries
__device__ __forceinline__ void block_recount(const int32_t* basic, int m, int32_t* bcount, int C) {
    for (int j = threadIdx.x; j < C; j += 256) bcount[j] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += 256) {
        const int b = basic[i];
        if (b >= 0 && b < C) atomicAdd(&bcount[b], 1);
    }
    __syncthreads();
}

// RebuildBasicsFromTableau (:706-723) by the whole workgroup: basicVars[i] is the first column
// whose GetBasicRow is i + 1, -1 where there is none, and the membership counts are counted again
// from it.  basic (R - 1 entries) and bcount (C entries) may lie in LDS or in global memory.
__device__ __forceinline__ void block_rebuild_basics(const double* T, int R, int C, int32_t* basic,
                                                     int32_t* bcount) {
    const int tid = threadIdx.x, m = R - 1, rhs = C - 1;
    for (int i = tid; i < m; i += 256) basic[i] = kSensNoBasic;
    for (int j = tid; j < C; j += 256) bcount[j] = 0;
    __syncthreads();
    for (int j = tid; j < rhs; j += 256) {  // the first such column per row
        const int r = column_basic_row(T, R, C, j);
        if (r >= 1) atomicMin(&basic[r - 1], j);
    }
    __syncthreads();
    for (int i = tid; i < m; i += 256) {
        const int b = basic[i];
        if (b == kSensNoBasic)
            basic[i] = -1;
        else
            atomicAdd(&bcount[b], 1);
    }
    __syncthreads();
}

// A compact R x C tableau re-strided to R2 x C2 >= R x C where it lies; value(i, j) gives entry
// (i, j) of the grown tableau from the old one, and reads an old entry only at a flat index at or
// below the new one's (columns and rows are inserted, never removed).
//   G: in place in LDS, the new flat indices in chunks of 256 from the last to the first.  A
//      chunk is loaded into registers, then a barrier, then stored: the stores of a chunk land at
//      or above its base, and every later chunk loads from below that base.
//   H: through the scenario's alt slice and back.  No ChangeRHS snapshot is alive at an edit
//      boundary, so alt is free, and cur stays the live tableau.
template <bool kLds, class F>
__device__ __forceinline__ void grow_tableau(double* T, double* alt, int R2, int C2, F value) {
    const int N2 = R2 * C2, tid = threadIdx.x;
    if constexpr (kLds) {
        for (int base = ((N2 - 1) / 256) * 256; base >= 0; base -= 256) {
            const int y = base + tid;
            double v = 0.0;
            if (y < N2) {
                const int i = y / C2;
                v = value(i, y - i * C2);
            }
            __syncthreads();
            if (y < N2) T[y] = v;
        }
    } else {
        for (int y = tid; y < N2; y += 256) {
            const int i = y / C2;
            alt[y] = value(i, y - i * C2);
        }
        __syncthreads();
        for (int y = tid; y < N2; y += 256) T[y] = alt[y];
    }
    __syncthreads();
}

template <bool kLds, bool kGrow>
__global__ __launch_bounds__(256) void k_sens_batch(SensBatchView vw,
                                                    const int32_t* __restrict__ idx_in, int n_in,
                                                    int32_t* __restrict__ idx_out,
                                                    int32_t* __restrict__ n_out, int chunk) {
    extern __shared__ double smem[];
    __shared__ double red_v[8];
    __shared__ int red_i[8];
    __shared__ int slot[8];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_in) return;
    const int k = idx_in[blockIdx.x];
    SensScenario* const d = vw.desc + k;
    // strides and the LDS carve-up: the batch's maximal shape; indexing: the scenario's own
    const int SR = vw.R, SC = vw.C;
    int R = SR, C = SC;
    if constexpr (kGrow) {
        R = d->R;
        C = d->C;
    }
    int m = R - 1, rhs = C - 1, RC = R * C;
    double* const cur = vw.cur + (size_t)k * SR * SC;
    double* const alt = vw.alt + (size_t)k * SR * SC;
    int32_t* const g_basic = vw.basic + (size_t)k * (SR - 1);
    int32_t* const g_bcount = vw.bcount + (size_t)k * SC;
    int32_t* const g_snap = vw.snap + (size_t)k * (SR - 1 + SC);
    double* const g_sol = vw.sol + (size_t)k * vw.sol_cap;
    int32_t* const g_log = vw.log + (size_t)k * 3 * vw.log_cap;

    // LDS: [tableau (G)] factor column (R), pivot row (C), membership counts (C), basicVars (R - 1);
    // row-indexed data is staged in the factor column, column-indexed data in the pivot row
    double* T;
    double* fcol;
    if constexpr (kLds) {
        T = smem;
        fcol = smem + SR * SC;
    } else {
        T = cur;
        fcol = smem;
    }
    double* const prow = fcol + SR;
    int32_t* const bcount = reinterpret_cast<int32_t*>(prow + SC);
    int32_t* const basic = bcount + SC;

    // the descriptor, uniform over the workgroup
    double z = d->z, old_z = d->old_z;
    const int64_t edit_off = d->edit_off, pivot_stop = d->pivot_stop;
    int64_t pivots = d->pivots, edit_pivots = d->edit_pivots, log_n = d->log_n;
    const int nedits = d->nedits;
    int edit = d->edit, phase = d->phase, it_d = d->iter_dual, it_p = d->iter_primal;
    int nsol = d->nsol;
    bool dirty = false;  // G: the LDS tableau differs from the cur slice
    if constexpr (kLds) {
        const double* src = d->in_alt ? alt : cur;
        dirty = d->in_alt != 0;
        for (int x = tid; x < RC; x += 256) T[x] = src[x];
    }
    for (int j = tid; j < C; j += 256) bcount[j] = g_bcount[j];
    for (int i = tid; i < m; i += 256) basic[i] = g_basic[i];
    __syncthreads();

    int32_t status = kRunning;
    int done = 0, begun = 0;  // pivots and edits of this launch
    while (status == kRunning) {
        if (phase == kPhaseApply) {
            if (edit >= nedits) {
                status = LPR_OK_OPTIMAL;
                break;
            }
            if (begun >= kSensBatchEditsPerLaunch) break;
            ++begun;
            const lpr_sens_edit e = vw.edits[edit_off + edit];
            edit_pivots = 0;
            it_d = 0;
            it_p = 0;
            bool valid = true;
            int refused = LPR_SENS_INVALID_INDEX;  // the outcome of an edit that is not valid
            if (e.op == LPR_SENS_EDIT_RESOLVE_ALL) {
                phase = kPhaseRebuild;
            } else if (e.op == LPR_SENS_EDIT_NONBASIC_CBAR) {  // :306-318
                valid = e.a >= 0 && e.a < rhs && bcount[e.a] == 0;
                if (valid) {
                    if (tid == 0) T[e.a] = e.v;
                    phase = kPhaseRebuild;
                }
            } else if (e.op == LPR_SENS_EDIT_BASIC) {  // :368-388
                valid = e.a >= 0 && e.a < rhs && bcount[e.a] > 0;
                int r = -1;
                if (valid) r = block_basic_row<256>(T, R, C, e.a, slot);
                valid = valid && r >= 1;  // "Could not locate basic row." :379
                if (valid) {
                    for (int j = tid; j < C; j += 256) {  // j < C - 1, then the RHS entry
                        const double prod = e.v * T[(size_t)r * C + j];
                        T[j] = T[j] + prod;
                    }
                    __syncthreads();
                    z = T[rhs];
                    phase = kPhaseRebuild;
                }
            } else if (e.op == LPR_SENS_EDIT_RHS) {  // :430-451
                valid = e.a >= 1 && e.a < R;
                if (valid) {
                    // snapshot (:437-439): tableau, finalZ, basicVars and the counts that shadow it
                    if constexpr (kLds) {
                        if (dirty)
                            for (int x = tid; x < RC; x += 256) cur[x] = T[x];
                        dirty = false;
                    } else {
                        for (int x = tid; x < RC; x += 256) alt[x] = T[x];
                    }
                    for (int i = tid; i < m; i += 256) g_snap[i] = basic[i];
                    for (int j = tid; j < C; j += 256) g_snap[m + j] = bcount[j];
                    old_z = z;
                    const double delta = e.v - T[(size_t)e.a * C + rhs];  // :441-442
                    const int sCol = (C - R) + (e.a - 1);
                    __syncthreads();  // every lane has read the old b
                    for (int i = tid; i < R; i += 256) {  // :445-450 (row 0: y_k * delta)
                        const double prod = delta * T[(size_t)i * C + sCol];
                        T[(size_t)i * C + rhs] = T[(size_t)i * C + rhs] + prod;
                    }
                    __syncthreads();
                    z = T[rhs];
                    phase = kPhaseDual;  // no rebuild (:455-456)
                }
            } else if (kGrow && e.op == LPR_SENS_EDIT_ADD_ACTIVITY) {  // :534-584
                // the batch's one rule of its own: a column that is not R - 1 long changes nothing
                // (lpr_sens_add_activity refuses the call)
                valid = e.b == m && C >= R;
                if (valid) {
                    const int n = C - R;
                    const double* a = vw.payload + e.a;
                    // yTa (:543-551): every product rounded on its own, then one lane adds them
                    // in index order from 0.0, as the loop does
                    for (int i = tid; i < m; i += 256) fcol[i] = T[n + i] * a[i];
                    __syncthreads();
                    if (tid == 0) {
                        double yTa = 0.0;
                        for (int i = 0; i < m; ++i) yTa = yTa + fcol[i];
                        red_v[0] = yTa - e.v;
                    }
                    __syncthreads();
                    const double cbar = red_v[0];
                    const int C0 = C;
                    // the column goes in front of the slacks (:553-570)
                    grow_tableau<kLds>(T, alt, R, C0 + 1, [&](int i, int j) -> double {
                        if (j == n) return i == 0 ? cbar : a[i - 1];
                        return T[(size_t)i * C0 + (j < n ? j : j - 1)];
                    });
                    C = C0 + 1;
                    rhs = C - 1;
                    RC = R * C;
                    for (int i = tid; i < m; i += 256)  // :575-577
                        if (basic[i] >= n) basic[i] += 1;
                    __syncthreads();
                    block_recount(basic, m, bcount, C);
                    phase = kPhaseRebuild;
                }
            } else if (kGrow && e.op == LPR_SENS_EDIT_ADD_CONSTRAINT) {  // :609-659
                valid = e.b == rhs;  // :616-617
                if (valid && rhs > 0) {  // tech[basicVars[pos]] throws on -1 (:640)
                    int bad = 0;
                    for (int i = tid; i < m; i += 256) bad |= basic[i] < 0 || basic[i] >= e.b;
                    if (__syncthreads_or(bad)) {
                        valid = false;
                        refused = LPR_SENS_INDEX_OUT_OF_RANGE;
                    }
                }
                if (valid) {
                    const double* tech = vw.payload + e.a;
                    // aX (:647-651) over the stored solutionVector: products, then one lane adds
                    const int lim = e.b < nsol ? e.b : nsol;
                    for (int j = tid; j < lim; j += 256) prow[j] = tech[j] * g_sol[j];
                    if (rhs > 0)  // checked above to lie in [0, ntech)
                        for (int i = tid; i < m; i += 256) fcol[i] = tech[basic[i]];
                    __syncthreads();
                    if (tid == 0) {
                        double aX = 0.0;
                        for (int j = 0; j < lim; ++j) aX = aX + prow[j];
                        red_v[0] = e.v - aX;
                    }
                    __syncthreads();
                    const double newb = red_v[0];
                    // the new row (:636-645): one lane per column, positions ascending
                    for (int j = tid; j < rhs; j += 256) {
                        double coeff = -tech[j];
                        for (int pos = 0; pos < m; ++pos) {
                            const double prod = fcol[pos] * T[(size_t)(pos + 1) * C + j];
                            coeff = coeff + prod;
                        }
                        prow[j] = coeff;
                    }
                    __syncthreads();
                    const int R0 = R, C0 = C, s0 = rhs;
                    // a zero column for the new slack in front of the RHS (:621-631), 1.0 in the
                    // new row (:652-653)
                    grow_tableau<kLds>(T, alt, R0 + 1, C0 + 1, [&](int i, int j) -> double {
                        if (i == R0) return j < s0 ? prow[j] : (j == s0 ? 1.0 : newb);
                        if (j == s0) return 0.0;
                        return T[(size_t)i * C0 + (j < s0 ? j : s0)];
                    });
                    R = R0 + 1;
                    C = C0 + 1;
                    m = R - 1;
                    rhs = C - 1;
                    RC = R * C;
                    if (tid == 0) basic[m - 1] = s0;  // basicVars.Add(newSlackCol) :656
                    __syncthreads();
                    block_recount(basic, m, bcount, C);
                    phase = kPhaseRebuild;
                }
            } else {  // LPR_SENS_EDIT_NONBASIC_COLUMN :505-526 (the create refused anything else)
                valid = e.a >= 1 && e.a < R && e.b >= 0 && e.b < rhs && bcount[e.b] == 0;
                if (valid) {
                    const double oldVal = T[(size_t)e.a * C + e.b];
                    const double yi = T[(C - R) + (e.a - 1)];
                    const double cbar = T[e.b];
                    __syncthreads();
                    if (tid == 0) {
                        const double delta = e.v - oldVal;
                        const double prod = yi * delta;
                        T[(size_t)e.a * C + e.b] = e.v;
                        T[e.b] = cbar + prod;
                    }
                    phase = kPhaseRebuild;
                }
            }
            __syncthreads();
            if (!valid) {  // the C# prints "Invalid ..." and returns; nothing changed
                if (tid == 0) {
                    vw.outcome[edit_off + edit] = refused;
                    vw.edit_piv[edit_off + edit] = 0;
                }
                ++edit;
                continue;
            }
            dirty = true;
        }

        if (phase == kPhaseRebuild) {
            block_rebuild_basics(T, R, C, basic, bcount);
            phase = kPhaseDual;
        }

        int outcome = kSensEditNotRun;  // set when the re-solve of this edit ends
        int leave = -1, enter = -1;
        if (phase == kPhaseDual) {
            // `bi < mostNeg - EPS`, mostNeg = 0.0 at the start, rows ascending (:174-178)
            for (int i = tid; i < R; i += 256) fcol[i] = T[(size_t)i * C + rhs];
            __syncthreads();
            leave = staged_eps_fold(fcol, 1, R, 0.0, slot);
            if (leave == -1) {
                phase = kPhasePrimal;  // break (:180) -> ReOptimize
            } else {
                if (done >= chunk) break;
                if (pivot_stop > 0 && pivots >= pivot_stop) {
                    status = LPR_PIVOT_LIMIT;
                    break;
                }
                if (it_d > kSensMaxIter) {  // `if (iter++ > maxIter) throw` (:183)
                    outcome = LPR_SENS_ITER_LIMIT;
                } else {
                    ++it_d;
                    // `a < -EPS: ratio = cbar / (-a); ratio < best - EPS`, columns ascending
                    const double* lrow = T + (size_t)leave * C;
                    for (int j = tid; j < rhs; j += 256) prow[j] = dual_ratio(T[j], lrow[j]);
                    __syncthreads();
                    enter = staged_eps_fold(prow, 0, rhs, INFINITY, slot);
                    if (enter == -1) outcome = LPR_SENS_INFEASIBLE;  // :197
                }
            }
        }
        if (phase == kPhasePrimal) {
            // IsOptimal (:86-96) and the entering column `rc < mostNeg`, first index (:131-141)
            int notopt = 0;
            Cand best = entering_start();
            for (int j = tid; j < rhs; j += 256) entering_step(bcount, T, j, notopt, best);
            notopt = __syncthreads_or(notopt);
            if (!notopt) {
                phase = kPhaseEpilogue;
            } else {
                if (done >= chunk) break;
                if (pivot_stop > 0 && pivots >= pivot_stop) {
                    status = LPR_PIVOT_LIMIT;
                    break;
                }
                if (it_p > kSensMaxIter) {  // `if (iter++ > maxIter) throw` (:126)
                    outcome = LPR_SENS_ITER_LIMIT;
                } else {
                    ++it_p;
                    best = dpp_block_cand_min(best, red_v, red_i);
                    enter = best.i;
                    if (enter < 0) {
                        phase = kPhaseEpilogue;  // `if (enter == -1) break` (:142)
                    } else {
                        // `a > EPS: ratio = rhs / a; ratio < best - EPS`, rows ascending (:144-150)
                        // (staged in the factor column's buffer, which is idle until the pivot)
                        for (int i = tid; i < R; i += 256)
                            fcol[i] = primal_ratio(T[(size_t)i * C + rhs], T[(size_t)i * C + enter]);
                        __syncthreads();
                        leave = staged_eps_fold(fcol, 1, R, INFINITY, slot);
                        if (leave == -1) outcome = LPR_SENS_UNBOUNDED;  // :151
                    }
                }
            }
        }

        if (outcome == kSensEditNotRun && leave >= 1 && enter >= 0) {
            // ---- Pivot :98-119 ----
            const double piv = T[(size_t)leave * C + enter];
            if (zero_pivot(piv)) {
                outcome = LPR_SENS_ZERO_PIVOT;  // :101
            } else {
                __syncthreads();  // the staged ratios have been read
                for (int i = tid; i < R; i += 256) fcol[i] = T[(size_t)i * C + enter];
                for (int j = tid; j < C; j += 256) prow[j] = ieee_div(T[(size_t)leave * C + j], piv);
                __syncthreads();
                // rows with |factor| < EPS are left untouched (:110); element-parallel over the
                // flattened tableau, four elements in flight per lane
                {
                    constexpr int U = 4;
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
                                if (ii[u] == leave) {
                                    T[x] = prow[jj[u]];
                                } else {
                                    const double f = fcol[ii[u]];
                                    if (!row_untouched(f)) {
                                        const double prod = f * prow[jj[u]];  // rounded: no FMA
                                        T[x] = v[u] - prod;
                                    }
                                }
                            }
                        }
                    }
                }
                if (tid == 0) {
                    basis_enter(basic, bcount, leave, enter, phase == kPhaseDual ? 0 : 1, g_log, log_n,
                                vw.log_cap);
                }
                ++log_n;
                ++pivots;
                ++edit_pivots;
                ++done;
                __syncthreads();
                continue;
            }
        }

        if (phase == kPhaseEpilogue) {  // :159-165
            z = T[rhs];
            for (int j = tid; j < rhs; j += 256) {
                const int r = column_basic_row(T, R, C, j);
                g_sol[j] = (r == -1) ? 0.0 : T[(size_t)r * C + rhs];
            }
            nsol = rhs;
            outcome = LPR_SENS_OK;
        }

        // ---- the edit has ended ----
        if (outcome != LPR_SENS_OK && vw.edits[edit_off + edit].op == LPR_SENS_EDIT_RHS) {
            // catch: restore (:462-469); solutionVector is not restored
            __syncthreads();
            if constexpr (kLds) {
                for (int x = tid; x < RC; x += 256) T[x] = cur[x];
                dirty = false;
            } else {
                for (int x = tid; x < RC; x += 256) T[x] = alt[x];
            }
            for (int i = tid; i < m; i += 256) basic[i] = g_snap[i];
            for (int j = tid; j < C; j += 256) bcount[j] = g_snap[m + j];
            z = old_z;
            outcome = LPR_SENS_ROLLED_BACK;
        }
        if (tid == 0) {
            vw.outcome[edit_off + edit] = outcome;
            vw.edit_piv[edit_off + edit] = edit_pivots;
        }
        ++edit;
        phase = kPhaseApply;
        __syncthreads();
    }

    // ---- write the scenario back ----
    __syncthreads();
    int in_alt = 0;
    if constexpr (kLds) {
        if (phase == kPhaseApply) {  // at an edit boundary: cur is the scenario's state
            if (dirty)
                for (int x = tid; x < RC; x += 256) cur[x] = T[x];
        } else {  // inside an edit: cur may be a ChangeRHS snapshot
            for (int x = tid; x < RC; x += 256) alt[x] = T[x];
            in_alt = 1;
        }
    }
    for (int j = tid; j < C; j += 256) g_bcount[j] = bcount[j];
    for (int i = tid; i < m; i += 256) g_basic[i] = basic[i];
    if (tid == 0) {
        d->z = z;
        d->old_z = old_z;
        d->pivots = pivots;
        d->edit_pivots = edit_pivots;
        d->log_n = log_n;
        d->edit = edit;
        d->phase = phase;
        d->iter_dual = it_d;
        d->iter_primal = it_p;
        d->nsol = nsol;
        d->in_alt = in_alt;
        d->status = status;
        if constexpr (kGrow) {
            d->R = R;
            d->C = C;
        }
        if (status == kRunning) idx_out[atomicAdd(n_out, 1)] = k;
    }
}

template __global__ void k_sens_batch<true, false>(SensBatchView, const int32_t*, int, int32_t*,
                                                   int32_t*, int);
template __global__ void k_sens_batch<false, false>(SensBatchView, const int32_t*, int, int32_t*,
                                                    int32_t*, int);
template __global__ void k_sens_batch<true, true>(SensBatchView, const int32_t*, int, int32_t*,
                                                  int32_t*, int);
template __global__ void k_sens_batch<false, true>(SensBatchView, const int32_t*, int, int32_t*,
                                                   int32_t*, int);

// The base state (R x C) into every scenario: the tableau compact (the base pads its rows to ld)
// into the cur slice, basicVars and its membership counts as stored, solutionVector.
__global__ __launch_bounds__(256) void k_sens_batch_init(SensBatchView vw, int count, int R, int C,
                                                         const double* __restrict__ baseT, int ld,
                                                         const int32_t* __restrict__ base_basic,
                                                         const int32_t* __restrict__ base_bcount,
                                                         const double* __restrict__ base_sol,
                                                         int nsol) {
    const int k = blockIdx.x;
    if (k >= count) return;
    const int tid = threadIdx.x;
    const int m = R - 1;
    double* T = vw.cur + (size_t)k * vw.R * vw.C;
    for_each_ij<256>(R, C, tid, [&](int x, int i, int j) { T[x] = baseT[(size_t)i * ld + j]; });
    for (int q = tid; q < m; q += 256) vw.basic[(size_t)k * (vw.R - 1) + q] = base_basic[q];
    for (int q = tid; q < C; q += 256) vw.bcount[(size_t)k * vw.C + q] = base_bcount[q];
    for (int q = tid; q < nsol; q += 256) vw.sol[(size_t)k * vw.sol_cap + q] = base_sol[q];
}

// new SensitivityAnalyzer(GetFinalTableau(), SolutionVector, FinalZ, BasicVariables)
// (Program.cs:147-151, SensitivityAnalyzer.cs:22-39) for every scenario of a batch made from an LP
// batch: one workgroup per scenario, on the LP src[k] names.  In order:
//   1. the LP's compact rows x cols tableau into the scenario's cur slice (:24), compact by the
//      scenario's own cols; row 0's last cell already holds finalZ, so :32 stores what is there
//   2. solutionVector = ExtractSolution() over the LP's n (extract_solution, select_common.hpp),
//      one lane per decision column; finalZ = tableau[0, cols - 1]
//   3. RebuildBasicsFromTableau (:35), not the LP batch's stored basis
//   4. the membership counts of basicVars
//   5. the descriptor fields that depend on the LP: R, C, nsol, z, old_z
// Steps 2 and 3 read the LP batch's slab, which nothing writes, so they do not wait for step 1.
// No division; nothing depends on arrival order (atomicMin / atomicAdd on int32 in LDS).
__global__ __launch_bounds__(256) void k_sens_batch_from_models(SensBatchView vw, int count,
                                                                const SensModelSrc* __restrict__ src,
                                                                const double* __restrict__ slab) {
    __shared__ int32_t s_basic[kBatchMaxRowsH];  // R - 1 entries used
    __shared__ int32_t s_bcount[kBatchMaxColsH];
    const int k = blockIdx.x;
    if (k >= count) return;
    const int tid = threadIdx.x;
    const SensModelSrc s = src[k];
    const int R = s.rows, C = s.cols, m = R - 1, rhs = C - 1, RC = R * C;
    const double* const S = slab + s.t_off;
    double* const T = vw.cur + (size_t)k * vw.R * vw.C;
    for (int x = tid; x < RC; x += 256) T[x] = S[x];
    double* const sol = vw.sol + (size_t)k * vw.sol_cap;
    for (int j = tid; j < s.n; j += 256) sol[j] = extract_solution(S, C, R, C, j);
    block_rebuild_basics(S, R, C, s_basic, s_bcount);
    int32_t* const g_basic = vw.basic + (size_t)k * (vw.R - 1);
    int32_t* const g_bcount = vw.bcount + (size_t)k * vw.C;
    for (int i = tid; i < m; i += 256) g_basic[i] = s_basic[i];
    for (int j = tid; j < C; j += 256) g_bcount[j] = s_bcount[j];
    if (tid == 0) {
        SensScenario* const d = vw.desc + k;
        const double z = S[rhs];
        d->R = R;
        d->C = C;
        d->nsol = s.n;
        d->z = z;
        d->old_z = z;
    }
}

// ------------------------------------------------------------------------------------------
// Launchers (declared in sens_batch_common.hpp).
int sens_batch_launch_from_models(hipStream_t s, const SensBatchView& vw, int count,
                                  const SensModelSrc* src, const double* slab) {
    hipLaunchKernelGGL(k_sens_batch_from_models, dim3(count), dim3(256), 0, s, vw, count, src, slab);
    char name[64];
    snprintf(name, sizeof(name), "k_sens_batch_from_models (%d scenarios)", count);
    return launch_checked(name);
}

namespace {

template <bool kLds, bool kGrow>
int sens_batch_launch_one(int form, hipStream_t s, const SensBatchView& vw, size_t lds,
                          const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out,
                          int chunk) {
    return batch_launch<&k_sens_batch<kLds, kGrow>>("k_sens_batch", "scenarios", form, s, n_in,
                                                    lds, kBatchMaxLdsG, vw, idx_in, n_in, idx_out,
                                                    n_out, chunk);
}

}  // namespace

int sens_batch_launch(int form, bool grow, hipStream_t s, const SensBatchView& vw,
                      const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out,
                      int chunk) {
    if (form == kFormG) {
        const size_t lds = sens_batch_footprint_g(vw.R, vw.C);
        return grow ? sens_batch_launch_one<true, true>(form, s, vw, lds, idx_in, n_in, idx_out,
                                                        n_out, chunk)
                    : sens_batch_launch_one<true, false>(form, s, vw, lds, idx_in, n_in, idx_out,
                                                         n_out, chunk);
    }
    const size_t lds = sens_batch_aux_bytes(vw.R, vw.C);
    return grow ? sens_batch_launch_one<false, true>(form, s, vw, lds, idx_in, n_in, idx_out,
                                                     n_out, chunk)
                : sens_batch_launch_one<false, false>(form, s, vw, lds, idx_in, n_in, idx_out,
                                                      n_out, chunk);
}

int sens_batch_launch_init(hipStream_t s, const SensBatchView& vw, int count, int R, int C,
                           const double* baseT, int ld, const int32_t* base_basic,
                           const int32_t* base_bcount, const double* base_sol, int nsol) {
    hipLaunchKernelGGL(k_sens_batch_init, dim3(count), dim3(256), 0, s, vw, count, R, C, baseT, ld,
                       base_basic, base_bcount, base_sol, nsol);
    return launch_checked("k_sens_batch_init");
}

}  // namespace lpr
