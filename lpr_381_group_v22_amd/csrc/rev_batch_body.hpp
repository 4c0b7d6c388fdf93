// rev_batch_body.hpp -- the loop of Solve() (RevisedPrimalSimplexSolver.cs:82-251) and
// ExtractSolution (:277-287) for one LP of a batch, stated once for the untraced kernels
// (rev_batch_kernels.hip) and the traced ones (rev_batch_trace_kernels.hip,
// section 21): rev_batch_run<NT, kLds, kTrace>.  The trace steps sit under `if constexpr (kTrace)`;
// with kTrace false nothing of them is compiled.
//
// Every sum is one lane's sequential chain in the C#'s index order from 0, each product rounded
// before it is added; the lanes of an LP share outputs, never a sum.
#pragma once

#include "rev_batch_common.hpp"
#include "batch_device.hpp"
#include "revised_select.hpp"

#pragma clang fp contract(off)

namespace lpr {

// Is pred true on any of the NT lanes of one LP?  (every lane gets the answer)
template <int NT>
__device__ __forceinline__ bool group_any(bool pred) {
    if constexpr (NT == kWave) return __ballot(pred) != 0ull;
    else return __syncthreads_or(pred) != 0;
}

// The entering fold (:105-121) over the staged values v = -rc (NaN: not a candidate), "take when
// v < best - EPS" from best = +inf over ascending index: one wave replays it as it is written.
template <int NT>
__device__ __forceinline__ int rev_batch_enter(const double* stage, int N, int lane, int* slot) {
    if constexpr (NT != kWave) {
        return staged_eps_fold(stage, 0, N, INFINITY, slot);
    } else {
        double best = INFINITY;
        int cur = -1;
        for (int b0 = 0; b0 < N; b0 += kWave) {
            const int idx = b0 + lane;
            const double x = (idx < N) ? stage[idx] : (double)NAN;
            unsigned long long alive = ~0ull;
            for (;;) {
                const unsigned long long hit = __ballot(x < best - kFoldEps) & alive;
                if (hit == 0ull) break;
                const int fl = __builtin_amdgcn_readfirstlane(__builtin_ctzll(hit));
                best = readlane_f64(x, fl);
                cur = b0 + fl;
                alive = (fl == kWave - 1) ? 0ull : (~0ull << (fl + 1));
            }
        }
        return cur;
    }
}

// The ratio fold (:154-176) over the staged ratios (NaN: u_i <= EPS), with its live tie clause:
// one wave replays the loop as it is written, 64 rows at a time; a ballot finds the first row
// after the last take that the loop would take next.
template <int NT>
__device__ __forceinline__ int rev_batch_ratio(const double* rat, const int32_t* bas, int m,
                                               int lane, int* slot) {
    int row = -1;
    if (NT == kWave || threadIdx.x < kWave) {
        double best = DBL_MAX;
        int brow = 0;
        for (int b0 = 0; b0 < m; b0 += kWave) {
            const int i = b0 + lane;
            const double ratio = (i < m) ? rat[i] : (double)NAN;
            const int bi = (i < m) ? bas[i] : 0;
            unsigned long long alive = ~0ull;
            for (;;) {
                const bool take = rev_ratio_take(ratio, best, row == -1, bi, brow);
                const unsigned long long hit = __ballot(take) & alive;
                if (hit == 0ull) break;
                const int fl = __builtin_amdgcn_readfirstlane(__builtin_ctzll(hit));
                best = readlane_f64(ratio, fl);
                brow = __builtin_amdgcn_readlane(bi, fl);
                row = b0 + fl;
                alive = (fl == kWave - 1) ? 0ull : (~0ull << (fl + 1));
            }
        }
        if (NT != kWave && lane == 0) *slot = row;
    }
    if constexpr (NT != kWave) {
        __syncthreads();
        row = *slot;
        __syncthreads();  // the slot is free for the next fold
    }
    return row;
}

// out[i] = sum over j ascending of M[i, j] * v[j], from 0 (MultiplyMatrixVector :398-410): lane i
// walks row i.  M in LDS: directly (odd ld, no bank conflict).  M in global memory: through tiles
// of NT rows x kRevBatchTileCols columns staged in LDS, so that the loads are contiguous runs.
// Padding never enters a sum (-0 + 0 * v is +0).
template <int NT, bool kLds>
__device__ __forceinline__ void rev_batch_rowmv(const double* __restrict__ M, int ld, int m,
                                                const double* v, double* out, double* tile,
                                                int lane) {
    if constexpr (kLds) {
        for (int i = lane; i < m; i += NT) {
            const double* row = M + (size_t)i * ld;
            double s = 0.0;
            for (int j = 0; j < m; ++j) s += row[j] * v[j];
            out[i] = s;
        }
    } else {
        constexpr int TJ = kRevBatchTileCols;
        for (int i0 = 0; i0 < m; i0 += NT) {
            const int i = i0 + lane;
            double s = 0.0;
            for (int j0 = 0; j0 < m; j0 += TJ) {
#pragma unroll
                for (int q = 0; q < TJ; ++q) {
                    const int t = lane + q * NT;
                    const int r = t / TJ, cj = t - (t / TJ) * TJ;
                    const bool ok = i0 + r < m && j0 + cj < m;
                    tile[r * (TJ + 1) + cj] = ok ? M[(size_t)(i0 + r) * ld + j0 + cj] : 0.0;
                }
                __syncthreads();
                if (i < m) {
                    const int w = (m - j0 < TJ) ? m - j0 : TJ;
                    const double* row = tile + lane * (TJ + 1);
                    for (int jj = 0; jj < w; ++jj) s += row[jj] * v[j0 + jj];
                }
                __syncthreads();
            }
            if (i < m) out[i] = s;
        }
    }
}

// rc_j = c_j - Dot(y, A_j) (:96-98): one lane down column j.
__device__ __forceinline__ double rev_batch_rc(const double* y, const double* A, int lda, int m,
                                               double cj, int j) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += y[i] * A[(size_t)i * lda + j];
    return cj - s;
}

// x of ExtractSolution (:277-283) / ComputeOriginalZFromCurrentBasis (:253-262) into xs[n]: zeros,
// then Math.Max(0.0, x_B[i]) (.NET Framework: `0.0 > v ? 0.0 : v`) at every structural basic.
template <int NT>
__device__ __forceinline__ void rev_batch_scatter_x(double* xs, int n, int m, const int32_t* bas,
                                                    const double* xB, int lane) {
    for (int j = lane; j < n; j += NT) xs[j] = 0.0;
    group_sync<NT, kFenceWave>();
    for (int i = lane; i < m; i += NT) {
        const int v = bas[i];
        if (v < n) {
            const double xb = xB[i];
            xs[v] = (0.0 > xb) ? 0.0 : xb;
        }
    }
    group_sync<NT, kFenceWave>();
}

// Dot(cOrig, x) (:284, :261), cOrig = -c for a minimisation: one lane's chain from 0.
__device__ __forceinline__ double rev_batch_z_original(const double* c, const double* xs, int n,
                                                       bool mn) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += (mn ? -c[j] : c[j]) * xs[j];
    return s;
}

// The part of a record that exists once B^-1 is final for it (basis, B^-1 and
// MultiplyMatrices(BInverse, A), :360): R[i,j] from +0.0 over k ascending, terms with
// |B^-1[i,k]| < EPS skipped, each product rounded before it is added (the expressions of
// k_rev_matmul_exact).  Consecutive lanes write consecutive addresses; in form H lane j reads
// consecutive A[k, j] and the B^-1 row is the same for the lanes of a row.
template <int NT>
__device__ __forceinline__ void rev_trace_tables(double* rec, int m, int n, const int32_t* bas,
                                                 const double* Binv, int ldb, const double* A,
                                                 int lda, int lane) {
    double* const post = rec + rev_trace_basis_post(m, n);
    for (int i = lane; i < m; i += NT) post[i] = (double)bas[i];
    double* const BA = rec + rev_trace_binva(m, n);
    for_each_ij<NT>(m, n, lane, [&](int x, int i, int j) {
        const double* row = Binv + (size_t)i * ldb;
        double s = 0.0;
        for (int k = 0; k < m; ++k) {
            const double aik = row[k];
            if (fabs(aik) < kRevEps) continue;
            const double p = aik * A[(size_t)k * lda + j];
            s = s + p;
        }
        BA[x] = s;
    });
    double* const BI = rec + rev_trace_binv(m, n);
    for_each_ij<NT>(m, m, lane, [&](int x, int i, int j) { BI[x] = Binv[(size_t)i * ldb + j]; });
}

// One LP per NT lanes; 256 / NT LPs per workgroup.  Everything the lanes of an LP share during a
// launch is in LDS (W, G) or ordered by workgroup barriers (H), so form W fences at wave scope.
// idx_in lists the LPs still running; an LP that is still running when its chunk is used up
// appends itself to idx_out (n_out counts them: the one word the host reads per launch).
//
// kTrace (section 21): record `iter` of the LP receives its pre-pivot part in the pass that makes
// pivot `iter`, while u, the staged ratios and the old basis are live, and its tables once B^-1
// is updated; x_B, y, rc and the two Z are what the top of the next pass computes anyway (:217-227
// recompute them with the operands of :89-102), so that pass -- in this launch or the next --
// completes the record.  The "Optimal" record is written whole on the optimal exit.  A record's
// lanes never read what other lanes wrote to it.
template <int NT, bool kLds, bool kTrace>
__device__ __forceinline__ void rev_batch_run(RevBatchDesc* __restrict__ desc,
                                              double* __restrict__ slab,
                                              int32_t* __restrict__ basis,
                                              int32_t* __restrict__ logs, double* __restrict__ xs,
                                              const int32_t* __restrict__ idx_in, int n_in,
                                              int32_t* __restrict__ idx_out,
                                              int32_t* __restrict__ n_out, int chunk, int slot,
                                              const RevBatchTrace tr) {
    extern __shared__ double smem[];
    __shared__ int s_slot;
    static_assert(kLds || NT == 256, "form H is one workgroup per LP");
    constexpr int kPerWg = 256 / NT;
    const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / NT);
    const int lane = (int)threadIdx.x % NT;
    const int q = blockIdx.x * kPerWg + sub;
    if (q >= n_in) return;  // uniform per LP (and per workgroup where NT == 256)
    const int k = idx_in[q];
    RevBatchDesc* d = desc + k;
    const int n = d->n, m = d->m, N = n + m;
    int64_t iter = d->iter;
    const int64_t max_iter = d->max_iter;
    const int log_cap = d->log_cap;
    int32_t* const bas_g = basis + d->b_off;
    int32_t* const lg = logs + 3 * d->log_off;
    double* const Bg = slab + d->s_off;
    double* const Ag = Bg + (size_t)m * m;
    double* const bg = Ag + (size_t)m * n;
    double* const cg = bg + m;
    double* const cBg = cg + n;
    double* const xBg = cBg + m;
    // the LP's records: record i at trec + i * tstride, kept while i < tr.cap
    double* trec = nullptr;
    int64_t tstride = 0;
    if constexpr (kTrace) {
        trec = tr.slab + tr.off[k];
        tstride = rev_trace_stride(m, n);
    }

    // ---- the LP's share of LDS ----
    double* p = smem + (size_t)sub * slot;
    const int ldb = kLds ? rev_batch_ld(m) : m, lda = kLds ? rev_batch_ld(n) : n;
    double* Binv = Bg;
    double* A = Ag;
    if constexpr (kLds) {
        Binv = p;
        p += (size_t)m * ldb;
        A = p;
        p += (size_t)m * lda;
    }
    double* const b = p;
    double* const cB = b + m;
    double* const xB = cB + m;
    double* const y = xB + m;     // then the staged ratios
    double* const u = y + m;      // then column r of E
    double* const prow = u + m;   // a_e, then the old pivot row of B^-1
    double* const c = prow + m;
    double* const stage = c + n;  // n + m
    int32_t* const bas = reinterpret_cast<int32_t*>(stage + N);
    uint8_t* const isb = reinterpret_cast<uint8_t*>(stage + N + (m + 1) / 2);
    double* const tile = stage + N + (m + 1) / 2 + (N + 7) / 8;  // H only

    if constexpr (kLds) {
        for_each_ij<NT>(m, m, lane, [&](int x, int i, int j) { Binv[i * ldb + j] = Bg[x]; });
        for_each_ij<NT>(m, n, lane, [&](int x, int i, int j) { A[i * lda + j] = Ag[x]; });
    }
    for (int i = lane; i < m; i += NT) {
        b[i] = bg[i];
        cB[i] = cBg[i];
        xB[i] = xBg[i];
        bas[i] = bas_g[i];
    }
    for (int j = lane; j < n; j += NT) c[j] = cg[j];
    for (int v = lane; v < N; v += NT) isb[v] = 0;
    group_sync<NT, kFenceWave>();
    for (int i = lane; i < m; i += NT) isb[bas[i]] = 1;  // the complement of nonBasicVariables
    group_sync<NT, kFenceWave>();

    int32_t status = kRunning;
    for (int pass = 0; pass < chunk; ++pass) {
        // ---- :89-91  x_B = B^-1 b; any x_B[i] < -EPS: infeasible basis ----
        rev_batch_rowmv<NT, kLds>(Binv, ldb, m, b, xB, tile, lane);
        group_sync<NT, kFenceWave>();
        bool bad = false;
        for (int i = lane; i < m; i += NT) bad = bad || xB[i] < -kRevEps;
        const bool infeasible = group_any<NT>(bad);
        // the record of the last pivot still lacks what :217-227 compute after UpdateBInverse
        double* post = nullptr;
        if constexpr (kTrace) {
            if (iter >= 1 && iter - 1 < tr.cap) post = trec + (iter - 1) * tstride;
        }
        if (infeasible) {
            status = LPR_INFEASIBLE_BASIS;
            if (post == nullptr) break;  // traced: the C# wrote that snapshot before :91 throws
        }
        // ---- :93  y = c_B B^-1 (MultiplyVectorMatrix :412-424): lane j down column j ----
        for (int j = lane; j < m; j += NT) {
            double s = 0.0;
            for (int i = 0; i < m; ++i) s += cB[i] * Binv[(size_t)i * ldb + j];
            y[j] = s;
        }
        group_sync<NT, kFenceWave>();
        if constexpr (kTrace) {
            if (post != nullptr) {  // :217-218, :245-246; the staged candidates are not live here
                rev_batch_scatter_x<NT>(stage, n, m, bas, xB, lane);
                for (int i = lane; i < m; i += NT) {
                    post[rev_trace_xb(m, n) + i] = xB[i];
                    post[rev_trace_y(m, n) + i] = y[i];
                }
                if (lane == 0) {
                    double zw = 0.0;
                    for (int i = 0; i < m; ++i) zw += cB[i] * xB[i];
                    post[kRevTraceZWorking] = zw;
                    post[kRevTraceZOriginal] = rev_batch_z_original(c, stage, n, d->is_min != 0);
                }
                group_sync<NT, kFenceWave>();  // stage is free for the candidates
            }
        }
        // ---- :96-102  rc_j = c_j - Dot(y, A_j), rcS_k = -y_k; staged for the fold ----
        for (int j = lane; j < n; j += NT) {
            const double rc = rev_batch_rc(y, A, lda, m, c[j], j);
            stage[j] = rev_enter_value(rc, isb[j] != 0);
            if constexpr (kTrace) {
                if (post != nullptr) post[rev_trace_rcx(m, n) + j] = rc;
            }
        }
        for (int i = lane; i < m; i += NT) {
            stage[n + i] = rev_enter_value(-y[i], isb[n + i] != 0);
            if constexpr (kTrace) {
                if (post != nullptr) post[rev_trace_rcs(m, n) + i] = -y[i];
            }
        }
        group_sync<NT, kFenceWave>();
        if constexpr (kTrace) {
            if (infeasible) break;
        }
        // ---- :105-146  entering variable; none: optimal ----
        const int e = rev_batch_enter<NT>(stage, N, lane, &s_slot);
        if (e < 0) {
            status = LPR_OK_OPTIMAL;
            break;
        }
        if (max_iter > 0 && iter >= max_iter) {
            status = LPR_PIVOT_LIMIT;
            break;
        }
        // ---- :149-151  u = B^-1 a_e, or column e - n of B^-1 for a slack ----
        if (e < n) {
            for (int i = lane; i < m; i += NT) prow[i] = A[(size_t)i * lda + e];
            group_sync<NT, kFenceWave>();
            rev_batch_rowmv<NT, kLds>(Binv, ldb, m, prow, u, tile, lane);
        } else {
            for (int i = lane; i < m; i += NT) u[i] = Binv[(size_t)i * ldb + (e - n)];
        }
        group_sync<NT, kFenceWave>();
        // ---- :154-179  ratio test ----
        for (int i = lane; i < m; i += NT) {
            const double ui = u[i];
            y[i] = (ui > kRevEps) ? ieee_div(xB[i], ui) : (double)NAN;
        }
        group_sync<NT, kFenceWave>();
        const int r = rev_batch_ratio<NT>(y, bas, m, lane, &s_slot);
        if (r < 0) {
            status = LPR_UNBOUNDED;
            break;
        }
        const int leaving = bas[r];
        if (leaving == e) {  // :182-183
            status = LPR_ENTERING_ALREADY_BASIC;
            break;
        }
        const double pivot = u[r];
        const double ce = (e < n) ? c[e] : 0.0;
        if constexpr (kTrace) {
            // :186-192, the pre-pivot part, while u, the ratios and the old basis are live; a
            // pivot that :267 refuses makes no record
            if (iter < tr.cap && !(fabs(pivot) < kRevEps)) {
                double* const rec = trec + iter * tstride;
                for (int i = lane; i < m; i += NT) {
                    const double ui = u[i];
                    rec[rev_trace_u(m, n) + i] = ui;
                    rec[rev_trace_ratios(m, n) + i] = (ui > kRevEps) ? y[i] : (double)INFINITY;
                    rec[rev_trace_basis_pre(m, n) + i] = (double)bas[i];
                }
                if (lane == 0) {
                    rec[kRevTraceEnter] = (double)e;
                    rec[kRevTraceRow] = (double)r;
                    rec[kRevTraceLeave] = (double)leaving;
                    rec[kRevTraceRcPre] = -stage[e];  // the staged value is -rc
                }
            }
        }
        group_sync<NT, kFenceWave>();  // every lane has read bas[r] and u[r]
        // ---- :194-212  bookkeeping ----
        if (lane == 0) {
            if (iter < log_cap) {
                lg[3 * iter] = r;
                lg[3 * iter + 1] = e;
                lg[3 * iter + 2] = leaving;
            }
            bas[r] = e;
            isb[e] = 1;
            isb[leaving] = 0;
            cB[r] = ce;
        }
        if (fabs(pivot) < kRevEps) {  // :267, after the bookkeeping; the iteration is not counted
            group_sync<NT, kFenceWave>();
            status = LPR_PIVOT_TOO_SMALL;
            break;
        }
        // ---- :264-275  UpdateBInverse = MultiplyMatrices(E, B^-1) ----
        for (int i = lane; i < m; i += NT) {
            u[i] = (i == r) ? ieee_div(1.0, pivot) : ieee_div(-u[i], pivot);  // :272
            prow[i] = Binv[(size_t)r * ldb + i];  // the old pivot row
        }
        group_sync<NT, kFenceWave>();
        // R[i,j] starts at +0.0 and adds the terms of the non-skipped k in ascending order:
        //     i <  r : (0.0 + 1.0*B[i,j]) + fac_i*B[r,j]     (second term skipped if |fac_i| < EPS)
        //     i >  r : (0.0 + fac_i*B[r,j]) + 1.0*B[i,j]     (first term skipped if |fac_i| < EPS)
        //     i == r :  0.0 + fac_r*B[r,j]                   (0.0 if |fac_r| < EPS)
        for_each_ij<NT>(m, m, lane, [&](int, int i, int j) {
            double* at = Binv + (size_t)i * ldb + j;
            const double x = *at;
            const double f = u[i];
            const bool use = !(fabs(f) < kRevEps);
            const double px = f * prow[j];
            double o;
            if (i == r) {
                o = use ? 0.0 + px : 0.0;
            } else if (i < r) {
                const double t = 0.0 + x;  // 1.0 * B[i,j] is exact
                o = use ? t + px : t;
            } else {
                const double t = use ? 0.0 + px : 0.0;
                o = t + x;
            }
            *at = o;
        });
        ++iter;  // :249
        group_sync<NT, kFenceWave>();
        if constexpr (kTrace) {
            if (iter - 1 < tr.cap)
                rev_trace_tables<NT>(trec + (iter - 1) * tstride, m, n, bas, Binv, ldb, A, lda,
                                     lane);
        }
    }

    // ---- ExtractSolution :277-287 on the optimal exit: x, then FinalZ = Dot(cOrig, x) ----
    if (status == LPR_OK_OPTIMAL) {
        rev_batch_scatter_x<NT>(stage, n, m, bas, xB, lane);
        double* const xg = xs + d->x_off;
        for (int j = lane; j < n; j += NT) xg[j] = stage[j];
        double z = 0.0;
        if (lane == 0) {
            z = rev_batch_z_original(c, stage, n, d->is_min != 0);
            d->z = z;
        }
        if constexpr (kTrace) {
            // :124-146, the "Optimal" record: no pivot (-1, rc 0, u = +0, ratios = +inf, the
            // basis twice), y and x_B of this pass, rc from the unstaged expression
            if (iter < tr.cap) {
                double* const rec = trec + iter * tstride;
                for (int j = lane; j < n; j += NT)
                    rec[rev_trace_rcx(m, n) + j] = rev_batch_rc(y, A, lda, m, c[j], j);
                for (int i = lane; i < m; i += NT) {
                    rec[rev_trace_y(m, n) + i] = y[i];
                    rec[rev_trace_rcs(m, n) + i] = -y[i];
                    rec[rev_trace_u(m, n) + i] = 0.0;
                    rec[rev_trace_ratios(m, n) + i] = (double)INFINITY;
                    rec[rev_trace_basis_pre(m, n) + i] = (double)bas[i];
                    rec[rev_trace_xb(m, n) + i] = xB[i];
                }
                if (lane == 0) {
                    rec[kRevTraceEnter] = -1.0;
                    rec[kRevTraceRow] = -1.0;
                    rec[kRevTraceLeave] = -1.0;
                    rec[kRevTraceRcPre] = 0.0;
                    double zw = 0.0;
                    for (int i = 0; i < m; ++i) zw += cB[i] * xB[i];
                    rec[kRevTraceZWorking] = zw;
                    rec[kRevTraceZOriginal] = z;
                }
                rev_trace_tables<NT>(rec, m, n, bas, Binv, ldb, A, lda, lane);
            }
        }
    }
    // ---- what the next launch and the reads need goes back to global memory ----
    if constexpr (kLds) {
        for_each_ij<NT>(m, m, lane, [&](int x, int i, int j) { Bg[x] = Binv[i * ldb + j]; });
    }
    for (int i = lane; i < m; i += NT) {
        cBg[i] = cB[i];
        xBg[i] = xB[i];
        bas_g[i] = bas[i];
    }
    if (lane == 0) {
        d->status = status;
        d->iter = iter;
        d->log_fill = (int32_t)(iter < log_cap ? iter : log_cap);
        if (status == kRunning) idx_out[atomicAdd(n_out, 1)] = k;
    }
}

// The dynamic LDS of one form's launch of either kernel of this text.  slot_doubles: W and G, the
// LDS share of one LP; H, the vectors of the largest LP (the tile follows them).
inline size_t rev_batch_lds(int form, int slot_doubles) {
    const size_t slot = (size_t)slot_doubles * sizeof(double);
    return form == kFormW ? 4 * slot
                          : (form == kFormG ? slot : slot + kRevBatchTile * sizeof(double));
}

}  // namespace lpr
