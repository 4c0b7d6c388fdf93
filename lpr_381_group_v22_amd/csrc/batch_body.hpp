// batch_body.hpp -- the loop of PrimalSimplexSolver.Solve() (Simplex/PrimalSimplexSolver.cs
// :102-150) for one LP of a batch, as one function template: batch_simplex_run<NT, kLds, kTrace>.
// batch_kernels.hip instantiates it without the trace steps (k_batch_simplex, DESIGN.md section
// 12), batch_trace_kernels.hip with them (k_batch_simplex_trace, section 22).  The trace steps sit
// under `if constexpr (kTrace)`; with kTrace false nothing of them is compiled.
#pragma once

#include "batch_common.hpp"
#include "batch_device.hpp"

#pragma clang fp contract(off)

namespace lpr {

// One LP per NT lanes; 256 / NT LPs per workgroup.  Everything the lanes of an LP share during a
// launch is in LDS (W, G) or ordered by workgroup barriers (H), so form W fences at wave scope.
// idx_in lists the LPs still running; an LP that is still running when its chunk is used up
// appends itself to idx_out (n_out counts them: the one word the host reads per launch).
//
// kTrace (section 22): the pass that makes pivot number iter + 1 also stores the tableau after it
// to record iter + 1 of the LP (batch_trace_* of batch_common.hpp) while that record index is
// below tr.cap: the lane that computes an element stores it twice, an element of the pivot row
// comes from prow, lane 0 writes the header.  Records are addressed by the LP's absolute iter, so
// a chunk boundary, a limit and a resumed call just continue; the exits that make no pivot write
// nothing.  No lane reads a record, so the trace adds no fence, no barrier and no LDS.
template <int NT, bool kLds, bool kTrace>
__device__ __forceinline__ void batch_simplex_run(BatchDesc* __restrict__ desc,
                                                  double* __restrict__ slab,
                                                  int32_t* __restrict__ basis,
                                                  int32_t* __restrict__ logs,
                                                  const int32_t* __restrict__ idx_in, int n_in,
                                                  int32_t* __restrict__ idx_out,
                                                  int32_t* __restrict__ n_out, int chunk,
                                                  int slot, const BatchTrace tr) {
    extern __shared__ double smem[];
    __shared__ double red_v[kWave];
    __shared__ int red_i[kWave];
    constexpr int kPerWg = 256 / NT;
    const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / NT);
    const int lane = (int)threadIdx.x % NT;
    const int q = blockIdx.x * kPerWg + sub;
    if (q >= n_in) return;  // uniform per LP (and per workgroup where NT == 256)
    const int k = idx_in[q];
    BatchDesc* d = desc + k;
    const int R = d->rows, C = d->cols;
    const int RC = R * C;
    int64_t iter = d->iter;
    const int64_t max_iter = d->max_iter;
    const int log_cap = d->log_cap;
    int32_t* bas = basis + d->b_off;
    int32_t* lg = logs + 2 * d->log_off;
    double* const Tg = slab + d->t_off;
    // the LP's records: record i at trec + i * tstride, kept while i < tr.cap
    double* trec = nullptr;
    int64_t tstride = 0;
    if constexpr (kTrace) {
        trec = tr.slab + tr.off[k];
        tstride = batch_trace_stride(R, C);
    }

    double* T;      // the tableau this launch works on
    double* fcol;   // factor column, staged before any row is updated
    double* prow = nullptr;  // normalised pivot row (H: a copy in LDS; W, G: row r of T)
    if constexpr (kLds) {
        T = smem + (size_t)sub * slot;
        fcol = T + RC;
        for (int x = lane; x < RC; x += NT) T[x] = Tg[x];
        group_sync<NT, kFenceWave>();
    } else {
        T = Tg;
        fcol = smem;
        prow = smem + R;
    }

    int32_t status = kRunning;
    for (int p = 0; p < chunk; ++p) {
        // ---- FindEnteringVariable  :152-167: strict < against a running minimum from 0 ----
        Cand c;
        c.v = 0.0;
        c.i = -1;
        for (int j = lane; j < C - 1; j += NT) {
            const double v = T[j];
            if (v < c.v) {  // -0.0 and NaN never enter
                c.v = v;
                c.i = j;
            }
        }
        c = group_cand_min<NT>(c, red_v, red_i);
        const int e = c.i;
        if (e < 0) {
            status = LPR_OK_OPTIMAL;
            break;
        }
        // ---- FindLeavingVariable  :169-191: a > 1e-9, 0 <= ratio < double.MaxValue ----
        Cand l;
        l.v = DBL_MAX;
        l.i = -1;
        for (int i = 1 + lane; i < R; i += NT) {
            const double a = T[(size_t)i * C + e];
            if (a > 1e-9) {
                const double ratio = ieee_div(T[(size_t)i * C + (C - 1)], a);
                if (ratio >= 0 && ratio < DBL_MAX && (l.i < 0 || ratio < l.v)) {
                    l.v = ratio;
                    l.i = i;
                }
            }
        }
        l = group_cand_min<NT>(l, red_v, red_i);
        const int r = l.i;
        if (r < 0) {
            status = LPR_UNBOUNDED;
            break;
        }
        if (max_iter > 0 && iter >= max_iter) {
            status = LPR_PIVOT_LIMIT;
            break;
        }
        // ---- Pivot  :193-211 ----
        for (int i = lane; i < R; i += NT) fcol[i] = T[(size_t)i * C + e];
        group_sync<NT, kFenceWave>();
        const double pe = fcol[r];
        double* const Tr = T + (size_t)r * C;
        for (int j = lane; j < C; j += NT) {  // :198-199, every column, RHS included
            const double v = ieee_div(Tr[j], pe);
            Tr[j] = v;
            if constexpr (!kLds) prow[j] = v;
        }
        if constexpr (kLds) prow = Tr;
        group_sync<NT, kFenceWave>();
        // the tableau of the record this pivot makes, or null once the cap is reached
        double* rtab = nullptr;
        if constexpr (kTrace) {
            if (iter + 1 < (int64_t)tr.cap) rtab = trec + (iter + 1) * tstride + batch_trace_tab();
        }
        // :201-210: every row but r, the Z row included, and no row skipped for a zero factor
        // (+0 * a negative p_j is -0.0, and -0.0 - -0.0 is +0.0; 0 * inf is NaN).  Element-
        // parallel over the flattened tableau, four elements in flight per lane.
        {
            constexpr int U = 4;
            const int di = NT / C, dj = NT - (NT / C) * C;
            int i = lane / C, j = lane - (lane / C) * C;
            for (int base = 0; base < RC; base += U * NT) {
                double v[U];
                int ii[U], jj[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int x = base + u * NT + lane;
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
                    const int x = base + u * NT + lane;
                    if constexpr (!kTrace) {
                        if (x < RC && ii[u] != r) {
                            const double prod = fcol[ii[u]] * prow[jj[u]];  // rounded: no FMA
                            T[x] = v[u] - prod;
                        }
                    } else if (x < RC) {
                        double nv = prow[jj[u]];  // the pivot row, which the pass leaves as it is
                        if (ii[u] != r) {
                            const double prod = fcol[ii[u]] * prow[jj[u]];  // rounded: no FMA
                            nv = v[u] - prod;
                            T[x] = nv;
                        }
                        if (rtab) rtab[x] = nv;
                    }
                }
            }
        }
        if (lane == 0) {
            bas[r - 1] = e;  // :142
            if (iter < log_cap) {
                lg[2 * iter] = r;  // 1-based, :138
                lg[2 * iter + 1] = e;
            }
            if constexpr (kTrace) {
                if (rtab) {
                    double* const rec = rtab - batch_trace_tab();
                    rec[batch_trace_row()] = (double)r;
                    rec[batch_trace_col()] = (double)e;
                }
            }
        }
        ++iter;
        group_sync<NT, kFenceWave>();
    }

    if constexpr (kLds) {  // the LDS copy goes back to the slab
        for (int x = lane; x < RC; x += NT) Tg[x] = T[x];
    }
    if (lane == 0) {
        d->status = status;
        d->iter = iter;
        d->log_fill = (int32_t)(iter < log_cap ? iter : log_cap);
        if (status == kRunning) idx_out[atomicAdd(n_out, 1)] = k;
    }
}

}  // namespace lpr
