// batch_kernels.hip -- the batched primal simplex: many independent LPs per
// launch, each solved with the rules of PrimalSimplexSolver (Simplex/PrimalSimplexSolver.cs), the
// same bits as lpr_primal_solve and the oracle give for that LP alone.
//
//   k_batch_simplex<NT, kLds>  the loop of Solve() (:102-150), at most `chunk` pivots per LP per
//                              launch; NT lanes per LP (64: form W, 256: forms G and H), the
//                              tableau in LDS (W, G) or in the global slab (H)
//   k_batch_build              the constructor (:27-87) for every LP of lpr_batch_from_lps
//   k_batch_extract            FinalZ (:113) and ExtractSolution() (:213-252) for every LP
#include "batch_common.hpp"
#include "batch_device.hpp"

#pragma clang fp contract(off)

namespace lpr {

// One LP per NT lanes; 256 / NT LPs per workgroup.  Everything the lanes of an LP share during a
// launch is in LDS (W, G) or ordered by workgroup barriers (H), so form W fences at wave scope.
// idx_in lists the LPs still running; an LP that is still running when its chunk is used up
// appends itself to idx_out (n_out counts them: the one word the host reads per launch).
template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_batch_simplex(BatchDesc* __restrict__ desc,
                                                       double* __restrict__ slab,
                                                       int32_t* __restrict__ basis,
                                                       int32_t* __restrict__ logs,
                                                       const int32_t* __restrict__ idx_in, int n_in,
                                                       int32_t* __restrict__ idx_out,
                                                       int32_t* __restrict__ n_out, int chunk,
                                                       int slot) {
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
                    if (x < RC && ii[u] != r) {
                        const double prod = fcol[ii[u]] * prow[jj[u]];  // rounded: no FMA
                        T[x] = v[u] - prod;
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

template __global__ void k_batch_simplex<kWave, true>(BatchDesc*, double*, int32_t*, int32_t*,
                                                      const int32_t*, int, int32_t*, int32_t*,
                                                      int, int);
template __global__ void k_batch_simplex<256, true>(BatchDesc*, double*, int32_t*, int32_t*,
                                                    const int32_t*, int, int32_t*, int32_t*, int,
                                                    int);
template __global__ void k_batch_simplex<256, false>(BatchDesc*, double*, int32_t*, int32_t*,
                                                     const int32_t*, int, int32_t*, int32_t*, int,
                                                     int);

// ------------------------------------------------------------------------------------------
// Constructor  PrimalSimplexSolver.cs:27-87, one wave per LP, every element of the tableau
// written (the slab is not zero-filled first).  Same bytes as k_build_rows / k_build_obj.
__global__ __launch_bounds__(256) void k_batch_build(const BatchDesc* __restrict__ desc,
                                                     const BatchBuild* __restrict__ bd, int count,
                                                     double* __restrict__ slab,
                                                     int32_t* __restrict__ basis,
                                                     const double* __restrict__ obj,
                                                     const double* __restrict__ A,
                                                     const int32_t* __restrict__ ncoef,
                                                     const int8_t* __restrict__ rel,
                                                     const double* __restrict__ rhs,
                                                     const int8_t* __restrict__ is_max) {
    const int k = blockIdx.x * 4 + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (k >= count) return;
    const BatchDesc& d = desc[k];
    const BatchBuild& b = bd[k];
    const int R = d.rows, C = d.cols, m = R - 1, n = d.n;
    double* T = slab + d.t_off;
    const bool mx = is_max[k] != 0;
    for (int x = lane; x < R * C; x += kWave) {
        const int i = x / C, j = x - (x / C) * C;
        double v = 0.0;
        if (i == 0) {
            if (j < n) v = mx ? -obj[b.obj_off + j] : obj[b.obj_off + j];  // :61-62
        } else {
            const int ci = i - 1;
            const bool ge = rel[b.row_off + ci] == LPR_REL_GE;  // :36-41
            const int cnt = ncoef ? ncoef[b.row_off + ci] : n;
            if (j < n) {
                if (j < cnt) {  // :68-72
                    const double a = A[b.a_off + (int64_t)ci * n + j];
                    v = ge ? -a : a;
                }
            } else if (j == n + ci) {
                v = 1.0;  // :75-76
            } else if (j == C - 1) {
                const double h = rhs[b.row_off + ci];
                v = ge ? -h : h;  // :82
            }
        }
        T[x] = v;
    }
    for (int i = lane; i < m; i += kWave) basis[d.b_off + i] = n + i;  // :78
}

// FinalZ = T[0, C-1] for every LP (z may be null); x (may be null) by ExtractSolution() for the
// optimal ones, 0 for the others.  One wave per LP, one lane per decision column.
__global__ __launch_bounds__(256) void k_batch_extract(const BatchDesc* __restrict__ desc,
                                                       int count, const double* __restrict__ slab,
                                                       double* __restrict__ x,
                                                       double* __restrict__ z) {
    const int k = blockIdx.x * 4 + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (k >= count) return;
    const BatchDesc& d = desc[k];
    const int R = d.rows, C = d.cols;
    const double* T = slab + d.t_off;
    if (z && lane == 0) z[k] = T[C - 1];
    if (!x) return;
    const bool opt = d.status == LPR_OK_OPTIMAL;
    for (int j = lane; j < d.n; j += kWave) {
        x[d.x_off + j] = opt ? extract_solution(T, C, R, C, j) : 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// Launchers (batch_engine.hip).
int batch_launch_simplex(int form, hipStream_t s, BatchDesc* desc, double* slab, int32_t* basis,
                         int32_t* logs, const int32_t* idx_in, int n_in, int32_t* idx_out,
                         int32_t* n_out, int chunk, int slot_doubles, int max_rows,
                         int max_cols) {
    static unsigned long long g_mask = 0;  // per device bit: the G attribute is set
    if (n_in <= 0) return LPR_OK_OPTIMAL;
    if (form == kFormW) {
        const size_t lds = (size_t)4 * slot_doubles * sizeof(double);
        hipLaunchKernelGGL((k_batch_simplex<kWave, true>), dim3((n_in + 3) / 4), dim3(256), lds,
                           s, desc, slab, basis, logs, idx_in, n_in, idx_out, n_out, chunk,
                           slot_doubles);
    } else if (form == kFormG) {
        const size_t lds = (size_t)slot_doubles * sizeof(double);
        if (lds > ((size_t)64 << 10)) {
            const int rc = raise_dynamic_lds(
                reinterpret_cast<const void*>(&k_batch_simplex<256, true>), kBatchMaxLdsG, &g_mask);
            if (rc != LPR_OK_OPTIMAL) return rc;
        }
        hipLaunchKernelGGL((k_batch_simplex<256, true>), dim3(n_in), dim3(256), lds, s, desc,
                           slab, basis, logs, idx_in, n_in, idx_out, n_out, chunk, slot_doubles);
    } else {
        const size_t lds = (size_t)(max_rows + max_cols) * sizeof(double);
        hipLaunchKernelGGL((k_batch_simplex<256, false>), dim3(n_in), dim3(256), lds, s, desc,
                           slab, basis, logs, idx_in, n_in, idx_out, n_out, chunk, 0);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        set_error("k_batch_simplex (form %d, %d LPs) failed to launch: %s", form, n_in,
                  hipGetErrorString(err));
        return LPR_DEVICE_ERROR;
    }
    return LPR_OK_OPTIMAL;
}

void batch_launch_build(hipStream_t s, const BatchDesc* desc, const BatchBuild* bd, int count,
                        double* slab, int32_t* basis, const double* obj, const double* A,
                        const int32_t* ncoef, const int8_t* rel, const double* rhs,
                        const int8_t* is_max) {
    hipLaunchKernelGGL(k_batch_build, dim3((count + 3) / 4), dim3(256), 0, s, desc, bd, count,
                       slab, basis, obj, A, ncoef, rel, rhs, is_max);
}

void batch_launch_extract(hipStream_t s, const BatchDesc* desc, int count, const double* slab,
                          double* x, double* z) {
    hipLaunchKernelGGL(k_batch_extract, dim3((count + 3) / 4), dim3(256), 0, s, desc, count, slab,
                       x, z);
}

}  // namespace lpr
