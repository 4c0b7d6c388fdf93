// batch_kernels.hip -- the batched primal simplex: many independent LPs per
// launch, each solved with the rules of PrimalSimplexSolver (Simplex/PrimalSimplexSolver.cs), the
// same bits as lpr_primal_solve and the oracle give for that LP alone.
//
//   k_batch_simplex<NT, kLds>  the loop of Solve() (:102-150), at most `chunk` pivots per LP per
//                              launch; NT lanes per LP (64: form W, 256: forms G and H), the
//                              tableau in LDS (W, G) or in the global slab (H); the loop itself
//                              is batch_body.hpp, which batch_trace_kernels.hip instantiates
//                              with its trace steps for a traced handle
//   k_batch_build             the constructor (:27-87) for every LP of lpr_batch_from_lps
//   k_batch_extract            FinalZ (:113) and ExtractSolution() (:213-252) for every LP
#include "batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

// The loop of batch_body.hpp without its trace steps.
template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_batch_simplex(BatchDesc* __restrict__ desc,
                                                       double* __restrict__ slab,
                                                       int32_t* __restrict__ basis,
                                                       int32_t* __restrict__ logs,
                                                       const int32_t* __restrict__ idx_in, int n_in,
                                                       int32_t* __restrict__ idx_out,
                                                       int32_t* __restrict__ n_out, int chunk,
                                                       int slot) {
    batch_simplex_run<NT, kLds, false>(desc, slab, basis, logs, idx_in, n_in, idx_out, n_out,
                                       chunk, slot, BatchTrace{nullptr, nullptr, 0});
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
// Launchers (batch_engine.hip).  slot_doubles: W and G, the LDS share of one LP, which is also the
// kernel's last argument; max_rows, max_cols: H, the factor column and pivot row of the largest LP.
int batch_launch_simplex(int form, hipStream_t s, BatchDesc* desc, double* slab, int32_t* basis,
                         int32_t* logs, const int32_t* idx_in, int n_in, int32_t* idx_out,
                         int32_t* n_out, int chunk, int slot_doubles, int max_rows,
                         int max_cols) {
    const char* const name = "k_batch_simplex";
    const size_t slot = (size_t)slot_doubles * sizeof(double);
    if (form == kFormW)
        return batch_launch<&k_batch_simplex<kWave, true>>(
            name, "LPs", form, s, n_in, 4 * slot, kBatchMaxLdsG, desc, slab, basis, logs, idx_in,
            n_in, idx_out, n_out, chunk, slot_doubles);
    if (form == kFormG)
        return batch_launch<&k_batch_simplex<256, true>>(
            name, "LPs", form, s, n_in, slot, kBatchMaxLdsG, desc, slab, basis, logs, idx_in, n_in,
            idx_out, n_out, chunk, slot_doubles);
    return batch_launch<&k_batch_simplex<256, false>>(
        name, "LPs", form, s, n_in, (size_t)(max_rows + max_cols) * sizeof(double), kBatchMaxLdsG,
        desc, slab, basis, logs, idx_in, n_in, idx_out, n_out, chunk, 0);
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
