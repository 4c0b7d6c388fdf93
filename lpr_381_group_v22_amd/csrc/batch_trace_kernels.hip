// batch_trace_kernels.hip -- the traced form of the batched primal simplex:
// the loop of batch_body.hpp with its trace steps, which also writes, per LP, the tableau after
// every pivot -- what PrimalSimplexSolver appends to IterationSnapshots as text
// (Simplex/PrimalSimplexSolver.cs:86, :148) -- as numbers (the record of batch_common.hpp).  A
// handle made traced by lpr_batch_trace_reserve launches these instead of k_batch_simplex;
// everything else an LP ends with is the same bytes.
//
//   k_batch_simplex_trace<NT, kLds>  NT lanes per LP (64: form W, 256: forms G and H), the tableau
//                                    in LDS (W, G) or in the global slab (H); the LDS footprint is
//                                    that of k_batch_simplex<NT, kLds>
//   k_batch_trace_first              record 0 of every LP: the tableau as built or uploaded (:86)
#include "batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_batch_simplex_trace(BatchDesc* __restrict__ desc,
                                                             double* __restrict__ slab,
                                                             int32_t* __restrict__ basis,
                                                             int32_t* __restrict__ logs,
                                                             const int32_t* __restrict__ idx_in,
                                                             int n_in,
                                                             int32_t* __restrict__ idx_out,
                                                             int32_t* __restrict__ n_out,
                                                             int chunk, double* __restrict__ trace,
                                                             const int64_t* __restrict__ trace_off,
                                                             int trace_cap, int slot) {
    batch_simplex_run<NT, kLds, true>(desc, slab, basis, logs, idx_in, n_in, idx_out, n_out, chunk,
                                      slot, BatchTrace{trace, trace_off, trace_cap});
}

template __global__ void k_batch_simplex_trace<kWave, true>(BatchDesc*, double*, int32_t*,
                                                            int32_t*, const int32_t*, int,
                                                            int32_t*, int32_t*, int, double*,
                                                            const int64_t*, int, int);
template __global__ void k_batch_simplex_trace<256, true>(BatchDesc*, double*, int32_t*, int32_t*,
                                                          const int32_t*, int, int32_t*, int32_t*,
                                                          int, double*, const int64_t*, int, int);
template __global__ void k_batch_simplex_trace<256, false>(BatchDesc*, double*, int32_t*,
                                                           int32_t*, const int32_t*, int,
                                                           int32_t*, int32_t*, int, double*,
                                                           const int64_t*, int, int);

// Record 0 of every LP ("Initial Tableau", :86): header -1, -1 and the tableau as it stands in the
// slab.  One wave per LP; trace_cap >= 1, so record 0 is always kept.
__global__ __launch_bounds__(256) void k_batch_trace_first(const BatchDesc* __restrict__ desc,
                                                           int count,
                                                           const double* __restrict__ slab,
                                                           double* __restrict__ trace,
                                                           const int64_t* __restrict__ trace_off) {
    const int k = blockIdx.x * 4 + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (k >= count) return;
    const BatchDesc& d = desc[k];
    const int RC = d.rows * d.cols;
    const double* T = slab + d.t_off;
    double* rec = trace + trace_off[k];
    if (lane == 0) {
        rec[batch_trace_row()] = -1.0;
        rec[batch_trace_col()] = -1.0;
    }
    double* rtab = rec + batch_trace_tab();
    for (int x = lane; x < RC; x += kWave) rtab[x] = T[x];
}

// Launchers (batch_engine.hip), as batch_launch_simplex.
int batch_trace_launch_simplex(int form, hipStream_t s, BatchDesc* desc, double* slab,
                               int32_t* basis, int32_t* logs, const int32_t* idx_in, int n_in,
                               int32_t* idx_out, int32_t* n_out, int chunk, int slot_doubles,
                               int max_rows, int max_cols, BatchTrace tr) {
    const char* const name = "k_batch_simplex_trace";
    const size_t slot = (size_t)slot_doubles * sizeof(double);
    if (form == kFormW)
        return batch_launch<&k_batch_simplex_trace<kWave, true>>(
            name, "LPs", form, s, n_in, 4 * slot, kBatchMaxLdsG, desc, slab, basis, logs, idx_in,
            n_in, idx_out, n_out, chunk, tr.slab, tr.off, tr.cap, slot_doubles);
    if (form == kFormG)
        return batch_launch<&k_batch_simplex_trace<256, true>>(
            name, "LPs", form, s, n_in, slot, kBatchMaxLdsG, desc, slab, basis, logs, idx_in, n_in,
            idx_out, n_out, chunk, tr.slab, tr.off, tr.cap, slot_doubles);
    return batch_launch<&k_batch_simplex_trace<256, false>>(
        name, "LPs", form, s, n_in, (size_t)(max_rows + max_cols) * sizeof(double), kBatchMaxLdsG,
        desc, slab, basis, logs, idx_in, n_in, idx_out, n_out, chunk, tr.slab, tr.off, tr.cap, 0);
}

void batch_trace_launch_first(hipStream_t s, const BatchDesc* desc, int count, const double* slab,
                              BatchTrace tr) {
    hipLaunchKernelGGL(k_batch_trace_first, dim3((count + 3) / 4), dim3(256), 0, s, desc, count,
                       slab, tr.slab, tr.off);
}

}  // namespace lpr
