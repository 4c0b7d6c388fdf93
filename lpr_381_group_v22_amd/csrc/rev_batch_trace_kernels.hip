// rev_batch_trace_kernels.hip -- the traced form of the batched revised primal simplex (DESIGN.md
// section 21): the loop of rev_batch_body.hpp with its trace steps, which also writes, per LP,
// every snapshot RevisedPrimalSimplexSolver.CaptureSnapshot (:294-387) would have appended, as
// numbers (the record of rev_batch_common.hpp).  A handle made traced by
// lpr_rev_batch_trace_reserve launches these instead of k_rev_batch; everything else an LP ends
// with is the same bytes.
//
//   k_rev_batch_trace<NT, kLds>  NT lanes per LP (64: form W, 256: forms G and H), B^-1 and A in
//                                LDS (W, G) or in the global slab (H); the LDS footprint is that
//                                of k_rev_batch<NT, kLds>
#include "rev_batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_rev_batch_trace(RevBatchDesc* __restrict__ desc,
                                                         double* __restrict__ slab,
                                                         int32_t* __restrict__ basis,
                                                         int32_t* __restrict__ logs,
                                                         double* __restrict__ xs,
                                                         const int32_t* __restrict__ idx_in,
                                                         int n_in, int32_t* __restrict__ idx_out,
                                                         int32_t* __restrict__ n_out, int chunk,
                                                         RevBatchTrace tr, int slot) {
    rev_batch_run<NT, kLds, true>(desc, slab, basis, logs, xs, idx_in, n_in, idx_out, n_out, chunk,
                                  slot, tr);
}

template __global__ void k_rev_batch_trace<kWave, true>(RevBatchDesc*, double*, int32_t*,
                                                        int32_t*, double*, const int32_t*, int,
                                                        int32_t*, int32_t*, int, RevBatchTrace,
                                                        int);
template __global__ void k_rev_batch_trace<256, true>(RevBatchDesc*, double*, int32_t*, int32_t*,
                                                      double*, const int32_t*, int, int32_t*,
                                                      int32_t*, int, RevBatchTrace, int);
template __global__ void k_rev_batch_trace<256, false>(RevBatchDesc*, double*, int32_t*, int32_t*,
                                                       double*, const int32_t*, int, int32_t*,
                                                       int32_t*, int, RevBatchTrace, int);

// Launcher (rev_batch_engine.hip), as rev_batch_launch.
int rev_batch_trace_launch(int form, hipStream_t s, RevBatchDesc* desc, double* slab,
                           int32_t* basis, int32_t* logs, double* xs, const int32_t* idx_in,
                           int n_in, int32_t* idx_out, int32_t* n_out, int chunk,
                           int slot_doubles, RevBatchTrace tr) {
    const char* const name = "k_rev_batch_trace";
    const size_t lds = rev_batch_lds(form, slot_doubles);
    if (form == kFormW)
        return batch_launch<&k_rev_batch_trace<kWave, true>>(
            name, "LPs", form, s, n_in, lds, kBatchMaxLdsG, desc, slab, basis, logs, xs, idx_in,
            n_in, idx_out, n_out, chunk, tr, slot_doubles);
    if (form == kFormG)
        return batch_launch<&k_rev_batch_trace<256, true>>(
            name, "LPs", form, s, n_in, lds, kBatchMaxLdsG, desc, slab, basis, logs, xs, idx_in,
            n_in, idx_out, n_out, chunk, tr, slot_doubles);
    return batch_launch<&k_rev_batch_trace<256, false>>(
        name, "LPs", form, s, n_in, lds, kBatchMaxLdsG, desc, slab, basis, logs, xs, idx_in, n_in,
        idx_out, n_out, chunk, tr, 0);
}

}  // namespace lpr
