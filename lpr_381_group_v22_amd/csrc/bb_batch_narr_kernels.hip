// bb_batch_narr_kernels.hip -- the narrated twins of k_bb_batch: the same
// search text (bb_batch_body.hpp) with kNarr = true, which also writes what the console text of
// ExecuteBranchAndBound (IntegerProgramming/BranchBoundSimplexSolver.cs:1006-1233) needs -- every
// tableau of every child's DoDualSimplex list (:292, :341, :388), the score of every pop
// (:1049-1076) and the incumbent's tableau (:935-983) -- in the layout of bb_narr_layout.hpp.  A
// handle made narrated by lpr_bb_batch_narrate_reserve launches these instead of k_bb_batch, in
// the form batch_pick_form gives the IP un-narrated and with the same dynamic LDS.
//
//   k_bb_batch_narr<NT, kLds>  forms W (64, LDS), G (256, LDS), H (256, work slab)
//   k_bb_batch_narr_reset      rewinds every IP's cursors; every run starts from the roots
#include "bb_batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_bb_batch_narr(BBBatchBufs B, BBNarr narr,
                                                       const int32_t* __restrict__ idx_in,
                                                       int n_in, int32_t* __restrict__ idx_out,
                                                       int32_t* __restrict__ n_out, int chunk,
                                                       int slot) {
    extern __shared__ double smem[];
    __shared__ double red_v[kWave];
    __shared__ int red_i[kWave];
    constexpr int kPerWg = 256 / NT;
    const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / NT);
    const int lane = (int)threadIdx.x % NT;
    const int q = blockIdx.x * kPerWg + sub;
    if (q >= n_in) return;  // uniform per IP (and per workgroup where NT == 256)
    bb_batch_body<NT, kLds, true>(B, narr, idx_in[q], sub, lane, idx_out, n_out, chunk, slot, smem,
                                  red_v, red_i);
}

template __global__ void k_bb_batch_narr<kWave, true>(BBBatchBufs, BBNarr, const int32_t*, int,
                                                      int32_t*, int32_t*, int, int);
template __global__ void k_bb_batch_narr<256, true>(BBBatchBufs, BBNarr, const int32_t*, int,
                                                    int32_t*, int32_t*, int, int);
template __global__ void k_bb_batch_narr<256, false>(BBBatchBufs, BBNarr, const int32_t*, int,
                                                     int32_t*, int32_t*, int, int);

// The cursors of every IP back to the start, and the root's record: no child tableau.
__global__ __launch_bounds__(256) void k_bb_batch_narr_reset(BBBatchBufs B, BBNarr narr,
                                                             int count) {
    const int k = blockIdx.x * 256 + (int)threadIdx.x;
    if (k >= count) return;
    narr_rewind(narr.desc[k]);
    narr.tab_off[B.desc[k].rec_off] = 0;
    narr.ntab[B.desc[k].rec_off] = 0;
}

// ------------------------------------------------------------------------------------------
// Launchers (bb_batch_engine.hip); the arguments of bb_batch_launch and the narration buffers.
int bb_batch_narr_launch(int form, hipStream_t s, const BBBatchBufs& B, const BBNarr& narr,
                         const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out,
                         int chunk, int slot_doubles, int max_rows) {
    const char* const name = "k_bb_batch_narr";
    const size_t slot = (size_t)slot_doubles * sizeof(double);
    if (form == kFormW)
        return batch_launch<&k_bb_batch_narr<kWave, true>>(name, "IPs", form, s, n_in, 4 * slot,
                                                           kBatchMaxLdsG, B, narr, idx_in, n_in,
                                                           idx_out, n_out, chunk, slot_doubles);
    if (form == kFormG)
        return batch_launch<&k_bb_batch_narr<256, true>>(name, "IPs", form, s, n_in, slot,
                                                         kBatchMaxLdsG, B, narr, idx_in, n_in,
                                                         idx_out, n_out, chunk, slot_doubles);
    return batch_launch<&k_bb_batch_narr<256, false>>(
        name, "IPs", form, s, n_in, (size_t)max_rows * sizeof(double), kBatchMaxLdsG, B, narr,
        idx_in, n_in, idx_out, n_out, chunk, 0);
}

void bb_batch_narr_launch_reset(hipStream_t s, const BBBatchBufs& B, const BBNarr& narr,
                                int count) {
    hipLaunchKernelGGL(k_bb_batch_narr_reset, dim3((count + 255) / 256), dim3(256), 0, s, B, narr,
                       count);
}

}  // namespace lpr
