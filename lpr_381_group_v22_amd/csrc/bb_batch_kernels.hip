// bb_batch_kernels.hip -- the batched Branch & Bound: many independent integer
// programs per launch, each running the whole ExecuteBranchAndBound (IntegerProgramming/
// BranchBoundSimplexSolver.cs:1006-1233) on the device with the rules of oracle/oracle_bb.c, the
// same bits as lpr_bb_run and the oracle give for that IP alone.
//
//   k_bb_batch<NT, kLds>  at most `chunk` pops of the DFS per IP per launch; NT lanes per IP (64:
//                         form W, 256: forms G and H), the child LP's working pair in LDS (W, G)
//                         or in the global work slab (H); the DFS stack in HBM
//                         (the search text is bb_batch_body.hpp, shared with the narrated
//                         twins of bb_batch_narr_kernels.hip)
//   k_bb_batch_load       the roots into their own stack slots (lpr_bb_batch_create / _from_batch)
//   k_bb_batch_reset      RoundAllTableaux of the root (:1021), record 0, an empty incumbent
#include "bb_batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

// One IP per NT lanes; 256 / NT IPs per workgroup.  idx_in lists the IPs still running; an IP that
// is still running when its chunk is used up appends itself to idx_out (n_out counts them: the one
// word the host reads per launch).  The search itself is bb_batch_body (bb_batch_body.hpp).
template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_bb_batch(BBBatchBufs B,
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
    if (q >= n_in) return;  // uniform per IP (and per workgroup where NT == 256)
    bb_batch_body<NT, kLds, false>(B, BBNarr{}, idx_in[q], sub, lane, idx_out, n_out, chunk, slot,
                                   smem, red_v, red_i);
}

template __global__ void k_bb_batch<kWave, true>(BBBatchBufs, const int32_t*, int, int32_t*,
                                                 int32_t*, int, int);
template __global__ void k_bb_batch<256, true>(BBBatchBufs, const int32_t*, int, int32_t*,
                                               int32_t*, int, int);
template __global__ void k_bb_batch<256, false>(BBBatchBufs, const int32_t*, int, int32_t*,
                                                int32_t*, int, int);

// ------------------------------------------------------------------------------------------
// The root of every IP (packed at src + src_off[k], rows x cols) into its own stack slot,
// node_cap + 1.  One wave per IP.
__global__ __launch_bounds__(256) void k_bb_batch_load(const BBBatchDesc* __restrict__ desc,
                                                       int count, const double* __restrict__ src,
                                                       const int64_t* __restrict__ src_off,
                                                       double* __restrict__ stack) {
    const int k = blockIdx.x * 4 + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (k >= count) return;
    const BBBatchDesc& d = desc[k];
    double* const root = stack + d.stack_off + (int64_t)(d.node_cap + 1) * d.slot_n();
    const double* const s = src + src_off[k];
    for (int x = lane; x < d.rows * d.cols; x += kWave) root[x] = s[x];
}

// The start of ExecuteBranchAndBound (:1016-1030) for every IP: RoundAllTableaux of the root
// (:1021) into stack slot 0, record 0, optimalValue = -inf, x = 0, nothing popped.
__global__ __launch_bounds__(256) void k_bb_batch_reset(BBBatchBufs B, int count) {
    const int k = blockIdx.x * 4 + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (k >= count) return;
    BBBatchDesc* const d = B.desc + k;
    const int R = d->rows, C = d->cols;
    double* const stack = B.stack + d->stack_off;
    const double* const root = stack + (int64_t)(d->node_cap + 1) * d->slot_n();
    for (int x = lane; x < R * C; x += kWave) stack[x] = dn_round4(root[x]);
    for (int i = lane; i < d->nvars; i += kWave) B.x[d->x_off + i] = 0.0;
    if (lane == 0) {
        int32_t* const e = B.rec_i + (int64_t)kBBRecInts * d->rec_off;
        e[0] = -1;
        e[1] = 0;
        e[2] = 0;
        e[3] = -1;
        e[4] = 0;
        B.rec_d[2 * d->rec_off] = 0.0;
        B.rec_d[2 * d->rec_off + 1] = dn_round4(dn_round4(root[C - 1]));
        B.stk[d->stk_off] = 0;
        B.stk[d->stk_off + 1] = 0;
        d->sp = 1;
        d->iteration = 0;
        d->nrec = 1;
        d->found = 0;
        d->best_node = -1;
        d->processed = 0;
        d->best_z = -INFINITY;
        d->pivots = 0;
        d->status = kRunning;
    }
}

// ------------------------------------------------------------------------------------------
// Launchers (bb_batch_engine.hip).
int bb_batch_launch(int form, hipStream_t s, const BBBatchBufs& B, const int32_t* idx_in,
                    int n_in, int32_t* idx_out, int32_t* n_out, int chunk, int slot_doubles,
                    int max_rows) {
    const char* const name = "k_bb_batch";
    const size_t slot = (size_t)slot_doubles * sizeof(double);
    if (form == kFormW)
        return batch_launch<&k_bb_batch<kWave, true>>(name, "IPs", form, s, n_in, 4 * slot,
                                                      kBatchMaxLdsG, B, idx_in, n_in, idx_out,
                                                      n_out, chunk, slot_doubles);
    if (form == kFormG)
        return batch_launch<&k_bb_batch<256, true>>(name, "IPs", form, s, n_in, slot,
                                                    kBatchMaxLdsG, B, idx_in, n_in, idx_out, n_out,
                                                    chunk, slot_doubles);
    return batch_launch<&k_bb_batch<256, false>>(name, "IPs", form, s, n_in,
                                                 (size_t)max_rows * sizeof(double), kBatchMaxLdsG,
                                                 B, idx_in, n_in, idx_out, n_out, chunk, 0);
}

void bb_batch_launch_load(hipStream_t s, const BBBatchDesc* desc, int count, const double* src,
                          const int64_t* src_off, double* stack) {
    hipLaunchKernelGGL(k_bb_batch_load, dim3((count + 3) / 4), dim3(256), 0, s, desc, count, src,
                       src_off, stack);
}

void bb_batch_launch_reset(hipStream_t s, const BBBatchBufs& B, int count) {
    hipLaunchKernelGGL(k_bb_batch_reset, dim3((count + 3) / 4), dim3(256), 0, s, B, count);
}

}  // namespace lpr
