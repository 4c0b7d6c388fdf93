// batch_device.hpp -- device helpers shared by the kernels of the three batch engines
// (batch_kernels.hip, bb_batch_kernels.hip, sens_batch_kernels.hip): the ordering and the
// candidate minimum over the NT lanes that work on one item, and the walk over a flattened
// rows x cols block.  (The two pivots that walk with four elements in flight, k_batch_simplex and
// k_sens_batch, keep that loop open-coded: through a shared helper k_sens_batch compiles to
// different code.)  The host side of what the engines share is batch_common.hpp.
#pragma once

#include "engine_common.hpp"
#include "select_common.hpp"

#pragma clang fp contract(off)

namespace lpr {

// Ordering between the NT lanes of one item.  NT == kWave (form W): one wave, no workgroup barrier
// (the four items of a workgroup never wait for each other); a wave's LDS operations complete in
// order, so where everything the lanes share is in LDS a wave-scope fence that keeps the compiler
// from moving them is enough (kFenceWave).  A kernel whose lanes also share global memory fences
// at workgroup scope (kFenceWorkgroup), which makes those writes visible to the other lanes too.
enum FenceScope : int { kFenceWave = 0, kFenceWorkgroup = 1 };

template <int NT, FenceScope kScope>
__device__ __forceinline__ void group_sync() {
    if constexpr (NT != kWave) {
        __syncthreads();
    } else if constexpr (kScope == kFenceWave) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// Lexicographic (value, index) minimum over the NT lanes of one item (no NaN candidates); every
// lane gets it.
template <int NT>
__device__ __forceinline__ Cand group_cand_min(Cand c, double* red_v, int* red_i) {
    if constexpr (NT == kWave) {
        return dpp_wave_cand_min(c);
    } else {
        return dpp_block_cand_min(c, red_v, red_i);
    }
}

// f(x, i, j) for every element x = i * cols + j of a rows x cols block, NT lanes apart; (i, j)
// advance by additions and one carry, without a division per element.
template <int NT, class F>
__device__ __forceinline__ void for_each_ij(int rows, int cols, int lane, F&& f) {
    const int n = rows * cols;
    const int di = NT / cols, dj = NT - di * cols;
    int i = lane / cols, j = lane - (lane / cols) * cols;
    for (int x = lane; x < n; x += NT) {
        f(x, i, j);
        i += di;
        j += dj;
        if (j >= cols) {
            j -= cols;
            ++i;
        }
    }
}

}  // namespace lpr
