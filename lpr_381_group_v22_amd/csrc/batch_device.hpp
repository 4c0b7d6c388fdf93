// batch_device.hpp -- device helpers shared by the kernels of the four batch engines
// (batch_kernels.hip, bb_batch_kernels.hip, sens_batch_kernels.hip, cut_batch_kernels.hip): the
// ordering and the candidate minimum over the NT lanes that work on one item, the walk over a
// flattened rows x cols block, and the staged EPS-band fold of the two engines that replay the
// C#'s sequential selections.  (The pivots that walk with four elements in flight,
// k_batch_simplex, k_sens_batch and k_cut_batch, keep that loop open-coded: through a shared
// helper k_sens_batch compiles to different code.)  The host side of what the engines share is batch_common.hpp.
#pragma once

#include "engine_common.hpp"
#include "fold_common.hpp"
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

// The C#'s "take idx when val(idx) < best - EPS" fold over ascending idx, replayed as it is
// written: the whole workgroup has staged val(idx) for idx in [lo, hi) (NaN = not a candidate) in
// LDS, and one wave walks the values 64 at a time; a ballot finds the first lane after the last
// take with val < best - EPS, which is what the sequential loop takes next.  This is the replay
// stage of eps_fold (fold_common.hpp) without its prefix-minimum compaction: eps_fold keeps 12 KiB
// of static LDS per instantiation for the compacted candidates, and form G leaves a workgroup
// 1 KiB besides its tableau.  Returns the last index taken (-1: none), to every lane.
__device__ __forceinline__ int staged_eps_fold(const double* stage, int lo, int hi, double best,
                                               int* slot) {
    if (threadIdx.x < kWave) {
        const int lane = threadIdx.x;
        int cur = -1;
        for (int b0 = lo; b0 < hi; b0 += kWave) {
            const int idx = b0 + lane;
            const double x = (idx < hi) ? stage[idx] : (double)NAN;
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
        if (lane == 0) *slot = cur;
    }
    __syncthreads();
    const int r = *slot;
    __syncthreads();  // the slot is free for the next fold
    return r;
}

}  // namespace lpr
