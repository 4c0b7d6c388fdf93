// cut_batch_kernels.hip -- the batched cutting plane: many option-4
// tableaux per launch, each taken through the whole recursion of
//   CuttingPlaneSolver.CuttingPlaneSolution  IntegerProgramming/CuttingPlaneSolver.cs:64-229
//   DualSimplexSolver.Solve                  Simplex/DualSimplex.cs:14-114
//   PrimalSimplexSolver2.Solve               Simplex/PrimalSimplexSolver2.cs:46-97
// with the rules of cut_kernels.hip (k_cut_select, k_cut_add, k_cut_update, k_cut_flags and the
// host loop of lpr_cutting_plane): the same bits as that call gives on a fresh lpr_tableau.
//
//   k_cut_batch<kLds>   one 256-lane workgroup per item expands the state machine of
//                       cut_batch_body.hpp (kNarr = false); at most `chunk` pivots per launch;
//                       the tableau in LDS (form G) or in the item's slice of the global slab
//                       (form H).  Its narrated twins are in cut_batch_narr_kernels.hip.
//   k_cut_batch_load    the tableaux into their slices (lpr_cut_batch_create / _from_batch)
#include "cut_batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

template <bool kLds>
__global__ __launch_bounds__(256) void k_cut_batch(CutBatchDesc* __restrict__ desc,
                                                   double* __restrict__ slab,
                                                   int32_t* __restrict__ logs, CutBatchCall call,
                                                   const int32_t* __restrict__ idx_in, int n_in,
                                                   int32_t* __restrict__ idx_out,
                                                   int32_t* __restrict__ n_out) {
    constexpr bool kNarr = false;
    const CutNarr narr{};
#define LPR_CUT_BATCH_BODY_TEXT
#include "cut_batch_body.hpp"
#undef LPR_CUT_BATCH_BODY_TEXT
}

template __global__ void k_cut_batch<true>(CutBatchDesc*, double*, int32_t*, CutBatchCall,
                                           const int32_t*, int, int32_t*, int32_t*);
template __global__ void k_cut_batch<false>(CutBatchDesc*, double*, int32_t*, CutBatchCall,
                                            const int32_t*, int, int32_t*, int32_t*);

// Tableau k (rows x cols, compact, at src + src_off[k]) into the front of its slice; z of the
// descriptor with it.
__global__ __launch_bounds__(256) void k_cut_batch_load(CutBatchDesc* __restrict__ desc, int count,
                                                        const double* __restrict__ src,
                                                        const int64_t* __restrict__ src_off,
                                                        double* __restrict__ slab) {
    const int k = blockIdx.x;
    if (k >= count) return;
    CutBatchDesc* const d = desc + k;
    const int n = d->rows * d->cols;
    const double* from = src + src_off[k];
    double* to = slab + d->t_off;
    for (int x = threadIdx.x; x < n; x += 256) to[x] = from[x];
    if (threadIdx.x == 0) d->z = from[d->cols - 1];
}

// ------------------------------------------------------------------------------------------
// Launchers (cut_batch_engine.hip).  lds: the largest dynamic LDS an item of this list needs.
int cut_batch_launch(int form, hipStream_t s, CutBatchDesc* desc, double* slab, int32_t* logs,
                     const CutBatchCall& call, size_t lds, const int32_t* idx_in, int n_in,
                     int32_t* idx_out, int32_t* n_out) {
    const char* const name = "k_cut_batch";
    if (form != kFormG)
        return batch_launch<&k_cut_batch<false>>(name, "items", form, s, n_in, lds, kBatchMaxLdsG,
                                                 desc, slab, logs, call, idx_in, n_in, idx_out,
                                                 n_out);
    if (n_in > 0 && lds > kBatchMaxLdsG) {
        set_error("k_cut_batch: %zu bytes of LDS asked for in form G", lds);
        return LPR_BAD_ARGUMENT;
    }
    return batch_launch<&k_cut_batch<true>>(name, "items", form, s, n_in, lds, kBatchMaxLdsG, desc,
                                            slab, logs, call, idx_in, n_in, idx_out, n_out);
}

int cut_batch_launch_load(hipStream_t s, CutBatchDesc* desc, int count, const double* src,
                          const int64_t* src_off, double* slab) {
    hipLaunchKernelGGL(k_cut_batch_load, dim3(count), dim3(256), 0, s, desc, count, src, src_off,
                       slab);
    return launch_checked("k_cut_batch_load");
}

}  // namespace lpr
