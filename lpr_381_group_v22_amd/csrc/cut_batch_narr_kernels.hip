// cut_batch_narr_kernels.hip -- the narrated twins of k_cut_batch: the same
// state machine (cut_batch_body.hpp) with kNarr = true, which also keeps what the console text of
//   CuttingPlaneSolver.CuttingPlaneSolution  IntegerProgramming/CuttingPlaneSolver.cs:47-54, 64-229
//   DualSimplexSolver.Solve                  Simplex/DualSimplex.cs:14-114, 193-207, 228-239
//   PrimalSimplexSolver2.Solve               Simplex/PrimalSimplexSolver2.cs:46-97, 184-189
// needs -- the events, the cut rows and the tableau after every pivot -- in the layout of
// cut_narr_layout.hpp.  A handle made narrated by lpr_cut_batch_narrate_reserve launches these
// instead of k_cut_batch, in the form batch_pick_form gives the item un-narrated and with the
// same dynamic LDS.
//
//   k_cut_batch_narr<kLds>   forms G (LDS) and H (global slab)
//   k_cut_batch_narr_first   block 0 of every item: its tableau at reserve time
//   k_cut_batch_narr_call    the kCutEvCall event of every item when a run starts (and, in modes
//                            1 / 2, the kCutEvSolveBegin of the one solve the call is)
#include "cut_batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

template <bool kLds>
__global__ __launch_bounds__(256) void k_cut_batch_narr(CutBatchDesc* __restrict__ desc,
                                                        double* __restrict__ slab,
                                                        int32_t* __restrict__ logs,
                                                        CutBatchCall call, CutNarr narr,
                                                        const int32_t* __restrict__ idx_in,
                                                        int n_in, int32_t* __restrict__ idx_out,
                                                        int32_t* __restrict__ n_out) {
    constexpr bool kNarr = true;
#define LPR_CUT_BATCH_BODY_TEXT
#include "cut_batch_body.hpp"
#undef LPR_CUT_BATCH_BODY_TEXT
}

template __global__ void k_cut_batch_narr<true>(CutBatchDesc*, double*, int32_t*, CutBatchCall,
                                                CutNarr, const int32_t*, int, int32_t*, int32_t*);
template __global__ void k_cut_batch_narr<false>(CutBatchDesc*, double*, int32_t*, CutBatchCall,
                                                 CutNarr, const int32_t*, int, int32_t*, int32_t*);

// Block 0: item k's rows x cols tableau as it stands in its slice, by the push rule.
__global__ __launch_bounds__(256) void k_cut_batch_narr_first(const CutBatchDesc* __restrict__ desc,
                                                              const double* __restrict__ slab,
                                                              CutNarr narr, int count) {
    const int k = blockIdx.x;
    if (k >= count) return;
    const CutBatchDesc* const d = desc + k;
    CutNarrDesc nc = cut_narr_load(narr.desc + k);
    const int64_t n = (int64_t)d->rows * d->cols;
    double* const rec = cut_narr_block(nc, narr.data, n);
    const double* from = slab + d->t_off;
    if (rec)
        for (int64_t x = threadIdx.x; x < n; x += 256) rec[x] = from[x];
    __syncthreads();  // every lane has read the cursors
    if (threadIdx.x == 0) cut_narr_store(narr.desc + k, nc);
}

// One thread per item: the call's own events.
__global__ __launch_bounds__(256) void k_cut_batch_narr_call(const CutBatchDesc* __restrict__ desc,
                                                             CutNarr narr, int count, int mode,
                                                             int print_steps) {
    const int k = blockIdx.x * 256 + (int)threadIdx.x;
    if (k >= count) return;
    CutNarrDesc nc = cut_narr_load(narr.desc + k);
    const int R = desc[k].rows;
    int64_t at = cut_narr_event(nc);
    if (at >= 0) {
        int32_t* e = narr.ev + 4 * (nc.ev_off + at);
        e[0] = kCutEvCall;
        e[1] = mode;
        e[2] = print_steps;
        e[3] = R;
    }
    if (mode != kCutModeCuttingPlane) {
        at = cut_narr_event(nc);
        if (at >= 0) {
            int32_t* e = narr.ev + 4 * (nc.ev_off + at);
            e[0] = kCutEvSolveBegin;
            e[1] = mode == kCutModeDual ? kCutDual : kCutPrimal2;
            e[2] = 0;
            e[3] = R;
        }
    }
    cut_narr_store(narr.desc + k, nc);
}

// ------------------------------------------------------------------------------------------
// Launchers (cut_batch_engine.hip); the arguments of cut_batch_launch and the narration buffers.
int cut_batch_narr_launch(int form, hipStream_t s, CutBatchDesc* desc, double* slab,
                          int32_t* logs, const CutBatchCall& call, const CutNarr& narr, size_t lds,
                          const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out) {
    const char* const name = "k_cut_batch_narr";
    if (form != kFormG)
        return batch_launch<&k_cut_batch_narr<false>>(name, "items", form, s, n_in, lds,
                                                      kBatchMaxLdsG, desc, slab, logs, call, narr,
                                                      idx_in, n_in, idx_out, n_out);
    if (n_in > 0 && lds > kBatchMaxLdsG) {
        set_error("k_cut_batch_narr: %zu bytes of LDS asked for in form G", lds);
        return LPR_BAD_ARGUMENT;
    }
    return batch_launch<&k_cut_batch_narr<true>>(name, "items", form, s, n_in, lds, kBatchMaxLdsG,
                                                 desc, slab, logs, call, narr, idx_in, n_in,
                                                 idx_out, n_out);
}

int cut_batch_narr_launch_first(hipStream_t s, const CutBatchDesc* desc, const double* slab,
                                const CutNarr& narr, int count) {
    hipLaunchKernelGGL(k_cut_batch_narr_first, dim3(count), dim3(256), 0, s, desc, slab, narr,
                       count);
    return launch_checked("k_cut_batch_narr_first");
}

int cut_batch_narr_launch_call(hipStream_t s, const CutBatchDesc* desc, const CutNarr& narr,
                               int count, int mode, int print_steps) {
    hipLaunchKernelGGL(k_cut_batch_narr_call, dim3((count + 255) / 256), dim3(256), 0, s, desc,
                       narr, count, mode, print_steps);
    return launch_checked("k_cut_batch_narr_call");
}

}  // namespace lpr
