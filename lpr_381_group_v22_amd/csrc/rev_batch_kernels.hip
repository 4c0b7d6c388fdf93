// rev_batch_kernels.hip -- the batched revised primal simplex: many
// independent LPs per launch, each solved with the rules of RevisedPrimalSimplexSolver
// (Simplex/RevisedPrimalSimplexSolver.cs), the same bits as lpr_revised_solve and the oracle give
// for that LP alone.
//
//   k_rev_batch<NT, kLds>  the loop of Solve() (:82-251) and ExtractSolution (:277-287), at most
//                          `chunk` passes per LP per launch; NT lanes per LP (64: form W, 256:
//                          forms G and H), B^-1 and A in LDS (W, G) or in the global slab (H)
//   k_rev_batch_build      the constructor (:41-80) for every LP of lpr_rev_batch_create
//
// Every sum is one lane's sequential chain in the C#'s index order from 0, each product rounded
// before it is added; the lanes of an LP share outputs, never a sum.
#include "rev_batch_body.hpp"

#pragma clang fp contract(off)

namespace lpr {

// The loop of rev_batch_body.hpp without its trace steps.
template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_rev_batch(RevBatchDesc* __restrict__ desc,
                                                   double* __restrict__ slab,
                                                   int32_t* __restrict__ basis,
                                                   int32_t* __restrict__ logs,
                                                   double* __restrict__ xs,
                                                   const int32_t* __restrict__ idx_in, int n_in,
                                                   int32_t* __restrict__ idx_out,
                                                   int32_t* __restrict__ n_out, int chunk,
                                                   int slot) {
    rev_batch_run<NT, kLds, false>(desc, slab, basis, logs, xs, idx_in, n_in, idx_out, n_out,
                                   chunk, slot, RevBatchTrace{nullptr, nullptr, 0});
}

template __global__ void k_rev_batch<kWave, true>(RevBatchDesc*, double*, int32_t*, int32_t*,
                                                  double*, const int32_t*, int, int32_t*,
                                                  int32_t*, int, int);
template __global__ void k_rev_batch<256, true>(RevBatchDesc*, double*, int32_t*, int32_t*,
                                                double*, const int32_t*, int, int32_t*, int32_t*,
                                                int, int);
template __global__ void k_rev_batch<256, false>(RevBatchDesc*, double*, int32_t*, int32_t*,
                                                 double*, const int32_t*, int, int32_t*, int32_t*,
                                                 int, int);

// ------------------------------------------------------------------------------------------
// Constructor  RevisedPrimalSimplexSolver.cs:41-80, one wave per LP, every element of the slice
// written (the slab is not zero-filled first): B^-1 = I, A, b, c = -objective when is_min (:51),
// c_B = 0, x_B = 0, basis[i] = n + i, x = 0.
__global__ __launch_bounds__(256) void k_rev_batch_build(const RevBatchDesc* __restrict__ desc,
                                                         const RevBatchBuild* __restrict__ bd,
                                                         int count, double* __restrict__ slab,
                                                         int32_t* __restrict__ basis,
                                                         double* __restrict__ xs,
                                                         const double* __restrict__ obj,
                                                         const double* __restrict__ A,
                                                         const double* __restrict__ rhs) {
    const int k = blockIdx.x * 4 + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (k >= count) return;
    const RevBatchDesc& d = desc[k];
    const RevBatchBuild& in = bd[k];
    const int n = d.n, m = d.m;
    const bool mn = d.is_min != 0;
    double* Bg = slab + d.s_off;
    double* Ag = Bg + (size_t)m * m;
    double* bg = Ag + (size_t)m * n;
    double* cg = bg + m;
    double* cBg = cg + n;
    double* xBg = cBg + m;
    for_each_ij<kWave>(m, m, lane, [&](int x, int i, int j) { Bg[x] = (i == j) ? 1.0 : 0.0; });
    for (int x = lane; x < m * n; x += kWave) Ag[x] = A[in.a_off + x];
    for (int i = lane; i < m; i += kWave) {
        bg[i] = rhs[in.row_off + i];
        cBg[i] = 0.0;
        xBg[i] = 0.0;
        basis[d.b_off + i] = n + i;
    }
    for (int j = lane; j < n; j += kWave) {
        const double v = obj[in.obj_off + j];
        cg[j] = mn ? -v : v;
        xs[d.x_off + j] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// Launchers (rev_batch_engine.hip).  slot_doubles: W and G, the LDS share of one LP; H, the
// vectors of the largest LP (the tile follows them).
int rev_batch_launch(int form, hipStream_t s, RevBatchDesc* desc, double* slab, int32_t* basis,
                     int32_t* logs, double* xs, const int32_t* idx_in, int n_in,
                     int32_t* idx_out, int32_t* n_out, int chunk, int slot_doubles) {
    const char* const name = "k_rev_batch";
    const size_t lds = rev_batch_lds(form, slot_doubles);
    if (form == kFormW)
        return batch_launch<&k_rev_batch<kWave, true>>(
            name, "LPs", form, s, n_in, lds, kBatchMaxLdsG, desc, slab, basis, logs, xs, idx_in,
            n_in, idx_out, n_out, chunk, slot_doubles);
    if (form == kFormG)
        return batch_launch<&k_rev_batch<256, true>>(
            name, "LPs", form, s, n_in, lds, kBatchMaxLdsG, desc, slab, basis, logs, xs, idx_in,
            n_in, idx_out, n_out, chunk, slot_doubles);
    return batch_launch<&k_rev_batch<256, false>>(
        name, "LPs", form, s, n_in, lds, kBatchMaxLdsG, desc, slab, basis, logs, xs, idx_in, n_in,
        idx_out, n_out, chunk, 0);
}

void rev_batch_launch_build(hipStream_t s, const RevBatchDesc* desc, const RevBatchBuild* bd,
                            int count, double* slab, int32_t* basis, double* xs,
                            const double* obj, const double* A, const double* rhs) {
    hipLaunchKernelGGL(k_rev_batch_build, dim3((count + 3) / 4), dim3(256), 0, s, desc, bd, count,
                       slab, basis, xs, obj, A, rhs);
}

}  // namespace lpr
