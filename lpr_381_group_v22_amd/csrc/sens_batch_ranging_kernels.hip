// sens_batch_ranging_kernels.hip -- gfx950 kernel of the scenario batch's sensitivity report
// (lpr_sens_batch_ranging): per scenario the nine outputs of
// lpr_sens_ranging (section 18), for the whole batch in one launch.
//   DisplayRangeNonBasic :276-297, DisplayRangeBasic :324-359, DisplayRangeRHS :396-424,
//   ShadowPrices :212-222, GetBasicRow / IsPivotColumn :69-84 of
//   SensitivityAnalysis/SensitivityAnalyzer.cs.
// One 256-lane workgroup per scenario reads the scenario's slice of the global slab (`alt` when the
// scenario is stopped inside an edit in form G, else `cur`), compact at the scenario's own column
// count, with basicVars' membership counts as the batch keeps them.  Three steps:
//   1. column pass: one lane per column, rows 1..R-1 ascending.  GetBasicRow of the column and, for
//      a slack column, the RHS range are both sequential scans in the C#'s own order: nothing is
//      cut, .NET's Math.Max / Math.Min are applied as written.
//   2. row pass: one wave per row that some column of basicVars has as its basic row.  Lane l folds
//      the columns l, l + 64, ... ascending and carries (value, column); the 64 lanes are combined
//      by form (b) of section 18: a NaN on either side gives NaN, otherwise the larger (smaller)
//      value, on equal values the one of the later column.  Strided ownership keeps the loads
//      coalesced; the carried column makes the +0 / -0 tie come out as the scan leaves it.
//   3. one lane per column / constraint writes the outputs, the padding past the scenario's own
//      shape included, with plain vector stores.
// No atomics, nothing depends on arrival order; the batch is only read.
#include "dotnet_minmax.hpp"  // dn_max / dn_min
#include "sens_batch_common.hpp"
#include "sens_rules.hpp"

#include <climits>

#pragma clang fp contract(off)

namespace lpr {

static_assert(kSbrWaveLanes == kWave, "a wave folds a row");
constexpr int kSbrLoad = 4;  // entries a lane loads ahead of their use (8 spill SGPRs)
constexpr int kSbrDiv = 2;   // ... and divides behind one branch (more of them spill SGPRs)
static_assert(kSbrLoad % kSbrDiv == 0, "whole division groups per load group");

// What the kernel reads of the batch (a SensBatchView carries thirteen pointers; four are needed)
struct SensBatchRangingIn {
    const SensScenario* desc;
    const double *cur, *alt;
    const int32_t* bcount;
    int SR, SC;  // the maximal shape: the strides of the slabs
};

namespace {

// One step of the scan `v = Math.Max(v, q)` that also keeps the column the value came from
__device__ __forceinline__ void dn_max_at(double& v, int& at, double q, int j) {
    const bool keep = (v > q) || (v != v);  // dn_max's own two tests
    v = dn_max(v, q);
    at = keep ? at : j;
}
__device__ __forceinline__ void dn_min_at(double& v, int& at, double q, int j) {
    const bool keep = (v < q) || (v != v);
    v = dn_min(v, q);
    at = keep ? at : j;
}
// Form (b): the results of two disjoint sets of columns.  (-inf, -1) / (+inf, -1) is the identity.
__device__ __forceinline__ void combine_max(double& v, int& at, double ov, int oat) {
    const bool take = (v == v) && ((ov != ov) || ov > v || (ov == v && oat > at));
    if (take) {
        v = ov;
        at = oat;
    }
}
__device__ __forceinline__ void combine_min(double& v, int& at, double ov, int oat) {
    const bool take = (v == v) && ((ov != ov) || ov < v || (ov == v && oat > at));
    if (take) {
        v = ov;
        at = oat;
    }
}

}  // namespace

__global__ __launch_bounds__(kSbrLanes) void k_sens_batch_ranging(SensBatchRangingIn in, int count,
                                                                  SensBatchRangingLds lds,
                                                                  SensReportOut o, int mc, int mr) {
    extern __shared__ double smem[];
    const int k = blockIdx.x;
    if (k >= count) return;
    const int tid = threadIdx.x;
    const SensScenario* const d = in.desc + k;
    const int SR = in.SR, SC = in.SC;
    const int R = d->R, C = d->C;  // the scenario's own shape: R <= SR, C <= SC, C >= R
    const int m = R - 1, nc = C - 1, n = C - R;
    const double* __restrict__ T = (d->in_alt ? in.alt : in.cur) + (size_t)k * SR * SC;
    const int32_t* __restrict__ bcount = in.bcount + (size_t)k * SC;

    char* const base = reinterpret_cast<char*>(smem);
    double* const s_b = reinterpret_cast<double*>(base + lds.b_off);
    double* const s_lo = reinterpret_cast<double*>(base + lds.lo_off);
    double* const s_hi = reinterpret_cast<double*>(base + lds.hi_off);
    int32_t* const s_cand = reinterpret_cast<int32_t*>(base + lds.cand_off);
    int32_t* const s_need = reinterpret_cast<int32_t*>(base + lds.need_off);

    for (int i = tid; i < R; i += kSbrLanes) {
        s_b[i] = T[(size_t)i * C + nc];
        s_need[i] = 0;
    }
    __syncthreads();

    // ---- 1. column pass ----
    for (int j = tid; j < nc; j += kSbrLanes) {
        const bool slack = j >= n;  // slack column of constraint j - n + 1 (:62-67)
        int c = 0, rs = 0;
        double lo = -INFINITY, hi = INFINITY;
        // kSbrLoad rows at a time: all their loads first, then kSbrDiv of them at a time through
        // one division branch (ieee_div_n) and the fold steps, in row order.  A slot that is no
        // candidate divides 0 by 1.
#pragma unroll 1
        for (int i0 = 1; i0 < R; i0 += kSbrLoad) {
            double a[kSbrLoad];
#pragma unroll
            for (int u = 0; u < kSbrLoad; ++u) {
                // unconditional loads at a clamped row (a guarded load is a branch of its own);
                // past the last row: 0.0, no candidate
                const int i = i0 + u;
                const double v = T[(size_t)(i < R ? i : R - 1) * C + j];
                a[u] = (i < R) ? v : 0.0;
            }
#pragma unroll
            for (int g = 0; g < kSbrLoad; g += kSbrDiv) {
                double num[kSbrDiv], den[kSbrDiv], q[kSbrDiv];
#pragma unroll
                for (int u = 0; u < kSbrDiv; ++u) {
                    const int i = i0 + g + u;
                    const double v = a[g + u];
                    bool pos, neg;
                    range_sign(v, pos, neg);
                    const bool cand = pos || neg;  // above_eps(v)
                    basic_row_step(cand, i, c, rs);
                    num[u] = (cand && slack) ? -s_b[i] : 0.0;  // -bi / coeff (:415 :417)
                    den[u] = (cand && slack) ? v : 1.0;
                }
                if (slack) {
                    ieee_div_n<kSbrDiv>(num, den, q);
#pragma unroll
                    for (int u = 0; u < kSbrDiv; ++u) {
                        bool pos, neg;
                        range_sign(a[g + u], pos, neg);
                        lo = pos ? dn_max(lo, q[u]) : lo;
                        hi = neg ? dn_min(hi, q[u]) : hi;
                    }
                }
            }
        }
        const int r = basic_row_verdict(c, rs, T + j, C);  // GetBasicRow (:69-84)
        const bool member = bcount[j] > 0;  // basicVars.Contains(j)
        s_cand[j] = member ? r : -1;
        if (member && r >= 1) s_need[r] = 1;  // every writer stores the same 1
        if (slack) {
            const size_t t = (size_t)k * mr + (j - n);
            o.shadow[t] = T[j];
            o.rlo[t] = lo;
            o.rhi[t] = hi;
            o.now[t] = s_b[j - n + 1];
        }
    }
    __syncthreads();

    // ---- 2. row pass ----
    {
        const int lane = tid & (kSbrWaveLanes - 1), wave = tid / kSbrWaveLanes;
        for (int i = 1 + wave; i < R; i += kSbrWaves) {
            if (!s_need[i]) continue;  // the same in every lane of the wave
            const double* __restrict__ row = T + (size_t)i * C;
            double lo = -INFINITY, hi = INFINITY;
            int lo_at = -1, hi_at = -1;
#pragma unroll 1
            for (int j0 = lane; j0 < nc; j0 += kSbrLoad * kSbrWaveLanes) {
                double a[kSbrLoad], z[kSbrLoad];
#pragma unroll
                for (int u = 0; u < kSbrLoad; ++u) {
                    const int j = j0 + u * kSbrWaveLanes;
                    // basicVars.Contains(j) skips the column (:345; `j == index` there is dead)
                    // (unconditional loads at a clamped column, as in the column pass)
                    const int jc = j < nc ? j : nc - 1;
                    const bool free = j < nc && bcount[jc] == 0;
                    const double v = row[jc];
                    a[u] = free ? v : 0.0;
                    z[u] = T[jc];
                }
#pragma unroll
                for (int g = 0; g < kSbrLoad; g += kSbrDiv) {
                    double num[kSbrDiv], den[kSbrDiv], q[kSbrDiv];
#pragma unroll
                    for (int u = 0; u < kSbrDiv; ++u) {
                        const double v = a[g + u];
                        bool pos, neg;
                        range_sign(v, pos, neg);
                        const bool cand = pos || neg;
                        num[u] = cand ? -z[g + u] : 0.0;  // -cbar_j / a_rj (:351 :354)
                        den[u] = cand ? v : 1.0;
                    }
                    ieee_div_n<kSbrDiv>(num, den, q);
#pragma unroll
                    for (int u = 0; u < kSbrDiv; ++u) {  // the lane's columns ascend
                        const int j = j0 + (g + u) * kSbrWaveLanes;
                        bool pos, neg;
                        range_sign(a[g + u], pos, neg);
                        if (pos) dn_max_at(lo, lo_at, q[u], j);
                        if (neg) dn_min_at(hi, hi_at, q[u], j);
                    }
                }
            }
#pragma unroll
            for (int off = kSbrWaveLanes / 2; off > 0; off >>= 1) {
                const double olo = __shfl_xor(lo, off, kSbrWaveLanes);
                const int olo_at = __shfl_xor(lo_at, off, kSbrWaveLanes);
                const double ohi = __shfl_xor(hi, off, kSbrWaveLanes);
                const int ohi_at = __shfl_xor(hi_at, off, kSbrWaveLanes);
                combine_max(lo, lo_at, olo, olo_at);
                combine_min(hi, hi_at, ohi, ohi_at);
            }
            if (lane == 0) {
                s_lo[i] = lo;
                s_hi[i] = hi;
            }
        }
    }
    __syncthreads();

    // ---- 3. the outputs, padded to the batch's maximal shape ----
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int j = tid; j < mc; j += kSbrLanes) {
        const size_t t = (size_t)k * mc + j;
        if (j < nc) {
            const double cbar = T[j];
            double lo = -INFINITY, hi = INFINITY;
            const bool member = bcount[j] > 0;  // basicVars.Contains(j)
            int32_t kind, vr;
            range_classify(member, member ? s_cand[j] : -1, cbar, kind, vr);
            if (kind == LPR_SENS_RANGE_BASIC) {
                lo = s_lo[vr];
                hi = s_hi[vr];
            }
            o.rc[t] = cbar;
            o.clo[t] = lo;
            o.chi[t] = hi;
            o.kind[t] = kind;
            o.row[t] = vr;
        } else {
            o.rc[t] = qnan;
            o.clo[t] = qnan;
            o.chi[t] = qnan;
            o.kind[t] = INT32_MIN;
            o.row[t] = INT32_MIN;
        }
    }
    for (int i = m + tid; i < mr; i += kSbrLanes) {
        const size_t t = (size_t)k * mr + i;
        o.shadow[t] = qnan;
        o.rlo[t] = qnan;
        o.rhi[t] = qnan;
        o.now[t] = qnan;
    }
}

// the one launch on `s` (declared in sens_batch_common.hpp)
int sens_batch_ranging_launch(hipStream_t s, const SensBatchView& vw, char* out,
                              const SensBatchRangingPlan& pl) {
    const SensReportOut o = sens_report_bind(out, pl.out);
    SensBatchRangingIn in;
    in.desc = vw.desc;
    in.cur = vw.cur;
    in.alt = vw.alt;
    in.bcount = vw.bcount;
    in.SR = vw.R;
    in.SC = vw.C;
    const SensBatchRangingLds lds = sens_batch_ranging_lds(vw.R, vw.C);
    hipLaunchKernelGGL(k_sens_batch_ranging, dim3(pl.count), dim3(kSbrLanes), (size_t)lds.total, s,
                       in, pl.count, lds, o, pl.mc, pl.mr);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        set_error("k_sens_batch_ranging (%d scenarios) failed to launch: %s", pl.count,
                  hipGetErrorString(err));
        return LPR_DEVICE_ERROR;
    }
    return LPR_OK_OPTIMAL;
}

}  // namespace lpr
