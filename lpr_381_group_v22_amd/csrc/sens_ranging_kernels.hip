// sens_ranging_kernels.hip -- gfx950 kernels of the sensitivity report (lpr_sens_ranging, DESIGN.md
// section 18): every cost range and every right-hand-side range of an analyzer from one read of
// its tableau.
//   DisplayRangeNonBasic :276-297, DisplayRangeBasic :324-359, DisplayRangeRHS :396-424,
//   ShadowPrices :212-222 of SensitivityAnalysis/SensitivityAnalyzer.cs.
// A range is a fold of .NET Framework's Math.Max / Math.Min over -cbar / a along one tableau row
// (basic ranges) or over -b / coeff down one slack column (RHS ranges).  Such a fold can be cut
// into CONTIGUOUS segments and the segments' results combined with the same Max / Min, the left
// segment as first argument (-inf / +inf is the identity): with no NaN the fold returns the largest
// value and among equal values the LAST in scan order (only +0 against -0 shows in the bits), a
// NaN sticks once met, and the combine keeps both properties.  Everything below is that one rule:
// a lane folds its two adjacent columns, lanes are combined in lane order (= column order), tiles
// in tile order by the second launch.  No atomics, nothing depends on arrival order.
#include "dotnet_minmax.hpp"  // dn_max / dn_min
#include "engine_common.hpp"
#include "sens_ranging_common.hpp"
#include "sens_rules.hpp"

#pragma clang fp contract(off)

namespace lpr {

// One pass over rows 1..m.  Grid (tile columns, tile rows), tile = kRngTileRows x kRngTileCols.
// Every element is read from HBM once (one dwordx4 per lane and row); it feeds its row's partial
// when its column is not in basicVars, and its column's partial when the column is a slack column.
// The Z-row pair, the membership counts of the pair and (per sub-pass) the RHS values of the rows
// sit in registers, loaded one sub-pass ahead.  Row partials of a sub-pass go through LDS: lane l writes (lo, hi) of its column
// pair, then 32 threads per row fold 8 consecutive lanes each and an in-order shuffle tree folds
// the 32 results.  Column partials never leave the lane: rows ascend within a tile.
//   rowpart[(i - 1) * ntc + tile column] = (lo, hi) of row i over the tile's columns
//   colpart[tile row * m + (s - n)]      = (lo, hi) of slack column s over the tile's rows
// The `j == index` test of :345 is dead -- the guard at :330 has put `index` into basicVars, so
// basicVars.Contains(j) already skips it -- and so the fold of a row does not depend on which
// basic column asks for it.
__global__ __launch_bounds__(kRngLanes) void k_sens_ranging_sweep(
    const double* __restrict__ T, int ld, int R, int C, int n, const int32_t* __restrict__ bcount,
    double2* __restrict__ rowpart, int ntc, double2* __restrict__ colpart) {
    __shared__ double s_lo[kRngSubRows * kRngLdsStride];
    __shared__ double s_hi[kRngSubRows * kRngLdsStride];
    const int tid = threadIdx.x;
    const int tc = blockIdx.x, tr = blockIdx.y;
    const int m = R - 1, nc = C - 1;
    const int c2 = tc * kRngLanes + tid;
    const int j0 = 2 * c2;
    const int ld2 = ld >> 1;  // ld is a multiple of 16
    const bool in_ld = c2 < ld2;
    double z[2];
    bool rowok[2], colok[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int j = j0 + e;
        const bool valid = j < nc;  // the RHS column and the padding take no part
        z[e] = valid ? T[j] : 0.0;
        rowok[e] = valid && bcount[j] == 0;  // !basicVars.Contains(j)
        colok[e] = valid && j >= n;          // slack column of constraint j - n + 1
    }
    // does the tile hold a slack column at all?  (the same in every lane)
    const bool slack_tile = tc * kRngTileCols + kRngTileCols > n && tc * kRngTileCols < nc;
    double clo[2] = {-INFINITY, -INFINITY}, chi[2] = {INFINITY, INFINITY};
    const double2* __restrict__ T2 = reinterpret_cast<const double2*>(T);
    const int i_base = 1 + tr * kRngTileRows;

    double2 x[kRngSubRows];
    double b[kRngSubRows];
    // rows i0 .. i0 + 7 of the lane's column pair, and their RHS values where the tile needs them
    auto load_rows = [&](int i0) {
#pragma unroll
        for (int k = 0; k < kRngSubRows; ++k) {
            const int i = i0 + k;
            x[k] = (i < R && in_ld) ? T2[(size_t)i * ld2 + c2] : make_double2(0.0, 0.0);
            b[k] = (slack_tile && i < R) ? T[(size_t)i * ld + nc] : 0.0;
        }
    };
    load_rows(i_base);
    for (int sp = 0; sp < kRngTileRows / kRngSubRows; ++sp) {
        const int i0 = i_base + sp * kRngSubRows;
        if (i0 >= R) break;
#pragma unroll
        for (int k = 0; k < kRngSubRows; ++k) {
            double lo = -INFINITY, hi = INFINITY;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double a = e ? x[k].y : x[k].x;
                bool pos, neg;
                range_sign(a, pos, neg);
                if (pos || neg) {
                    if (rowok[e]) {
                        const double q = ieee_div(-z[e], a);  // -cbar_j / a_rj (:351 :354)
                        if (pos) lo = dn_max(lo, q);
                        else hi = dn_min(hi, q);
                    }
                    if (colok[e]) {
                        const double q = ieee_div(-b[k], a);  // -bi / coeff (:415 :417)
                        if (pos) clo[e] = dn_max(clo[e], q);
                        else chi[e] = dn_min(chi[e], q);
                    }
                }
            }
            const int p = k * kRngLdsStride + tid + (tid >> 3);
            s_lo[p] = lo;
            s_hi[p] = hi;
        }
        // the next sub-pass's rows are on their way while this one goes through LDS (rows past
        // the tile or the tableau load nothing)
        if (sp + 1 < kRngTileRows / kRngSubRows) load_rows(i0 + kRngSubRows);
        __syncthreads();
        {
            const int r = tid >> 5, seg = tid & 31;
            const int base = r * kRngLdsStride + seg * 9;  // lanes 8 seg .. 8 seg + 7
            double lo = s_lo[base], hi = s_hi[base];
#pragma unroll
            for (int q = 1; q < 8; ++q) {
                lo = dn_max(lo, s_lo[base + q]);
                hi = dn_min(hi, s_hi[base + q]);
            }
            // thread seg holds [seg, seg + off) and takes [seg + off, seg + 2 off) as the right
            // argument: thread 0 of the 32 ends with all of them in order
#pragma unroll
            for (int off = 1; off < 32; off <<= 1) {
                const double olo = __shfl_down(lo, off, 32);
                const double ohi = __shfl_down(hi, off, 32);
                lo = dn_max(lo, olo);
                hi = dn_min(hi, ohi);
            }
            const int i = i0 + r;
            if (seg == 0 && i < R) rowpart[(size_t)(i - 1) * ntc + tc] = make_double2(lo, hi);
        }
        __syncthreads();
    }
    if (slack_tile) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (colok[e]) colpart[(size_t)tr * m + (j0 + e - n)] = make_double2(clo[e], chi[e]);
    }
}

// The launch boundary is the reduce: thread t folds the row slab of column t's basic row, and the
// column slab of constraint t + 1, in tile order, and writes the report.  cand = GetBasicRow of
// every column, made by k_sens_colscan + k_sens_cand on zeroed scratch just before the sweep.
__global__ __launch_bounds__(256) void k_sens_ranging_finish(
    const double* __restrict__ T, int ld, int R, int C, int n, const int32_t* __restrict__ bcount,
    const int32_t* __restrict__ cand, const double2* __restrict__ rowpart, int ntc,
    const double2* __restrict__ colpart, int ntr, SensReportOut o) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = R - 1, nc = C - 1;
    if (t < nc) {
        const double cbar = T[t];
        double lo = -INFINITY, hi = INFINITY;
        const bool member = bcount[t] > 0;  // basicVars.Contains(t)
        int32_t kind, vr;
        range_classify(member, member ? cand[t] : -1, cbar, kind, vr);
        if (kind == LPR_SENS_RANGE_BASIC) {
            const double2* __restrict__ p = rowpart + (size_t)(vr - 1) * ntc;
#pragma unroll 4
            for (int q = 0; q < ntc; ++q) {
                const double2 v = p[q];
                lo = dn_max(lo, v.x);
                hi = dn_min(hi, v.y);
            }
        }
        o.rc[t] = cbar;
        o.clo[t] = lo;
        o.chi[t] = hi;
        o.kind[t] = kind;
        o.row[t] = vr;
    }
    if (t < m) {  // constraint k = t + 1, slack column n + t
        double lo = -INFINITY, hi = INFINITY;
#pragma unroll 8  // the loads of 8 tile rows in flight; the fold itself stays in tile order
        for (int q = 0; q < ntr; ++q) {
            const double2 v = colpart[(size_t)q * m + t];
            lo = dn_max(lo, v.x);
            hi = dn_min(hi, v.y);
        }
        o.shadow[t] = T[n + t];
        o.rlo[t] = lo;
        o.rhi[t] = hi;
        o.now[t] = T[(size_t)(t + 1) * ld + nc];
    }
}

// both launches on `st` (declared in engine_common.hpp)
int sens_ranging_launch(hipStream_t st, const double* T, int ld, int R, int C,
                        const int32_t* bcount, const int32_t* cand, char* ws,
                        const SensRangingPlan& pl, hipEvent_t ev_mid) {
    double2* rowpart = reinterpret_cast<double2*>(ws + pl.rowpart_off);
    double2* colpart = reinterpret_cast<double2*>(ws + pl.colpart_off);
    const SensReportOut o = sens_report_bind(ws, pl.out);
    hipLaunchKernelGGL(k_sens_ranging_sweep, dim3(pl.ntc, pl.ntr), dim3(kRngLanes), 0, st, T, ld, R,
                       C, pl.n, bcount, rowpart, pl.ntc, colpart);
    LPR_HIP(hipGetLastError());
    if (ev_mid) LPR_HIP(hipEventRecord(ev_mid, st));
    const int nt = pl.nc > pl.m ? pl.nc : pl.m;
    hipLaunchKernelGGL(k_sens_ranging_finish, dim3((nt + 255) / 256), dim3(256), 0, st, T, ld, R, C,
                       pl.n, bcount, cand, rowpart, pl.ntc, colpart, pl.ntr, o);
    LPR_HIP(hipGetLastError());
    return LPR_OK_OPTIMAL;
}

}  // namespace lpr
