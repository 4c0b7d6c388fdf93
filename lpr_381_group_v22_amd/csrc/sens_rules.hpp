// sens_rules.hpp -- the rules of SensitivityAnalysis/SensitivityAnalyzer.cs (cited as :n), once
// each, for every kernel of the sensitivity family: the re-solve handle (sens_engine.hip), the
// scenario batch (sens_batch_kernels.hip) and the two reports (sens_ranging_kernels.hip,
// sens_batch_ranging_kernels.hip).  A rule here is one element or one scan step; grids, lane
// mappings, staging and which division form (ieee_div / ieee_div_n) a kernel uses stay with the
// kernel, and nothing below knows which caller it serves.  Device code only.
#pragma once
#pragma clang fp contract(off)

#include "engine_common.hpp"
#include "fold_common.hpp"
#include "select_common.hpp"

namespace lpr {

constexpr double kSensEps = 1e-9;             // :20
constexpr int kSensMaxIter = 10000;           // default maxIter of ReOptimize / DualSimplexIfNeeded
// "no column yet" while basicVars is rebuilt (memset 0x7f, then atomicMin of the columns)
constexpr int32_t kSensNoBasic = 0x7f7f7f7f;
static_assert(kSensEps == kFoldEps, "eps_fold / staged_eps_fold replay the analyzer's EPS band");

// ---- GetBasicRow / IsPivotColumn :69-84 -------------------------------------------------------
// IsPivotColumn(i, j) && |T[i][j] - 1| < EPS  <=>  exactly one row (1..R-1) of column j has
// |v| > EPS, it is row i, and |v - 1| < EPS (a row within EPS of 1 is itself counted).  So a scan
// counts such rows and sums their indices (the sum is the row itself when the count is 1).
// `|v| > EPS` is also `v > EPS || v < -EPS` on every double, a NaN being neither: a kernel that
// needs the two signs anyway (range_sign below) passes `pos || neg` as the verdict.
__device__ __forceinline__ bool above_eps(double v) { return fabs(v) > kSensEps; }

// above: above_eps of the entry of row i
__device__ __forceinline__ void basic_row_step(bool above, int i, int& cnt, int& rowsum) {
    cnt += above ? 1 : 0;
    rowsum += above ? i : 0;
}

// The verdict on a column whose entry of row i is col[i * stride]: that entry is read only when
// the count is 1 (any other row sum need not be a row).
__device__ __forceinline__ int basic_row_verdict(int cnt, int rowsum, const double* col,
                                                 int stride) {
    if (cnt == 1 && fabs(col[(size_t)rowsum * stride] - 1.0) < kSensEps) return rowsum;
    return -1;
}

// GetBasicRow of column `col` of an R-row tableau with row stride `stride`, by a whole workgroup of
// kLanes lanes; every lane gets the row.  slot: 2 * kLanes / kWave ints of LDS, free on return.
template <int kLanes>
__device__ __forceinline__ int block_basic_row(const double* T, int R, int stride, int col,
                                               int* slot) {
    int c = 0, rs = 0;
    for (int i = 1 + (int)threadIdx.x; i < R; i += kLanes)
        basic_row_step(above_eps(T[(size_t)i * stride + col]), i, c, rs);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c += __shfl_xor(c, off, kWave);
        rs += __shfl_xor(rs, off, kWave);
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
        slot[2 * wave] = c;
        slot[2 * wave + 1] = rs;
    }
    __syncthreads();
    int tc = 0, tr = 0;
    for (int w = 0; w < kLanes / kWave; ++w) {
        tc += slot[2 * w];
        tr += slot[2 * w + 1];
    }
    __syncthreads();
    return basic_row_verdict(tc, tr, T + col, stride);
}

// ---- DualSimplexIfNeeded :168-201, ReOptimize :121-166 ----------------------------------------
// The value a column / a row brings to the ratio fold `ratio < best - EPS`; NaN: not a candidate.
// `a < -EPS: ratio = cbar / (-a)` (:186-195)
__device__ __forceinline__ double dual_ratio(double cbar, double a) {
    return (a < -kSensEps) ? ieee_div(cbar, -a) : (double)NAN;
}
// `a > EPS: ratio = rhs / a` (:144-150)
__device__ __forceinline__ double primal_ratio(double rhs, double a) {
    return (a > kSensEps) ? ieee_div(rhs, a) : (double)NAN;
}

// IsOptimal (:86-96) and the entering column `rc < mostNeg`, first index (:131-141), one scan over
// the columns outside basicVars: mostNeg = 0.0 at the start, and a lane that takes its columns in
// ascending order keeps the first index with the strict <.
__device__ __forceinline__ Cand entering_start() {
    Cand best;
    best.v = 0.0;
    best.i = -1;
    return best;
}
__device__ __forceinline__ void entering_step(const int32_t* bcount, const double* zrow, int j,
                                              int& notopt, Cand& best) {
    if (bcount[j] > 0) return;  // basicVars.Contains(j)
    const double rc = zrow[j];
    if (rc < -kSensEps) notopt = 1;
    if (rc < best.v) {
        best.v = rc;
        best.i = j;
    }
}

// ---- Pivot :98-119 ------------------------------------------------------------------------------
// `|pivot| < EPS` throws (:101); a row i != leaveRow with `|factor| < EPS` is left untouched (:110)
__device__ __forceinline__ bool zero_pivot(double piv) { return fabs(piv) < kSensEps; }
__device__ __forceinline__ bool row_untouched(double factor) { return fabs(factor) < kSensEps; }

// basicVars[leaveRow - 1] = enterCol (:117-118) with the membership counts that shadow basicVars,
// and the pivot's log triple (kind: 0 dual, 1 primal) while the log has room.  One lane.
__device__ __forceinline__ void basis_enter(int32_t* basic, int32_t* bcount, int leave, int enter,
                                            int kind, int32_t* log, int64_t log_n,
                                            int64_t log_cap) {
    const int old = basic[leave - 1];
    if (old >= 0) bcount[old] -= 1;
    basic[leave - 1] = enter;
    bcount[enter] += 1;
    if (log_n < log_cap) {
        int32_t* e = log + 3 * log_n;
        e[0] = kind;
        e[1] = leave;
        e[2] = enter;
    }
}

// ---- the reports: DisplayRangeNonBasic :276-297, DisplayRangeBasic :324-359, DisplayRangeRHS
// :396-424 -----------------------------------------------------------------------------------
// Which fold an entry a feeds with -cbar / a (:351 :354) or -b / a (:415 :417): the lower one
// (Math.Max) when a > EPS, the upper one (Math.Min) when a < -EPS, none otherwise; a NaN entry is
// neither.  The division stays with the caller.
__device__ __forceinline__ void range_sign(double a, bool& pos, bool& neg) {
    pos = a > kSensEps;
    neg = a < -kSensEps;
}

// kind and var_row of column j.  member: basicVars.Contains(j); row: GetBasicRow(j), looked at
// only for a member.
__device__ __forceinline__ void range_classify(bool member, int32_t row, double cbar,
                                               int32_t& kind, int32_t& var_row) {
    var_row = -1;
    if (member) {  // DisplayRangeBasic
        if (row >= 1) {
            kind = LPR_SENS_RANGE_BASIC;
            var_row = row;
        } else {
            kind = LPR_SENS_RANGE_BASIC_ROW_NOT_FOUND;  // :337
        }
    } else if (cbar > kSensEps) {  // DisplayRangeNonBasic :291-296
        kind = LPR_SENS_RANGE_NONBASIC_RANGE;
    } else if (fabs(cbar) <= kSensEps) {
        kind = LPR_SENS_RANGE_NONBASIC_BOUNDARY;
    } else {  // negative, or NaN
        kind = LPR_SENS_RANGE_NONBASIC_NOT_OPTIMAL;
    }
}

}  // namespace lpr
