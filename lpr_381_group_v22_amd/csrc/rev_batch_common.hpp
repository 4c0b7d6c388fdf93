// rev_batch_common.hpp -- definitions shared by the batched revised simplex (rev_batch_engine.hip,
// host) and its kernels (rev_batch_body.hpp, instantiated by rev_batch_kernels.hip and, traced, by
// rev_batch_trace_kernels.hip); DESIGN.md sections 17 and 21.  The forms, the rule that picks one,
// the running-list driver and the handle plumbing are those of batch_common.hpp.  Not part of the
// ABI (include/lpr_engine.h is).
#pragma once

#include "batch_common.hpp"

namespace lpr {

// What one LP keeps resident while a launch works on it (doubles).  B^-1 (m x m) and A (m x n)
// are in LDS in forms W and G, with ODD leading dimensions: the row walks (x_B = B^-1 b and
// u = B^-1 a_e, lane i down row i) would otherwise put every lane on the same bank whenever the
// leading dimension is a multiple of 32 doubles.  The vectors are in LDS in every form:
//   kRevBatchVecM vectors of m  b, c_B, x_B, y (later the staged ratios), u (later the column fac
//                               of E), and the saved pivot row of B^-1 (before that: a_e)
//   c                           n
//   the staged candidates       n + m: v = -rc of the entering fold, NaN = not a candidate
//   basis                       m int32, rounded up to whole doubles
//   the non-basic flags         n + m bytes, rounded up to whole doubles
constexpr int kRevBatchVecM = 6;
constexpr int rev_batch_ld(int k) { return k | 1; }
constexpr size_t rev_batch_vectors(int m, int n) {
    return (size_t)kRevBatchVecM * m + n + (size_t)(n + m) + (size_t)(m + 1) / 2 +
           (size_t)(n + m + 7) / 8;
}
constexpr size_t rev_batch_footprint(int m, int n) {  // forms W and G
    return (size_t)m * rev_batch_ld(m) + (size_t)m * rev_batch_ld(n) + rev_batch_vectors(m, n);
}
// H: B^-1 and A stay in the LP's slice of the global slab, compact.  A row walk stages
// 256 rows x kRevBatchTileCols columns at a time in LDS (leading dimension + 1, odd), so that the
// global loads are contiguous runs of 128 bytes while each lane keeps its own sequential sum.
constexpr int kRevBatchTileCols = 16;
constexpr size_t kRevBatchTile = (size_t)256 * (kRevBatchTileCols + 1);
// The shapes lpr_batch_from_lps takes: rows = m + 1 <= kBatchMaxRowsH, cols = n + m + 1 <=
// kBatchMaxColsH.
constexpr int kRevBatchMaxM = kBatchMaxRowsH - 1;
constexpr int kRevBatchMaxNM = kBatchMaxColsH - 1;
static_assert((rev_batch_vectors(kRevBatchMaxM, kRevBatchMaxNM - kRevBatchMaxM) + kRevBatchTile) *
                      sizeof(double) <= kBatchMaxLdsG,
              "form H keeps the vectors of the largest LP and one tile in dynamic LDS");
// Iterations per LP per launch, by form: no launch runs without a bound, even on an LP that cycles.
constexpr int kRevBatchChunk[kNumForms] = {256, 128, 16};
static_assert(sizeof(kRevBatchChunk) / sizeof(int) == kNumForms, "one chunk per form");

// One LP of a batch, in device memory.  Its slice of the slab (doubles, compact) is
//   B^-1 (m x m) | A (m x n) | b (m) | c (n, negated when is_min, :51) | c_B (m) | x_B (m)
struct RevBatchDesc {
    int64_t s_off;     // the slice, at slab + s_off
    int64_t b_off;     // basis: m entries at basis + b_off
    int64_t log_off;   // pivot log: log_cap (row, enter, leave) triples at log + 3 * log_off
    int64_t x_off;     // solution: n entries at x + x_off, written on the optimal exit only
    int64_t iter;      // iterations so far (exact; the log keeps the first log_cap)
    int64_t max_iter;  // this call stops when iter reaches it (<= 0: no limit)
    double z;          // FinalZ = Dot(cOrig, x), written on the optimal exit only
    int32_t n, m;
    int32_t log_cap;
    int32_t status;    // kRunning or an lpr_status
    int32_t log_fill;  // triples kept: min(iter, log_cap)
    int32_t is_min;
};

inline int64_t rev_batch_slice(int m, int n) {  // doubles
    return (int64_t)m * m + (int64_t)m * n + 3 * (int64_t)m + n;
}

// One CaptureSnapshot (:294-387) of a traced batch as numbers, in doubles,
// indices stored as doubles:
//   [0] enteringIdx  [1] leavingRow  [2] leavingVarIndex_Pre  [3] enteringRC_pre  [4] zWorking
//   [5] zOriginal, then y[m], rcX[n], rcS[m], u_pre[m], ratios_pre[m], basisForRatios_Pre[m],
//   basicVariables (post)[m], xB[m], BInvA[m x n], BInv[m x m]
// LP k's records are at trace + trace_off[k], rev_trace_stride apart, the first trace_cap kept.
enum RevTraceScalar : int {
    kRevTraceEnter = 0, kRevTraceRow = 1, kRevTraceLeave = 2, kRevTraceRcPre = 3,
    kRevTraceZWorking = 4, kRevTraceZOriginal = 5, kRevTraceScalars = 6
};
constexpr int64_t rev_trace_y(int, int) { return kRevTraceScalars; }
constexpr int64_t rev_trace_rcx(int m, int n) { return rev_trace_y(m, n) + m; }
constexpr int64_t rev_trace_rcs(int m, int n) { return rev_trace_rcx(m, n) + n; }
constexpr int64_t rev_trace_u(int m, int n) { return rev_trace_rcs(m, n) + m; }
constexpr int64_t rev_trace_ratios(int m, int n) { return rev_trace_u(m, n) + m; }
constexpr int64_t rev_trace_basis_pre(int m, int n) { return rev_trace_ratios(m, n) + m; }
constexpr int64_t rev_trace_basis_post(int m, int n) { return rev_trace_basis_pre(m, n) + m; }
constexpr int64_t rev_trace_xb(int m, int n) { return rev_trace_basis_post(m, n) + m; }
constexpr int64_t rev_trace_binva(int m, int n) { return rev_trace_xb(m, n) + m; }
constexpr int64_t rev_trace_binv(int m, int n) { return rev_trace_binva(m, n) + (int64_t)m * n; }
constexpr int64_t rev_trace_stride(int m, int n) { return rev_trace_binv(m, n) + (int64_t)m * m; }
static_assert(rev_trace_stride(3, 4) == 6 + 7 * 3 + 4 + 3 * 4 + 3 * 3, "6 + 7m + n + mn + mm");

// Where a traced batch keeps its records; all zero for an untraced one.
struct RevBatchTrace {
    double* slab;        // every LP's records
    const int64_t* off;  // per LP, doubles
    int32_t cap;         // records kept per LP; a record index >= cap is counted, not written
};

// Inputs of lpr_rev_batch_create per LP: offsets into the packed arrays.
struct RevBatchBuild {
    int64_t obj_off;  // objective: n entries
    int64_t a_off;    // A: m x n row-major
    int64_t row_off;  // b: m entries
};

// rev_batch_kernels.hip and, traced, rev_batch_trace_kernels.hip: the launchers
// rev_batch_engine.hip calls
int rev_batch_launch(int form, hipStream_t s, RevBatchDesc* desc, double* slab, int32_t* basis,
                     int32_t* logs, double* xs, const int32_t* idx_in, int n_in,
                     int32_t* idx_out, int32_t* n_out, int chunk, int slot_doubles);
int rev_batch_trace_launch(int form, hipStream_t s, RevBatchDesc* desc, double* slab,
                           int32_t* basis, int32_t* logs, double* xs, const int32_t* idx_in,
                           int n_in, int32_t* idx_out, int32_t* n_out, int chunk,
                           int slot_doubles, RevBatchTrace tr);
void rev_batch_launch_build(hipStream_t s, const RevBatchDesc* desc, const RevBatchBuild* bd,
                            int count, double* slab, int32_t* basis, double* xs,
                            const double* obj, const double* A, const double* rhs);

}  // namespace lpr
