// batch_common.hpp -- definitions shared by the batched primal simplex (batch_engine.hip, host)
// and its kernels (batch_kernels.hip).  Not part of the ABI (include/lpr_engine.h is).
#pragma once

#include "engine_common.hpp"

namespace lpr {

// Forms of one LP in a batch.  The host picks one per LP by its LDS
// footprint, (rows * cols + rows) doubles: the tableau, compact, and the staged factor column.
enum BatchForm : int { kFormW = 0, kFormG = 1, kFormH = 2, kNumForms = 3 };

// Every workgroup keeps kBatchWgScratch bytes of LDS for itself (the reduction slots).
constexpr size_t kBatchWgScratch = (size_t)1 << 10;
// W: one wave per LP, four LPs per 256-lane workgroup, each in a quarter of the 64 KiB a
// workgroup gets without the dynamic-LDS attribute.
constexpr size_t kBatchWgLdsW = (size_t)64 << 10;
constexpr size_t kBatchMaxLdsW = (kBatchWgLdsW - kBatchWgScratch) / 4;
// G: one workgroup per LP, the tableau in dynamic LDS: 160 KiB less the workgroup's scratch.
constexpr size_t kBatchMaxLdsG = ((size_t)160 << 10) - kBatchWgScratch;
// H: one workgroup per LP, the tableau in its slice of the global slab; factor column and pivot
// row staged in LDS.  The limit of DESIGN.md section 4c.
constexpr int kBatchMaxRowsH = 1024;
constexpr int kBatchMaxColsH = 2048;
// Pivots per LP per launch, by form: a launch stays within a few milliseconds, and no launch runs
// without a bound, even on an LP that cycles.
constexpr int kBatchChunk[kNumForms] = {256, 128, 16};
// Pivot-log pairs kept per LP when the caller passes log_cap = 0: 4 * (rows + cols), at most 4096.
constexpr int kBatchLogDefaultMax = 4096;

// One LP of a batch, in device memory.  The host owns the offsets; the kernels update status,
// iter and log_fill at the end of every launch.
struct BatchDesc {
    int64_t t_off;     // tableau: rows x cols row-major, compact, at slab + t_off (doubles)
    int64_t b_off;     // basis: rows - 1 entries at basis + b_off
    int64_t log_off;   // pivot log: log_cap (row, col) pairs at log + 2 * log_off
    int64_t x_off;     // solution: n entries at x + x_off (lpr_batch_solution_read)
    int64_t iter;      // pivots performed so far (exact; the log keeps the first log_cap)
    int64_t max_iter;  // this call stops when iter reaches it (<= 0: no limit)
    int32_t rows, cols;
    int32_t n;         // decision variables (columns 0 .. n-1 of ExtractSolution)
    int32_t log_cap;
    int32_t status;    // kRunning or an lpr_status
    int32_t log_fill;  // pairs kept: min(iter, log_cap)
};

// Inputs of lpr_batch_from_lps per LP: offsets into the packed arrays.
struct BatchBuild {
    int64_t obj_off;  // objective: n entries
    int64_t a_off;    // A: m x n row-major
    int64_t row_off;  // ncoef, relation, rhs: m entries
};

inline size_t batch_footprint(int rows, int cols) {  // doubles of LDS one LP needs
    return (size_t)rows * cols + rows;
}

}  // namespace lpr
