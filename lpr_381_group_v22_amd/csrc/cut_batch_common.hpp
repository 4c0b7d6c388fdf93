// cut_batch_common.hpp -- definitions shared by the batched cutting plane (DESIGN.md sections 15
// and 24): cut_batch_engine.hip (host), cut_batch_body.hpp (the one text of the state machine) and
// its two instantiations, cut_batch_kernels.hip and cut_batch_narr_kernels.hip (the narrated
// twins, which also keep what cut_narr_layout.hpp lays out).  Not part of the ABI
// (include/lpr_engine.h is).
#pragma once

#include "batch_common.hpp"
#include "cut_common.hpp"
#include "cut_narr_layout.hpp"

namespace lpr {

// Forms of one item, picked per item (mixed in one call) by batch_pick_form on the footprint at
// FULL row capacity, rcap = rows at create + max_cuts: a cut appends a row to the compact
// tableau, so an item that fits a form at capacity fits it after every cut.  The numbers are
// those of BatchForm (a wave-per-item form W is not built).
//   G: the tableau (rcap x cols, compact), the factor column (rcap) and the pivot row (cols) in
//      dynamic LDS; written back to the item's slice when a launch ends.
//   H: the tableau stays in the item's slice of the global slab; the two vectors in LDS.
inline size_t cut_batch_aux_bytes(int rcap, int cols) {  // LDS of both forms besides the tableau
    return (size_t)(rcap + cols) * sizeof(double);
}
inline size_t cut_batch_footprint_g(int rcap, int cols) {  // bytes of dynamic LDS in form G
    return (size_t)rcap * cols * sizeof(double) + cut_batch_aux_bytes(rcap, cols);
}

// Pivots per item per launch, by form (index kFormG / kFormH); the cut's pivot and the pivots of
// both clean-up solvers count alike.  No launch is unbounded.
constexpr int kCutBatchChunk[kNumForms] = {0, 128, 16};
static_assert(sizeof(kCutBatchChunk) / sizeof(int) == kNumForms, "one chunk per form");

constexpr int kCutBatchDefaultMaxCuts = 64;  // max_cuts <= 0, as lpr_cutting_plane
constexpr int kCutBatchInnerIters = 10000;   // maxIters of :190 / :200

enum CutBatchMode : int32_t { kCutModeCuttingPlane = 0, kCutModeDual = 1, kCutModePrimal2 = 2 };

// Where an item stands.  A launch can stop only in front of a pivot: an item that is still
// running is stored in CutPivot, Dual or Primal2 and selects that pivot again when it resumes.
enum CutBatchPhase : int32_t {
    kCutPhaseAdd = 0,       // steps 1-5 (:76-110): source row, the cut appended
    kCutPhaseCutPivot = 1,  // steps 6-7 (:113-176): pivot column on the cut row, the pivot
    kCutPhaseDual = 2,      // DualSimplexSolver.Solve (DualSimplex.cs:14-114)
    kCutPhasePrimal2 = 3,   // PrimalSimplexSolver2.Solve (PrimalSimplexSolver2.cs:46-97)
    kCutPhaseClosing = 4,   // step 9 (:215-228): the three flag scans
};

// One item, in device memory.  The host owns the offsets and the per-call fields; a launch
// updates the rest when it ends.
struct CutBatchDesc {
    int64_t t_off;     // tableau slice: rcap x cols doubles at slab + t_off, rows x cols in use
    int64_t log_off;   // log: log_cap triples at log + 3 * log_off
    int64_t log_n;     // triples so far, over the handle's life (exact; the first log_cap kept)
    int64_t iter;      // the C#'s `iter` of the inner solve that is running
    int64_t done;      // pivots of the inner solve that is running (what hard_cap counts)
    int64_t pivots;    // pivots of this call, all three kinds
    double z;          // T[0, cols - 1] as of the last launch
    int32_t rows, cols;
    int32_t rcap;      // rows at create + max_cuts
    int32_t log_cap;
    int32_t phase;     // CutBatchPhase
    int32_t cuts;      // cuts of this call
    int32_t cut_limit; // this call may add so many: min(opts.max_cuts, rcap - rows at its start)
    int32_t code;      // kRunning, or the exit code (mode 0) / lpr_status (modes 1, 2)
};

// What every item of one call shares.
struct CutBatchCall {
    int32_t mode;         // CutBatchMode
    int32_t print_steps;  // modes 1, 2 (mode 0: 1)
    int64_t max_iters;    // modes 1, 2 (mode 0: kCutBatchInnerIters)
    int64_t hard_cap;     // per inner solve, <= 0: none
    int32_t chunk;
};

// The narration buffers of a narrated handle (cut_narr_layout.hpp); all null otherwise.
struct CutNarr {
    CutNarrDesc* desc = nullptr;  // count cursors
    int32_t* ev = nullptr;        // events: four int32 each, packed by ev_cap
    double* data = nullptr;       // the data slab: cap doubles per item
};

// cut_batch_kernels.hip: the launchers cut_batch_engine.hip calls
int cut_batch_launch(int form, hipStream_t s, CutBatchDesc* desc, double* slab, int32_t* logs,
                     const CutBatchCall& call, size_t lds, const int32_t* idx_in, int n_in,
                     int32_t* idx_out, int32_t* n_out);
int cut_batch_launch_load(hipStream_t s, CutBatchDesc* desc, int count, const double* src,
                          const int64_t* src_off, double* slab);
// cut_batch_narr_kernels.hip
int cut_batch_narr_launch(int form, hipStream_t s, CutBatchDesc* desc, double* slab,
                          int32_t* logs, const CutBatchCall& call, const CutNarr& narr, size_t lds,
                          const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out);
int cut_batch_narr_launch_first(hipStream_t s, const CutBatchDesc* desc, const double* slab,
                                const CutNarr& narr, int count);
int cut_batch_narr_launch_call(hipStream_t s, const CutBatchDesc* desc, const CutNarr& narr,
                               int count, int mode, int print_steps);

}  // namespace lpr
