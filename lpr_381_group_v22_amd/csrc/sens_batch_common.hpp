// sens_batch_common.hpp -- definitions shared by the sensitivity scenario batch (DESIGN.md section
// 14): sens_batch_engine.hip (host) and sens_batch_kernels.hip.  Not part of the ABI
// (include/lpr_engine.h is).
#pragma once

#include "batch_common.hpp"
#include "sens_batch_ranging_common.hpp"

#pragma clang fp contract(off)

namespace lpr {

// Forms of a scenario batch.  One call runs one form, chosen by the batch's maximal shape: the
// base's shape, or in a grow batch (lpr_sens_batch_create_grow) the largest shape a script can
// reach.  Strides and the LDS carve-up are sized by that shape; a scenario indexes its tableau
// compactly by its own column count.  The numbers are those of BatchForm (a wave-per-scenario
// form W is not built).
//   G: the working state of a scenario lives in dynamic LDS: the tableau (rows x cols, compact),
//      the factor column (rows), the pivot row (cols), the membership counts (cols, int32) and
//      basicVars (rows - 1, int32).  Budget: kBatchMaxLdsG, 160 KiB less the workgroup's 1 KiB.
//   H: the tableau stays in the scenario's slice of the global slab, up to kBatchMaxRowsH x
//      kBatchMaxColsH; everything else of the list above is staged in LDS (at most 36 KiB).
inline size_t sens_batch_aux_bytes(int rows, int cols) {  // LDS of both forms besides the tableau
    const size_t b = (size_t)(rows + cols) * sizeof(double) +
                     (size_t)(cols + rows - 1) * sizeof(int32_t);
    return (b + 7) & ~(size_t)7;
}
inline size_t sens_batch_footprint_g(int rows, int cols) {  // bytes of dynamic LDS in form G
    return (size_t)rows * cols * sizeof(double) + sens_batch_aux_bytes(rows, cols);
}

// Pivots per scenario per launch, by form (index kFormG / kFormH), and edits begun per scenario
// per launch: no launch is unbounded, neither on a scenario that cycles nor on a script of many
// edits that never pivot.
constexpr int kSensBatchChunk[kNumForms] = {0, 128, 16};
static_assert(sizeof(kSensBatchChunk) / sizeof(int) == kNumForms, "one chunk per form");
constexpr int kSensBatchEditsPerLaunch = 64;

constexpr int32_t kSensEditNotRun = kRunning;  // outcome of an edit that has not ended yet

// Where a scenario stands inside its current edit.  A launch can stop only in front of a pivot,
// so Dual and Primal are the phases a descriptor is stored with in the middle of an edit; the
// others run through within one launch.
enum SensPhase : int32_t {
    kPhaseApply = 0,     // at the boundary: the next edit has not been applied
    kPhaseRebuild = 1,   // RebuildBasicsFromTableau (:706-723)
    kPhaseDual = 2,      // DualSimplexIfNeeded (:168-201)
    kPhasePrimal = 3,    // ReOptimize's loop (:121-157)
    kPhaseEpilogue = 4,  // ReOptimize's epilogue (:159-165)
    kPhaseRollback = 5,  // ChangeRHS's catch block (:462-469)
};

// One scenario, in device memory.  Every array of the batch is indexed by the scenario number
// times a stride of SensBatchView, so the descriptor holds only what changes.
struct SensScenario {
    double z;            // finalZ
    double old_z;        // ChangeRHS snapshot of finalZ (:438)
    int64_t edit_off;    // first edit of the script in the packed edit / outcome arrays
    int64_t pivots;      // pivots so far, all edits
    int64_t pivot_stop;  // this call stops the scenario when pivots reaches it (<= 0: no cap)
    int64_t edit_pivots; // pivots of the current edit
    int64_t log_n;       // pivot-log triples so far (exact; the log keeps the first log_cap)
    int32_t nedits;
    int32_t edit;        // current edit; nedits when the script has ended
    int32_t phase;       // SensPhase
    int32_t iter_dual;   // the C#'s `iter` of DualSimplexIfNeeded, restarted per edit
    int32_t iter_primal; // ... of ReOptimize
    int32_t nsol;        // solutionVector.Count
    int32_t in_alt;      // form G, stopped inside an edit: the working tableau is in the alt slice
    int32_t status;      // kRunning, LPR_OK_OPTIMAL (script ended) or LPR_PIVOT_LIMIT (resumable)
    int32_t R, C;        // the scenario's shape now (AddNewActivity / AddNewConstraint grow it)
};

// lpr_sens_batch_from_batch: the LP a scenario is constructed on, as the LP batch's descriptor
// (BatchDesc) has it.  rows <= cols, 0 <= n <= cols - 1.
struct SensModelSrc {
    int64_t t_off;  // the LP's final tableau: rows x cols row-major, compact, at slab + t_off
    int32_t rows, cols;
    int32_t n;      // decision variables: solutionVector.Count
    int32_t item;   // the LP's index in its batch
};

// What a launch needs of the batch: strides and the device arrays.
struct SensBatchView {
    int32_t R, C;        // the maximal shape of a scenario: what every stride below is sized by
    int32_t sol_cap;     // doubles per scenario in `sol`: max(base solutionVector.Count, C - 1)
    int32_t log_cap;     // triples per scenario in `log`
    SensScenario* desc;
    double* cur;         // count slices of R * C: the state as of the last edit (H: the live one)
    double* alt;         // count slices of R * C: G: the state inside an edit; H: the snapshot
    int32_t* basic;      // count x (R - 1)
    int32_t* bcount;     // count x C: positions of basicVars that hold column j
    int32_t* snap;       // count x (R - 1 + C): ChangeRHS snapshot of basic and bcount
    double* sol;         // count x sol_cap
    int32_t* log;        // count x 3 * log_cap
    const lpr_sens_edit* edits;
    const double* payload;  // grow batch: the columns and rows the add edits point into
    int32_t* outcome;    // per edit, packed
    int64_t* edit_piv;   // per edit, packed
};

// Launchers, for sens_batch_engine.hip.  sens_batch_kernels.hip: the base state into every
// scenario; the analyzer's constructor per scenario on the LPs `src` names in `slab`; one bounded
// round of the script kernel in `form` over the scenarios idx_in lists.
int sens_batch_launch_init(hipStream_t s, const SensBatchView& vw, int count, int R, int C,
                           const double* baseT, int ld, const int32_t* base_basic,
                           const int32_t* base_bcount, const double* base_sol, int nsol);
int sens_batch_launch_from_models(hipStream_t s, const SensBatchView& vw, int count,
                                  const SensModelSrc* src, const double* slab);
int sens_batch_launch(int form, bool grow, hipStream_t s, const SensBatchView& vw,
                      const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out,
                      int chunk);
// sens_batch_ranging_kernels.hip: the report of every scenario into `out`, laid out by `pl`
int sens_batch_ranging_launch(hipStream_t s, const SensBatchView& vw, char* out,
                              const SensBatchRangingPlan& pl);

}  // namespace lpr
