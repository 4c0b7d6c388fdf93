// cut_common.hpp -- what the single-handle cutting-plane path (cut_kernels.hip) and its batch
// (cut_batch_kernels.hip) both state: the EPS of the three C# classes, Frac,
// the kinds of a log triple and the exit codes of CuttingPlaneSolution.  Not part of the ABI
// (include/lpr_engine.h is).
#pragma once

#include "engine_common.hpp"
#include "fold_common.hpp"

#pragma clang fp contract(off)

namespace lpr {

constexpr double kCutEps = 1e-9;  // DualSimplex.cs:8, PrimalSimplexSolver2.cs, CuttingPlaneSolver.cs:10
static_assert(kCutEps == kFoldEps, "eps_fold / staged_eps_fold replay the cut path's EPS band");

// Kinds of a log triple (kind, row in the C#'s own numbering, column); the first two are also the
// solver a loop head belongs to.
enum : int { kCutDual = 0, kCutPrimal2 = 1, kCutKindCut = 2 };

// Which `return` of CuttingPlaneSolution (CuttingPlaneSolver.cs:64-229) was taken.
enum CutExit : int {
    kCutExitOptimal = 0,      // "Displayed the Optimal Tableau" :224
    kCutExitIntegral = 1,     // all RHS integral, no cut needed :87-91
    kCutExitNoColumn = 2,     // no valid pivot column on the cut :134-138
    kCutExitSmallPivot = 3,   // pivot too small :146-150
    kCutExitDualFailed = 4,   // dual simplex failed :191
    kCutExitStepDone = 5,     // "Cutting-plane step finished" :228
    kCutExitMaxCuts = 6,      // max_cuts reached (no C# counterpart)
    kCutExitException = 7,    // an InvalidOperationException escaped a solver
    kNumCutExits = 8,
};

#if defined(__HIPCC__)
__device__ __forceinline__ double cut_frac(double a) {  // CuttingPlaneSolver.cs:12-17
    const double f = a - floor(a);
    if (fabs(f) < kCutEps || fabs(1 - f) < kCutEps) return 0.0;
    return f;
}
#endif

}  // namespace lpr

// cut_kernels.hip: frees the cut context of a tableau handle (release_device of lpr_engine.hip)
void lpr_cut_release(lpr_tableau* t);
