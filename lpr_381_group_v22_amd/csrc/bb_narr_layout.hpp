// bb_narr_layout.hpp -- what a narrated B&B batch keeps per IP; the cursor
// rule that places the child tableaux is kept_prefix.hpp's.  Needs no HIP: the search kernels
// (bb_batch_body.hpp), the engine (bb_batch_engine.hip) and the host-only walker
// tools/bb_narr_check.cpp include this one text.
// Restated for the host mirror at the head of bb_batch.py.
//
// Per IP k, all addressed through BBNarrDesc k:
//   child tableaux  slab[slab_off + tab_off[rid] ...]: for the child with record id rid the list
//                   DoDualSimplex returns (BranchBoundSimplexSolver.cs:292, :341, :388) -- the
//                   tableau AddConstraint hands it, then one per pivot -- each (R0 + depth) x
//                   (C0 + depth) doubles, row-major, unrounded, back to back.  tab_off[rid] (int64,
//                   doubles from the IP's slice start) and ntab[rid] (int32, tableaux MADE, after
//                   the drop of :392-400) go with record rid; the root has ntab = 0.
//   pops            per position i in the pop order: pop_z[i] = objVal, pop_vals[i * nvars ..] the
//                   decision values, pop_flags[i] (kNarrScored | kNarrInteger | kNarrIncumbent);
//                   a pruned pop keeps objVal and flags 0.
//   incumbent       best[best_off ...]: the popped node, rounded by :1047, that
//                   UpdateOptimalSolution (:935-983) took last; (R0 + best_depth) x
//                   (C0 + best_depth).
// Capacity: `cap` doubles of child tableaux, kept by the rule of kept_prefix.hpp: a tableau is a
// block of its cursor.
#pragma once

#include "kept_prefix.hpp"

namespace lpr {

enum : int32_t { kNarrScored = 1, kNarrInteger = 2, kNarrIncumbent = 4 };

// The cursors of one IP; they live here between launches.  k_bb_batch_narr_reset rewinds them.
struct BBNarrDesc {
    int64_t slab_off;  // doubles: this IP's slice of the slab
    int64_t best_off;  // doubles: its incumbent buffer of slot_n doubles
    KeptPrefix kp;     // the child tableaux in the slice; the drop of :392-400 is kept_drop
    int32_t best_depth;  // depth of the incumbent's node, -1 if none
    int32_t pad;
};
static_assert(sizeof(BBNarrDesc) == 64, "BBNarrDesc is 64 bytes");

LPR_HD void narr_rewind(BBNarrDesc& c) {
    kept_rewind(c.kp);
    c.best_depth = -1;
}

}  // namespace lpr
