// bb_narr_layout.hpp -- what a narrated B&B batch keeps per IP, and the
// cursor rules that place it.  Needs no HIP: the search kernels (bb_batch_body.hpp), the engine
// (bb_batch_engine.hip) and the host-only walker tools/bb_narr_check.cpp include this one text.
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
// Capacity: `cap` doubles of child tableaux.  A tableau that does not fit whole is counted and not
// written, and so is every later one: what is kept is a prefix, and made_t / made_d stay exact.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LPR_NARR_HD __host__ __device__ inline
#else
#define LPR_NARR_HD inline
#endif

namespace lpr {

enum : int32_t { kNarrScored = 1, kNarrInteger = 2, kNarrIncumbent = 4 };

// The cursors of one IP; they live here between launches.  k_bb_batch_narr_reset rewinds them.
struct BBNarrDesc {
    int64_t slab_off;  // doubles: this IP's slice of the slab
    int64_t cap;       // doubles reserved for it
    int64_t best_off;  // doubles: its incumbent buffer of slot_n doubles
    int64_t cur;       // doubles kept so far: the next kept tableau starts here
    int64_t made_d;    // doubles made (exact)
    int64_t made_t;    // tableaux made (exact)
    int64_t kept_t;    // tableaux kept: the first kept_t of the made ones
    int32_t best_depth;  // depth of the incumbent's node, -1 if none
    int32_t pad;
};

// One more tableau of n doubles.  Returns where it goes in the slice, or -1 where it is only
// counted: it does not fit, or an earlier one was not kept.
LPR_NARR_HD int64_t narr_push(BBNarrDesc& c, int64_t n) {
    const bool keep = c.kept_t == c.made_t && n <= c.cap - c.cur;
    const int64_t at = keep ? c.cur : -1;
    ++c.made_t;
    c.made_d += n;
    if (keep) {
        ++c.kept_t;
        c.cur += n;
    }
    return at;
}

// The last tableau made, of n doubles, is dropped (:392-400): the cursor steps back by it where
// it was kept.
LPR_NARR_HD void narr_drop(BBNarrDesc& c, int64_t n) {
    if (c.kept_t == c.made_t) {
        --c.kept_t;
        c.cur -= n;
    }
    --c.made_t;
    c.made_d -= n;
}

LPR_NARR_HD void narr_rewind(BBNarrDesc& c) {
    c.cur = c.made_d = c.made_t = c.kept_t = 0;
    c.best_depth = -1;
}

}  // namespace lpr
