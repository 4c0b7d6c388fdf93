// kept_prefix.hpp -- the one cursor of every narrated batch engine (B&B: bb_narr_layout.hpp,
// DESIGN.md section 23; cutting plane: cut_narr_layout.hpp, section 24) and the one statement of
// its rule.  An item has a slice of `cap` doubles and appends blocks of doubles to it, back to
// back.  A block that does not fit whole is counted and not written, and so is every later one:
// what is kept is a prefix of what was made, and made_n / made_d stay exact, so a caller that
// finds less kept than made knows the exact capacity to reserve.  Needs no HIP: the kernels, the
// engines and the host-only walkers under tools/ include this one text.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LPR_HD __host__ __device__ inline
#else
#define LPR_HD inline
#endif

namespace lpr {

struct KeptPrefix {
    int64_t cap;     // doubles reserved for the item (the host's; no kernel writes it)
    int64_t cur;     // doubles kept so far: the next kept block starts here
    int64_t made_d;  // doubles made (exact)
    int64_t made_n;  // blocks made (exact)
    int64_t kept_n;  // blocks kept: the first kept_n of the made ones
};
static_assert(sizeof(KeptPrefix) == 40, "KeptPrefix is five int64");

// One more block of n doubles.  Returns where it goes in the slice, or -1 where it is only
// counted: it does not fit, or an earlier one was not kept.
LPR_HD int64_t kept_push(KeptPrefix& c, int64_t n) {
    const bool keep = c.kept_n == c.made_n && n <= c.cap - c.cur;
    const int64_t at = keep ? c.cur : -1;
    ++c.made_n;
    c.made_d += n;
    if (keep) {
        ++c.kept_n;
        c.cur += n;
    }
    return at;
}

// The last block made, of n doubles, is taken back: the cursor steps back by it where it was kept.
LPR_HD void kept_drop(KeptPrefix& c, int64_t n) {
    if (c.kept_n == c.made_n) {
        --c.kept_n;
        c.cur -= n;
    }
    --c.made_n;
    c.made_d -= n;
}

// Nothing made, nothing kept; the capacity stays.
LPR_HD void kept_rewind(KeptPrefix& c) { c.cur = c.made_d = c.made_n = c.kept_n = 0; }

}  // namespace lpr
