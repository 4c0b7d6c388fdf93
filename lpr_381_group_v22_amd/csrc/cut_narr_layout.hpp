// cut_narr_layout.hpp -- what a narrated cutting-plane batch keeps per
// item; the cursor rule that places the data blocks is kept_prefix.hpp's.  Needs no HIP: the
// kernels (cut_batch_body.hpp), the engine (cut_batch_engine.hip) and the host-only walker
// tools/cut_narr_check.cpp include this one text.  Restated for the host mirror at the head of
// cut_batch.py.
//
// Per item k, all addressed through CutNarrDesc k, appended over the handle's life as the log is:
//   events   ev[4 * (ev_off + i) ...]: event i as four int32 (kind, a, b, rows_now).  ev_n is
//            exact; the first ev_cap are kept.
//            kind             a                      b                       pushed
//            kCutEvCall       mode                   print_steps             start of every run
//            kCutEvLevel      0                      0                       entry of kCutPhaseAdd
//            kCutEvCut        source row (0-based    0                       the cut appended
//                             constraint index)
//            kCutEvSolveBegin 0 dual / 1 primal2     0                       the phase change
//            kCutEvSolveEnd   lpr_status             1: the hard_cap stop    the inner solve returns
//            kCutEvExit       code                   column (exit 3 only)    the item ends
//            kCutEvPivot + q  row                    column                  the pivot; q the log
//                             (as in the log triple)                         kind 0 / 1 / 2
//            rows_now is the item's row count when the event is pushed (the cut's row included).
//   data     data[data_off ...]: blocks of doubles, compact and back to back, in event order.
//            Block 0 is the rows x cols tableau at reserve time; every kCutEvCut adds the appended
//            row (cols doubles), every pivot event the whole tableau after it (rows_now x cols).
//            cut_narr_event_doubles is that rule; offsets are its prefix sum.
// Capacity: `cap` doubles of data, kept by the rule of kept_prefix.hpp.
#pragma once

#include "kept_prefix.hpp"

namespace lpr {

enum CutNarrEvent : int32_t {
    kCutEvCall = 0,
    kCutEvLevel = 1,
    kCutEvCut = 2,
    kCutEvSolveBegin = 3,
    kCutEvSolveEnd = 4,
    kCutEvExit = 5,
    kCutEvPivot = 8,  // + the log kind: 8 dual, 9 primal2, 10 cut
};

// The cursors of one item; they live here between launches and calls.
struct CutNarrDesc {
    int64_t ev_off;    // quads: this item's ev_cap events start at ev + 4 * ev_off
    int64_t ev_n;      // events made (exact); the first ev_cap kept
    int64_t data_off;  // doubles: this item's slice of the data slab
    KeptPrefix kp;     // the blocks in the slice
    int32_t ev_cap;
    int32_t pad;
};
static_assert(sizeof(CutNarrDesc) == 72, "CutNarrDesc is 72 bytes");

// Doubles of the block an event adds to the data.
constexpr int64_t cut_narr_event_doubles(int32_t kind, int32_t rows_now, int32_t cols) {
    return kind == kCutEvCut ? (int64_t)cols
                             : (kind >= kCutEvPivot ? (int64_t)rows_now * cols : (int64_t)0);
}

// One more event.  Returns its index among the kept ones, or -1 where it is only counted.
LPR_HD int64_t cut_narr_event(CutNarrDesc& c) {
    const int64_t at = c.ev_n < (int64_t)c.ev_cap ? c.ev_n : -1;
    ++c.ev_n;
    return at;
}

}  // namespace lpr
