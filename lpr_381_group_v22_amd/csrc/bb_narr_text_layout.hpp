// bb_narr_text_layout.hpp -- which tableaux of a narrated B&B batch become
// blocks of its device text (lpr_bb_batch_narrate_text, section 26), stated once.  Needs no HIP:
// the engine (bb_batch_engine.hip) and the host-only walker tools/bb_narr_text_check.cpp include
// this one text.  Restated for the host in bb_batch.narration_block_index.
//
// Per IP, in record-id order: record rid has a child LP whose list DoDualSimplex returned as ntab
// tableaux of (R0 + depth) x (C0 + depth) doubles from tab_off[rid] of the IP's slice on.  What
// the slice KEEPS is a prefix of `kept` doubles (kept_prefix.hpp), so a record keeps
//     min(ntab, (kept - tab_off) / (rows * cols)), never below 0
// of its tableaux, whole ones: the rule of bb_batch._child_tableaux.  Every kept tableau is one
// block, in list order within the record -- which is the order the text shows them in.
#pragma once

#include <cstdint>

namespace lpr {

// Statuses of a child record (bb_common.hpp: solved, infeasible, failed)
constexpr int32_t kNarrTextSolved = 0;

// Math.Round(v, 4) applications format_branch_and_bound puts a child's tableau through: a solved
// child's list goes through RoundAllTableaux (:1124 / :1187) and then DisplayTableau (:623-640);
// an infeasible child's first tableau through DisplayTableau alone (a failed child shows none).
inline int32_t narr_text_child_round4(int32_t status) { return status == kNarrTextSolved ? 2 : 1; }
// The incumbent buffer is stored rounded by :1047; DisplayTableau (:1221) rounds it again.
constexpr int32_t kNarrTextIncumbentRound4 = 1;

// The kept tableaux of one record: `count` blocks of rows x cols doubles, back to back from `off`
// (doubles from the IP's slice start).
struct NarrTextRun {
    int64_t off;
    int32_t rows, cols, count, round4;
};

inline NarrTextRun narr_text_run(int32_t R0, int32_t C0, int32_t depth, int32_t status,
                                 int64_t tab_off, int32_t ntab, int64_t kept) {
    NarrTextRun r;
    r.off = tab_off;
    r.rows = R0 + depth;
    r.cols = C0 + depth;
    r.round4 = narr_text_child_round4(status);
    const int64_t each = (int64_t)r.rows * r.cols;
    int64_t have = kept > tab_off ? (kept - tab_off) / each : 0;
    if (have > ntab) have = ntab;
    r.count = (int32_t)(have > 0 ? have : 0);
    return r;
}

// One IP: runs[rid] for rid = 0 .. nrec - 1 (the root's is empty), from the per-record arrays as
// the device keeps them: depth and status `stride` ints apart.  Returns the blocks of the IP's
// children.
inline int64_t narr_text_runs(int32_t R0, int32_t C0, int64_t nrec, const int32_t* depth,
                              const int32_t* status, int stride, const int64_t* tab_off,
                              const int32_t* ntab, int64_t kept, NarrTextRun* runs) {
    int64_t blocks = 0;
    for (int64_t rid = 0; rid < nrec; ++rid) {
        runs[rid] = narr_text_run(R0, C0, depth[rid * stride], status[rid * stride], tab_off[rid],
                                  ntab[rid], kept);
        blocks += runs[rid].count;
    }
    return blocks;
}

}  // namespace lpr
