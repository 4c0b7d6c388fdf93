// sens_batch_ranging_common.hpp -- the lane mapping, the LDS carve-up and the output layout of the
// scenario batch's sensitivity report (lpr_sens_batch_ranging), shared by
// sens_batch_engine.hip (host side), sens_batch_ranging_kernels.hip and
// tools/sens_batch_ranging_check.cpp (a stand-alone host program that walks every index the kernel
// forms against the sizes computed here).  Plain C++: no HIP header, so the checker builds with
// any host compiler.  Not part of the ABI (include/lpr_engine.h is).
#pragma once

#include "sens_ranging_common.hpp"  // the output block: SensReportLayout, SensReportOut

namespace lpr {

// One 256-lane workgroup per scenario.
//   column pass: lane l owns the columns l, l + kSbrLanes, ... and walks each down rows 1..R-1
//                ascending (the scan order of :406-418 and :69-84: no fold is cut);
//   row pass:    wave w owns the rows 1 + w, 1 + w + kSbrWaves, ...; lane l of the wave owns the
//                columns l, l + kSbrWaveLanes, ... of the row (coalesced loads), so the fold of a
//                row is cut by STRIDED ownership and carries (value, column).
constexpr int kSbrLanes = 256;
constexpr int kSbrWaveLanes = 64;
constexpr int kSbrWaves = kSbrLanes / kSbrWaveLanes;
static_assert(kSbrWaves * kSbrWaveLanes == kSbrLanes, "whole waves");

// Dynamic LDS of the workgroup, sized by the batch's maximal shape SR x SC (the scenario indexes it
// by its own R x C <= SR x SC).  Offsets in bytes; at the batch limit of 1024 x 2048 the total is
// 36 KiB, so they fit an int (and a kernel argument of six of them stays small).
struct SensBatchRangingLds {
    int b_off;     // SR doubles: the RHS column, b[i] = T[i][C - 1]
    int lo_off;    // SR doubles: the row fold's deltaLower of row i
    int hi_off;    // SR doubles: ... deltaUpper
    int cand_off;  // SC int32: GetBasicRow(j) of a column of basicVars, else -1
    int need_off;  // SR int32: some column of basicVars has row i as its basic row
    int total;
};
inline SensBatchRangingLds sens_batch_ranging_lds(int SR, int SC) {
    SensBatchRangingLds l;
    const int D = (int)sizeof(double), I = (int)sizeof(int32_t);
    int off = 0;
    l.b_off = off;    off += SR * D;
    l.lo_off = off;   off += SR * D;
    l.hi_off = off;   off += SR * D;
    l.cand_off = off; off += SC * I;
    l.need_off = off; off += SR * I;
    l.total = (off + 7) & ~7;
    return l;
}

// The output block is the whole device buffer (and its pinned mirror): scenario k at row k of each
// array, rows of max_cols - 1 and max_rows - 1.
struct SensBatchRangingPlan {
    int count;
    int mc, mr;            // max_cols - 1, max_rows - 1: the row lengths
    SensReportLayout out;  // at offset 0
    size_t total;
};

// false: no report (no scenario, rows < 2, or n = cols - rows < 0 at the base: the C# would index
// tableau[0, n + k - 1] out of range; no edit lowers cols - rows)
inline bool sens_batch_ranging_plan(int count, int base_R, int base_C, int max_R, int max_C,
                                    SensBatchRangingPlan* p) {
    if (count < 1 || base_R < 2 || base_C < base_R || max_R < base_R || max_C < base_C)
        return false;
    p->count = count;
    p->mc = max_C - 1;
    p->mr = max_R - 1;
    p->out = sens_report_layout(count, p->mc, p->mr, 0);
    p->total = p->out.end;
    return true;
}

}  // namespace lpr
