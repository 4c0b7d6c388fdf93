// sens_ranging_common.hpp -- the tile geometry and the workspace layout of the sensitivity report
// (lpr_sens_ranging), shared by sens_engine.hip (host side),
// sens_ranging_kernels.hip and tools/ranging_plan_check.cpp (a stand-alone host program that walks
// every index the kernels form against the sizes computed here).  Plain C++: no HIP header, so the
// checker builds with any host compiler.  Not part of the ABI (include/lpr_engine.h is).
#pragma once

#include <cstddef>
#include <cstdint>

namespace lpr {

// One sweep tile: kRngTileRows tableau rows x kRngTileCols columns, one 256-lane workgroup; lane l
// owns the column pair (2l, 2l + 1) of the tile, so lane order is column order.  The rows of a tile
// are taken kRngSubRows at a time (one LDS transposition each).
constexpr int kRngLanes = 256;
constexpr int kRngTileCols = 2 * kRngLanes;
constexpr int kRngTileRows = 32;
constexpr int kRngSubRows = 8;
// LDS row of lane partials: lane l sits at l + l / 8 (one pad per 8 lanes: the 32 threads that
// each fold 8 consecutive lanes start 9 doubles apart, on 32 distinct bank pairs), one more
// double so that two rows do not start on the same bank.
constexpr int kRngLdsStride = kRngLanes + kRngLanes / 8 + 1;
static_assert(kRngTileRows % kRngSubRows == 0, "whole sub-passes per tile");
static_assert(kRngSubRows * 32 == kRngLanes, "phase 2: 32 threads per row of a sub-pass");

// A partial is (lo, hi), 16 bytes.  All offsets below are in bytes from the start of one device
// buffer; the output block [out_off, total) is what the single read-back copies.
struct SensRangingPlan {
    int m, n, nc;          // constraints, decision columns, columns without the RHS
    int ntr, ntc;          // tile rows over rows 1..m, tile columns over columns 0..nc-1
    size_t rowpart_off;    // m x ntc partials: [row - 1][tile column]
    size_t colpart_off;    // ntr x m partials: [tile row][slack column - n]
    size_t out_off;        // start of the output block (16-byte aligned)
    size_t o_rc, o_clo, o_chi;             // nc doubles each
    size_t o_shadow, o_rlo, o_rhi, o_now;  // m doubles each
    size_t o_kind, o_row;                  // nc int32 each
    size_t total;          // bytes of the buffer
};

// false: the shape has no report (rows < 2, or n = cols - rows < 0: the C# would index
// tableau[0, n + k - 1] out of range for small k)
inline bool sens_ranging_plan(int R, int C, SensRangingPlan* p) {
    if (R < 2 || C < 2 || C < R) return false;
    p->m = R - 1;
    p->nc = C - 1;
    p->n = C - R;
    p->ntr = (p->m + kRngTileRows - 1) / kRngTileRows;
    p->ntc = (p->nc + kRngTileCols - 1) / kRngTileCols;
    const size_t P = 2 * sizeof(double), D = sizeof(double), I = sizeof(int32_t);
    const size_t m = (size_t)p->m, nc = (size_t)p->nc;
    size_t off = 0;
    p->rowpart_off = off; off += m * (size_t)p->ntc * P;
    p->colpart_off = off; off += (size_t)p->ntr * m * P;
    p->out_off = off;
    p->o_rc = off;     off += nc * D;
    p->o_clo = off;    off += nc * D;
    p->o_chi = off;    off += nc * D;
    p->o_shadow = off; off += m * D;
    p->o_rlo = off;    off += m * D;
    p->o_rhi = off;    off += m * D;
    p->o_now = off;    off += m * D;
    p->o_kind = off;   off += nc * I;
    p->o_row = off;    off += nc * I;
    p->total = (off + 15) & ~(size_t)15;
    return true;
}

}  // namespace lpr
