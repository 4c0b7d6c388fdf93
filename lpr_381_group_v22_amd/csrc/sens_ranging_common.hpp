// sens_ranging_common.hpp -- the tile geometry and the workspace layout of the sensitivity report
// (lpr_sens_ranging), shared by sens_engine.hip (host side),
// sens_ranging_kernels.hip and tools/ranging_plan_check.cpp (a stand-alone host program that walks
// every index the kernels form against the sizes computed here); and the output block of nine
// arrays that this report and the scenario batch's (sens_batch_ranging_common.hpp, section 19)
// both write.  Plain C++: no HIP header, so the checkers build with any host compiler.  Not part of
// the ABI (include/lpr_engine.h is).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace lpr {

// The output block of a report: nine arrays, item k (a scenario; the one analyzer is item 0) at row
// k of each.  Offsets in bytes from the start of one device buffer, the block itself at
// [base, end); the doubles come first, so with a base aligned to 8 every array is aligned to its
// element.
struct SensReportLayout {
    int count;                             // items
    int mc, mr;                            // row lengths: per-column arrays, per-constraint arrays
    size_t base, end;                      // end is rounded up to 16
    size_t o_rc, o_clo, o_chi;             // count x mc doubles each
    size_t o_shadow, o_rlo, o_rhi, o_now;  // count x mr doubles each
    size_t o_kind, o_row;                  // count x mc int32 each
};
inline SensReportLayout sens_report_layout(int count, int mc, int mr, size_t base) {
    SensReportLayout l;
    l.count = count;
    l.mc = mc;
    l.mr = mr;
    const size_t D = sizeof(double), I = sizeof(int32_t);
    const size_t nc = (size_t)count * (size_t)mc, nr = (size_t)count * (size_t)mr;
    size_t off = base;
    l.base = off;
    l.o_rc = off;     off += nc * D;
    l.o_clo = off;    off += nc * D;
    l.o_chi = off;    off += nc * D;
    l.o_shadow = off; off += nr * D;
    l.o_rlo = off;    off += nr * D;
    l.o_rhi = off;    off += nr * D;
    l.o_now = off;    off += nr * D;
    l.o_kind = off;   off += nc * I;
    l.o_row = off;    off += nc * I;
    l.end = (off + 15) & ~(size_t)15;
    return l;
}

// The nine arrays in a buffer laid out so (buf: where the offsets count from)
struct SensReportOut {
    double *rc, *clo, *chi, *shadow, *rlo, *rhi, *now;
    int32_t *kind, *row;
};
inline SensReportOut sens_report_bind(char* buf, const SensReportLayout& l) {
    SensReportOut o;
    o.rc = reinterpret_cast<double*>(buf + l.o_rc);
    o.clo = reinterpret_cast<double*>(buf + l.o_clo);
    o.chi = reinterpret_cast<double*>(buf + l.o_chi);
    o.shadow = reinterpret_cast<double*>(buf + l.o_shadow);
    o.rlo = reinterpret_cast<double*>(buf + l.o_rlo);
    o.rhi = reinterpret_cast<double*>(buf + l.o_rhi);
    o.now = reinterpret_cast<double*>(buf + l.o_now);
    o.kind = reinterpret_cast<int32_t*>(buf + l.o_kind);
    o.row = reinterpret_cast<int32_t*>(buf + l.o_row);
    return o;
}

// The arrays a caller asked for (non-null), out of a host mirror of the block [base, end)
inline void sens_report_copy(const SensReportLayout& l, const char* mirror, int32_t* kind,
                             int32_t* var_row, double* reduced_cost, double* cost_lo,
                             double* cost_hi, double* shadow, double* rhs_lo, double* rhs_hi,
                             double* rhs_now) {
    const size_t nc = (size_t)l.count * (size_t)l.mc, nr = (size_t)l.count * (size_t)l.mr;
    auto put = [&](void* dst, size_t off, size_t bytes) {
        if (dst && bytes) std::memcpy(dst, mirror + (off - l.base), bytes);
    };
    put(kind, l.o_kind, nc * sizeof(int32_t));
    put(var_row, l.o_row, nc * sizeof(int32_t));
    put(reduced_cost, l.o_rc, nc * sizeof(double));
    put(cost_lo, l.o_clo, nc * sizeof(double));
    put(cost_hi, l.o_chi, nc * sizeof(double));
    put(shadow, l.o_shadow, nr * sizeof(double));
    put(rhs_lo, l.o_rlo, nr * sizeof(double));
    put(rhs_hi, l.o_rhi, nr * sizeof(double));
    put(rhs_now, l.o_now, nr * sizeof(double));
}

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
// buffer: the two slabs of partials, then the output block [out.base, out.end), which is what the
// single read-back copies (one item, rows of nc and m).
struct SensRangingPlan {
    int m, n, nc;          // constraints, decision columns, columns without the RHS
    int ntr, ntc;          // tile rows over rows 1..m, tile columns over columns 0..nc-1
    size_t rowpart_off;    // m x ntc partials: [row - 1][tile column]
    size_t colpart_off;    // ntr x m partials: [tile row][slack column - n]
    SensReportLayout out;  // behind the slabs (16-byte aligned)
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
    const size_t P = 2 * sizeof(double), m = (size_t)p->m;
    size_t off = 0;
    p->rowpart_off = off; off += m * (size_t)p->ntc * P;
    p->colpart_off = off; off += (size_t)p->ntr * m * P;
    p->out = sens_report_layout(1, p->nc, p->m, off);
    p->total = p->out.end;
    return true;
}

}  // namespace lpr
