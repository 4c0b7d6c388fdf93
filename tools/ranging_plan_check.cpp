// ranging_plan_check.cpp -- host-only check of the sensitivity report's workspace layout and tile
// geometry (csrc/sens_ranging_common.hpp).  It walks every index that
// k_sens_ranging_sweep and k_sens_ranging_finish form -- tableau loads, LDS slots, slab cells,
// output cells -- over exactly-sized heap buffers, so that an address sanitizer sees any index past
// a size the plan computed, and checks that every slab cell is written exactly once.  No GPU, no
// HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/ranging_plan_check.cpp -o /tmp/ranging_plan_check && /tmp/ranging_plan_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../lpr_381_group_v22_amd/csrc/sens_ranging_common.hpp"

using namespace lpr;

static int fail(const char* what, int R, int C) {
    std::fprintf(stderr, "ranging_plan_check: %s at %d x %d\n", what, R, C);
    return 1;
}

static int check_shape(int R, int C) {
    SensRangingPlan pl;
    const bool ok = sens_ranging_plan(R, C, &pl);
    if (R < 2 || C < 2 || C < R) return ok ? fail("a shape without a report was planned", R, C) : 0;
    if (!ok) return fail("a valid shape was refused", R, C);
    const int ld = (C + 15) / 16 * 16, ld2 = ld / 2;
    const int m = pl.m, nc = pl.nc, n = pl.n;
    if (m != R - 1 || nc != C - 1 || n != C - R || n + m != nc) return fail("m / n / nc", R, C);
    const SensReportLayout& o = pl.out;
    if (pl.rowpart_off % 16 || pl.colpart_off % 16 || o.base % 16 || o.o_rc % 8 ||
        o.o_now % 8 || o.o_kind % 4 || o.o_row % 4 || pl.total % 16)
        return fail("alignment", R, C);
    if (o.count != 1 || o.mc != nc || o.mr != m || o.end != pl.total)
        return fail("the output block is not one item of nc and m behind the slabs", R, C);
    if (o.o_row + (size_t)nc * 4 > pl.total)
        return fail("the output block passes the total", R, C);

    std::unique_ptr<double[]> T(new double[(size_t)R * ld]);
    std::unique_ptr<unsigned char[]> ws(new unsigned char[pl.total]);
    std::unique_ptr<double[]> lds(new double[(size_t)kRngSubRows * kRngLdsStride]);
    std::memset(T.get(), 0, (size_t)R * ld * sizeof(double));
    std::memset(ws.get(), 0, pl.total);
    // one byte per slab cell counts the writes
    auto rowcell = [&](size_t k) -> unsigned char& { return ws[pl.rowpart_off + k * 16]; };
    auto colcell = [&](size_t k) -> unsigned char& { return ws[pl.colpart_off + k * 16]; };
    double sink = 0.0;
    for (int tr = 0; tr < pl.ntr; ++tr)
        for (int tc = 0; tc < pl.ntc; ++tc) {
            const bool slack_tile = tc * kRngTileCols + kRngTileCols > n && tc * kRngTileCols < nc;
            for (int sp = 0; sp < kRngTileRows / kRngSubRows; ++sp) {
                const int i0 = 1 + tr * kRngTileRows + sp * kRngSubRows;
                if (i0 >= R) break;
                for (int tid = 0; tid < kRngLanes; ++tid) {
                    const int c2 = tc * kRngLanes + tid;
                    for (int k = 0; k < kRngSubRows; ++k) {
                        const int i = i0 + k;
                        if (i < R && c2 < ld2) sink += T[((size_t)i * ld2 + c2) * 2 + 1];
                        if (slack_tile && i < R) sink += T[(size_t)i * ld + nc];
                        lds[k * kRngLdsStride + tid + (tid >> 3)] = 1.0;
                    }
                }
                for (int tid = 0; tid < kRngLanes; ++tid) {
                    const int r = tid >> 5, seg = tid & 31;
                    for (int q = 0; q < 8; ++q) sink += lds[r * kRngLdsStride + seg * 9 + q];
                    const int i = i0 + r;
                    if (seg == 0 && i < R) rowcell((size_t)(i - 1) * pl.ntc + tc) += 1;
                }
            }
            if (slack_tile)
                for (int tid = 0; tid < kRngLanes; ++tid)
                    for (int e = 0; e < 2; ++e) {
                        const int j = 2 * (tc * kRngLanes + tid) + e;
                        if (j < nc && j >= n) colcell((size_t)tr * m + (j - n)) += 1;
                    }
        }
    for (size_t k = 0; k < (size_t)m * pl.ntc; ++k)
        if (rowcell(k) != 1) return fail("a row-slab cell is not written exactly once", R, C);
    for (size_t k = 0; k < (size_t)pl.ntr * m; ++k)
        if (colcell(k) != 1) return fail("a column-slab cell is not written exactly once", R, C);
    // the finish kernel's reads and writes
    for (int t = 0; t < (nc > m ? nc : m); ++t) {
        if (t < nc) {
            sink += T[t];
            for (int vr = 1; vr <= m; vr += (m > 8 ? m - 1 : 1))  // first and last basic row
                for (int q = 0; q < pl.ntc; ++q) sink += rowcell((size_t)(vr - 1) * pl.ntc + q);
            ws[o.o_rc + (size_t)t * 8] = ws[o.o_clo + (size_t)t * 8] = 1;
            ws[o.o_chi + (size_t)t * 8 + 7] = ws[o.o_kind + (size_t)t * 4 + 3] = 1;
            ws[o.o_row + (size_t)t * 4 + 3] = 1;
        }
        if (t < m) {
            for (int q = 0; q < pl.ntr; ++q) sink += colcell((size_t)q * m + t);
            sink += T[n + t] + T[(size_t)(t + 1) * ld + nc];
            ws[o.o_shadow + (size_t)t * 8 + 7] = ws[o.o_rlo + (size_t)t * 8 + 7] = 1;
            ws[o.o_rhi + (size_t)t * 8 + 7] = ws[o.o_now + (size_t)t * 8 + 7] = 1;
        }
    }
    return sink < 0.0;  // never: keeps the reads alive
}

int main() {
    int bad = 0, shapes = 0;
    for (int R = 0; R <= 70; ++R)
        for (int C = 0; C <= R + 40; ++C, ++shapes) bad += check_shape(R, C);
    const int wide[] = {511, 512, 513, 514, 1023, 1024, 1025, 1537, 2100};
    const int tall[] = {2, 9, 32, 33, 34, 65, 200};
    for (int R : tall)
        for (int C : wide)
            if (C >= R) {
                bad += check_shape(R, C);
                ++shapes;
            }
    bad += check_shape(1030, 2100);
    bad += check_shape(4097, 12289);
    shapes += 2;
    std::printf("ranging_plan_check: %d shapes, %d failures\n", shapes, bad);
    return bad ? 1 : 0;
}
