// sens_batch_ranging_check.cpp -- host-only check of the LDS carve-up, the output layout and the
// lane mapping of the scenario batch's sensitivity report (csrc/sens_batch_ranging_common.hpp,
// DESIGN.md section 19).  It walks every index k_sens_batch_ranging forms -- slab loads, LDS slots,
// output cells, the padding fill included -- over exactly-sized heap buffers, so that an address
// sanitizer sees any index past a size computed there, and checks that every output cell is
// written exactly once and every (row, column) of a row fold is visited exactly once, columns
// ascending inside a lane.  No GPU, no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sens_batch_ranging_check.cpp -o /tmp/sens_batch_ranging_check && \
//       /tmp/sens_batch_ranging_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../lpr_381_group_v22_amd/csrc/sens_batch_ranging_common.hpp"

using namespace lpr;

struct Shape {
    int R, C;
};

static int fail(const char* what, int SR, int SC, int k) {
    std::fprintf(stderr, "sens_batch_ranging_check: %s (max %d x %d, scenario %d)\n", what, SR, SC,
                 k);
    return 1;
}

// One batch: a base_R x base_C base, scenarios of the given shapes (all >= the base, <= the max)
static int check_batch(int base_R, int base_C, const std::vector<Shape>& sc) {
    const int count = (int)sc.size();
    int SR = base_R, SC = base_C;
    for (const Shape& s : sc) {
        if (s.R > SR) SR = s.R;
        if (s.C > SC) SC = s.C;
    }
    SensBatchRangingPlan pl;
    const bool ok = sens_batch_ranging_plan(count, base_R, base_C, SR, SC, &pl);
    if (count < 1 || base_R < 2 || base_C < base_R)
        return ok ? fail("a batch without a report was planned", SR, SC, -1) : 0;
    if (!ok) return fail("a valid batch was refused", SR, SC, -1);
    if (pl.mc != SC - 1 || pl.mr != SR - 1) return fail("row lengths", SR, SC, -1);
    const SensReportLayout& o = pl.out;
    if (o.count != count || o.mc != pl.mc || o.mr != pl.mr || o.base != 0 || o.end != pl.total)
        return fail("the output block is not the whole buffer", SR, SC, -1);
    if (o.o_rc % 8 || o.o_clo % 8 || o.o_chi % 8 || o.o_shadow % 8 || o.o_rlo % 8 ||
        o.o_rhi % 8 || o.o_now % 8 || o.o_kind % 4 || o.o_row % 4 || pl.total % 16)
        return fail("alignment", SR, SC, -1);
    if (o.o_row + (size_t)count * pl.mc * 4 > pl.total)
        return fail("the output block passes the total", SR, SC, -1);
    const SensBatchRangingLds l = sens_batch_ranging_lds(SR, SC);
    if (l.b_off % 8 || l.lo_off % 8 || l.hi_off % 8 || l.cand_off % 4 || l.need_off % 4 ||
        l.need_off + SR * 4 > l.total || l.total > 64 * 1024)
        return fail("LDS carve-up", SR, SC, -1);

    const size_t slice = (size_t)SR * SC;
    std::unique_ptr<double[]> slab(new double[slice * count]);
    std::unique_ptr<int32_t[]> bcount(new int32_t[(size_t)count * SC]);
    std::unique_ptr<unsigned char[]> out(new unsigned char[pl.total]);
    std::unique_ptr<unsigned char[]> lds(new unsigned char[(size_t)l.total]);
    std::memset(slab.get(), 0, slice * count * sizeof(double));
    std::memset(bcount.get(), 0, (size_t)count * SC * sizeof(int32_t));
    std::memset(out.get(), 0, pl.total);
    // the first byte of an output cell counts its writes
    auto d_cell = [&](size_t off, size_t t) -> unsigned char& { return out[off + t * 8]; };
    auto i_cell = [&](size_t off, size_t t) -> unsigned char& { return out[off + t * 4]; };
    double sink = 0.0;
    for (int k = 0; k < count; ++k) {
        const int R = sc[k].R, C = sc[k].C;
        if (R < base_R || C < base_C || C - R < base_C - base_R)
            return fail("the test's own scenario shape", SR, SC, k);
        const int m = R - 1, nc = C - 1, n = C - R;
        const double* T = slab.get() + (size_t)k * slice;
        const int32_t* bc = bcount.get() + (size_t)k * SC;
        std::memset(lds.get(), 0, (size_t)l.total);
        double* s_b = reinterpret_cast<double*>(lds.get() + l.b_off);
        double* s_lo = reinterpret_cast<double*>(lds.get() + l.lo_off);
        double* s_hi = reinterpret_cast<double*>(lds.get() + l.hi_off);
        int32_t* s_cand = reinterpret_cast<int32_t*>(lds.get() + l.cand_off);
        int32_t* s_need = reinterpret_cast<int32_t*>(lds.get() + l.need_off);
        for (int tid = 0; tid < kSbrLanes; ++tid)
            for (int i = tid; i < R; i += kSbrLanes) {
                s_b[i] = T[(size_t)i * C + nc];
                s_need[i] = 0;
            }
        // 1. column pass
        std::vector<int> col_seen((size_t)nc, 0);
        for (int tid = 0; tid < kSbrLanes; ++tid)
            for (int j = tid; j < nc; j += kSbrLanes) {
                col_seen[(size_t)j] += 1;
                for (int i = 1; i < R; ++i) sink += T[(size_t)i * C + j] + s_b[i];
                const int r = 1 + (j % m);  // any row a scan could return
                sink += T[(size_t)r * C + j] + bc[j];
                s_cand[j] = r;
                s_need[r] = 1;
                if (j >= n) {
                    const size_t t = (size_t)k * pl.mr + (size_t)(j - n);
                    sink += T[j] + s_b[j - n + 1];
                    d_cell(o.o_shadow, t) += 1;
                    d_cell(o.o_rlo, t) += 1;
                    d_cell(o.o_rhi, t) += 1;
                    d_cell(o.o_now, t) += 1;
                }
            }
        for (int j = 0; j < nc; ++j)
            if (col_seen[(size_t)j] != 1) return fail("a column is not walked exactly once", SR, SC, k);
        // 2. row pass: every row by exactly one wave, every column of it by exactly one lane
        std::vector<int> row_seen((size_t)R, 0);
        for (int wave = 0; wave < kSbrWaves; ++wave)
            for (int i = 1 + wave; i < R; i += kSbrWaves) {
                row_seen[(size_t)i] += 1;
                sink += s_need[i];
                std::vector<int> seen((size_t)nc, 0);
                for (int lane = 0; lane < kSbrWaveLanes; ++lane) {
                    int last = -1;
                    for (int j = lane; j < nc; j += kSbrWaveLanes) {
                        if (j <= last) return fail("a lane's columns do not ascend", SR, SC, k);
                        last = j;
                        seen[(size_t)j] += 1;
                        sink += bc[j] + T[(size_t)i * C + j] + T[j];
                    }
                }
                for (int j = 0; j < nc; ++j)
                    if (seen[(size_t)j] != 1)
                        return fail("a row's column is not folded exactly once", SR, SC, k);
                s_lo[i] = s_hi[i] = 0.0;
            }
        for (int i = 1; i < R; ++i)
            if (row_seen[(size_t)i] != 1) return fail("a row is not owned by exactly one wave", SR, SC, k);
        // 3. outputs and padding
        for (int tid = 0; tid < kSbrLanes; ++tid) {
            for (int j = tid; j < pl.mc; j += kSbrLanes) {
                const size_t t = (size_t)k * pl.mc + (size_t)j;
                if (j < nc) {
                    const int vr = s_cand[j];
                    sink += T[j] + bc[j] + s_lo[vr] + s_hi[vr];
                }
                d_cell(o.o_rc, t) += 1;
                d_cell(o.o_clo, t) += 1;
                d_cell(o.o_chi, t) += 1;
                i_cell(o.o_kind, t) += 1;
                i_cell(o.o_row, t) += 1;
            }
            for (int i = m + tid; i < pl.mr; i += kSbrLanes) {
                const size_t t = (size_t)k * pl.mr + (size_t)i;
                d_cell(o.o_shadow, t) += 1;
                d_cell(o.o_rlo, t) += 1;
                d_cell(o.o_rhi, t) += 1;
                d_cell(o.o_now, t) += 1;
            }
        }
    }
    const size_t ncell = (size_t)count * pl.mc, nrow = (size_t)count * pl.mr;
    for (size_t t = 0; t < ncell; ++t)
        if (d_cell(o.o_rc, t) != 1 || d_cell(o.o_clo, t) != 1 || d_cell(o.o_chi, t) != 1 ||
            i_cell(o.o_kind, t) != 1 || i_cell(o.o_row, t) != 1)
            return fail("a per-column output cell is not written exactly once", SR, SC, (int)t);
    for (size_t t = 0; t < nrow; ++t)
        if (d_cell(o.o_shadow, t) != 1 || d_cell(o.o_rlo, t) != 1 ||
            d_cell(o.o_rhi, t) != 1 || d_cell(o.o_now, t) != 1)
            return fail("a per-constraint output cell is not written exactly once", SR, SC, (int)t);
    return sink < 0.0;  // never: keeps the reads alive
}

int main() {
    int bad = 0, batches = 0;
    // fixed-shape batches, one and three scenarios
    for (int R = 0; R <= 40; ++R)
        for (int C = 0; C <= R + 30; ++C, ++batches) {
            std::vector<Shape> sc(R >= 2 && C >= R ? 3 : 1, Shape{R, C});
            bad += check_batch(R, C, sc);
        }
    const int wide[] = {64, 65, 66, 256, 257, 258, 512, 514, 1300, 2048};
    const int tall[] = {2, 4, 5, 6, 9, 65, 200, 257, 1024};
    for (int R : tall)
        for (int C : wide)
            if (C >= R) {
                bad += check_batch(R, C, {Shape{R, C}});
                ++batches;
            }
    // grow batches: scenarios at the base's shape, grown by columns, by rows and columns, mixed
    const Shape bases[] = {{2, 2}, {3, 5}, {9, 21}, {21, 63}, {64, 132}, {101, 255}};
    for (const Shape& b : bases) {
        std::vector<Shape> sc = {b, Shape{b.R, b.C + 1}, Shape{b.R + 1, b.C + 1},
                                 Shape{b.R + 2, b.C + 3}, b, Shape{b.R + 1, b.C + 2}};
        bad += check_batch(b.R, b.C, sc);
        ++batches;
    }
    bad += check_batch(0, 0, {});
    ++batches;
    std::printf("sens_batch_ranging_check: %d batches, %d failures\n", batches, bad);
    return bad ? 1 : 0;
}
