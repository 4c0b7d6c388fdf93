// batch_trace_check.cpp -- host-only check of the record layout of a traced primal batch
// (csrc/batch_common.hpp).  It walks every index the traced kernels and the
// engine form over the trace slab -- the per-LP offsets of lpr_batch_trace_reserve, the header and
// tableau offsets of batch_trace_*, the record cap, record 0 of k_batch_trace_first (64 lanes) and
// the four-in-flight lane walk of batch_body.hpp's update pass (its additions and carry, NT = 64
// and 256) -- over an exactly-sized heap buffer, so that an address sanitizer sees any index past
// the size computed there, and checks that every cell of every kept record is written exactly
// once and none past them.  A record index at or past the cap is counted, never written.  The
// header is taken with LPR_BATCH_LAYOUT_ONLY: no HIP, any host compiler.  No GPU is used:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/batch_trace_check.cpp -o batch_trace_check && ./batch_trace_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define LPR_BATCH_LAYOUT_ONLY
#include "../lpr_381_group_v22_amd/csrc/batch_common.hpp"

using namespace lpr;

struct Lp {
    int rows, cols;
    long long pivots;  // pivots the LP makes: it has 1 + pivots records
};

static int fail(const char* what, int k, long long rec) {
    std::fprintf(stderr, "batch_trace_check: %s (LP %d, record %lld)\n", what, k, rec);
    return 1;
}

// The update pass of batch_simplex_run for one lane and one pivot: U = 4 elements in flight,
// x = base + u * NT + lane, (i, j) carried by additions.  f(x, i, j) for every x < RC.
template <class F>
static void lane_walk(int NT, int R, int C, int lane, F&& f) {
    constexpr int U = 4;
    const int RC = R * C;
    const int di = NT / C, dj = NT - (NT / C) * C;
    int i = lane / C, j = lane - (lane / C) * C;
    for (int base = 0; base < RC; base += U * NT) {
        int ii[U], jj[U];
        for (int u = 0; u < U; ++u) {
            ii[u] = i;
            jj[u] = j;
            i += di;
            j += dj;
            if (j >= C) {
                j -= C;
                ++i;
            }
        }
        for (int u = 0; u < U; ++u) {
            const int x = base + u * NT + lane;
            if (x < RC) f(x, ii[u], jj[u]);
        }
    }
}

// One batch: the offsets as lpr_batch_trace_reserve forms them, then every write of the kernels.
static int check_batch(const std::vector<Lp>& lps, int cap, int NT) {
    const int count = (int)lps.size();
    std::vector<int64_t> off((size_t)count);
    int64_t total = 0;
    for (int k = 0; k < count; ++k) {
        off[(size_t)k] = total;
        total += (int64_t)cap * batch_trace_stride(lps[(size_t)k].rows, lps[(size_t)k].cols);
    }
    std::unique_ptr<unsigned char[]> hits(new unsigned char[(size_t)total]);  // writes per double
    std::memset(hits.get(), 0, (size_t)total);
    for (int k = 0; k < count; ++k) {
        const int R = lps[(size_t)k].rows, C = lps[(size_t)k].cols;
        const int64_t stride = batch_trace_stride(R, C);
        if (stride != 2 + (int64_t)R * C) return fail("the stride is not 2 + rows x cols", k, -1);
        if (batch_trace_row() != 0 || batch_trace_col() != 1 ||
            batch_trace_tab() + (int64_t)R * C != stride)
            return fail("the header and the tableau do not tile the record", k, -1);
        unsigned char* const trec = hits.get() + off[(size_t)k];
        // record 0: k_batch_trace_first, one wave per LP
        for (int lane = 0; lane < 64; ++lane) {
            if (lane == 0) {
                trec[batch_trace_row()] += 1;
                trec[batch_trace_col()] += 1;
            }
            for (int x = lane; x < R * C; x += 64) trec[batch_trace_tab() + x] += 1;
        }
        // record iter + 1: the pass that makes pivot iter + 1
        for (long long iter = 0; iter < lps[(size_t)k].pivots; ++iter) {
            if (!(iter + 1 < cap)) continue;  // counted, not written
            unsigned char* const rtab = trec + (iter + 1) * stride + batch_trace_tab();
            for (int lane = 0; lane < NT; ++lane) {
                lane_walk(NT, R, C, lane, [&](int x, int i, int j) {
                    if (i < 0 || i >= R || j < 0 || j >= C || x != i * C + j) std::abort();
                    rtab[x] += 1;
                });
                if (lane == 0) {
                    unsigned char* const rec = rtab - batch_trace_tab();
                    rec[batch_trace_row()] += 1;
                    rec[batch_trace_col()] += 1;
                }
            }
        }
        // every cell of every kept record exactly once, nothing past them
        const long long records = 1 + lps[(size_t)k].pivots;
        const long long kept = records < cap ? records : cap;
        for (int64_t t = 0; t < (int64_t)cap * stride; ++t) {
            const unsigned char want = t < kept * stride ? 1 : 0;
            if (trec[t] != want)
                return fail(want ? "a cell of a kept record is not written exactly once"
                                 : "a cell past the kept records is written",
                            k, (long long)(t / stride));
        }
        // lpr_batch_trace_read's range rule: [first, first + cnt) inside the kept records
        for (long long first = -1; first <= kept + 1; ++first)
            for (long long cnt = -1; cnt <= kept + 1; ++cnt) {
                const bool ok = !(first < 0 || cnt < 0 || first > kept || cnt > kept - first);
                if (ok && off[(size_t)k] + (first + cnt) * stride > total)
                    return fail("an accepted read range passes the slab", k, first);
                if (ok != (first >= 0 && cnt >= 0 && first + cnt <= kept))
                    return fail("the read range rule", k, first);
            }
    }
    return 0;
}

int main() {
    int bad = 0, batches = 0;
    // every small shape, alone and paired, in every lane count, below, at and past the cap
    for (int R = 1; R <= 9; ++R)
        for (int C = 2; C <= 13; ++C)
            for (int NT : {64, 256})
                for (int cap : {1, 2, 5}) {
                    bad += check_batch({Lp{R, C, 0}}, cap, NT);
                    bad += check_batch({Lp{R, C, 3}, Lp{R, C, 4}}, cap, NT);
                    batches += 2;
                }
    // mixed shapes and strides as neighbours: rows = 1, cols = 2, odd sizes, no multiple of the
    // lanes or of four times the lanes, cols above the lane count, LPs with no pivot, at the cap
    // and past it
    const std::vector<Lp> mixed = {{1, 2, 1},   {1, 13, 2},   {9, 2, 0},   {4, 8, 3},
                                   {32, 63, 2}, {1, 2, 0},    {34, 54, 9}, {64, 318, 1},
                                   {3, 300, 5}, {257, 65, 1}, {2, 3, 4}};
    for (int NT : {64, 256})
        for (int cap : {1, 4, 300}) {
            bad += check_batch(mixed, cap, NT);
            ++batches;
        }
    // the H limit, 1024 x 2048, between small neighbours, and the shape one row short of it
    bad += check_batch({Lp{1, 2, 1}, Lp{1024, 2048, 1}, Lp{1, 2, 2}, Lp{1023, 2048, 2}}, 2, 256);
    ++batches;
    std::printf("batch_trace_check: %d batches, %d failures\n", batches, bad);
    return bad ? 1 : 0;
}
