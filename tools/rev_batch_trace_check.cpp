// rev_batch_trace_check.cpp -- host-only check of the record layout of a traced revised-simplex
// batch (csrc/rev_batch_common.hpp).  It walks every index the traced
// kernels and the engine form over the trace slab -- the per-LP offsets of
// lpr_rev_batch_trace_reserve, the field offsets of rev_trace_*, the record cap, the lane walks
// of rev_batch_body.hpp (NT lanes apart; for_each_ij's additions and carry for the two tables) --
// over an exactly-sized heap buffer, so that an address sanitizer sees any index past the size
// computed there, and checks that every cell of every kept record is written exactly once: the
// pre-pivot part, the tables and the part the next pass completes for a pivot record, all at once
// for the "Optimal" record.  A record index at or past the cap is counted, never written.  No
// GPU is used:
//   hipcc -std=c++17 -O1 -g -DLPR_BUILD -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all --offload-arch=gfx950 \
//       tools/rev_batch_trace_check.cpp -o /tmp/rev_batch_trace_check && \
//       /tmp/rev_batch_trace_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../lpr_381_group_v22_amd/csrc/rev_batch_common.hpp"

using namespace lpr;

struct Lp {
    int m, n;
    long long pivots;  // iterations the LP makes
    bool optimal;      // and whether it ends with the "Optimal" record
};

static int fail(const char* what, int k, long long rec) {
    std::fprintf(stderr, "rev_batch_trace_check: %s (LP %d, record %lld)\n", what, k, rec);
    return 1;
}

// for_each_ij of batch_device.hpp for one lane: x = i * cols + j, NT apart, (i, j) by additions
template <class F>
static void lane_ij(int NT, int rows, int cols, int lane, F&& f) {
    const int n = rows * cols;
    const int di = NT / cols, dj = NT - di * cols;
    int i = lane / cols, j = lane - (lane / cols) * cols;
    for (int x = lane; x < n; x += NT) {
        f(x, i, j);
        i += di;
        j += dj;
        if (j >= cols) {
            j -= cols;
            ++i;
        }
    }
}

// One batch: the offsets as lpr_rev_batch_trace_reserve forms them, then every write of the
// kernels, NT lanes per LP.
static int check_batch(const std::vector<Lp>& lps, int cap, int NT) {
    const int count = (int)lps.size();
    std::vector<int64_t> off((size_t)count);
    int64_t total = 0;
    for (int k = 0; k < count; ++k) {
        off[(size_t)k] = total;
        total += (int64_t)cap * rev_trace_stride(lps[(size_t)k].m, lps[(size_t)k].n);
    }
    std::unique_ptr<unsigned char[]> hits(new unsigned char[(size_t)total]);  // writes per double
    std::memset(hits.get(), 0, (size_t)total);
    for (int k = 0; k < count; ++k) {
        const int m = lps[(size_t)k].m, n = lps[(size_t)k].n;
        const int64_t stride = rev_trace_stride(m, n);
        if (stride != 6 + 7LL * m + n + (int64_t)m * n + (int64_t)m * m)
            return fail("the stride is not 6 + 7m + n + mn + mm", k, -1);
        if (rev_trace_y(m, n) != kRevTraceScalars || rev_trace_binv(m, n) + (int64_t)m * m != stride)
            return fail("the fields do not tile the record", k, -1);
        unsigned char* const trec = hits.get() + off[(size_t)k];
        const long long records = lps[(size_t)k].pivots + (lps[(size_t)k].optimal ? 1 : 0);
        for (long long rec_i = 0; rec_i < records; ++rec_i) {
            if (!(rec_i < cap)) continue;  // counted, not written
            unsigned char* const rec = trec + rec_i * stride;
            const bool pivot = rec_i < lps[(size_t)k].pivots;
            for (int lane = 0; lane < NT; ++lane) {
                if (pivot) {
                    // the pre-pivot part, in the pass that makes the pivot
                    for (int i = lane; i < m; i += NT) {
                        rec[rev_trace_u(m, n) + i] += 1;
                        rec[rev_trace_ratios(m, n) + i] += 1;
                        rec[rev_trace_basis_pre(m, n) + i] += 1;
                    }
                    if (lane == 0)
                        for (int s : {kRevTraceEnter, kRevTraceRow, kRevTraceLeave, kRevTraceRcPre})
                            rec[s] += 1;
                    // what the top of the next pass completes
                    for (int i = lane; i < m; i += NT) {
                        rec[rev_trace_xb(m, n) + i] += 1;
                        rec[rev_trace_y(m, n) + i] += 1;
                        rec[rev_trace_rcs(m, n) + i] += 1;
                    }
                    for (int j = lane; j < n; j += NT) rec[rev_trace_rcx(m, n) + j] += 1;
                    if (lane == 0) {
                        rec[kRevTraceZWorking] += 1;
                        rec[kRevTraceZOriginal] += 1;
                    }
                } else {
                    // the "Optimal" record, whole
                    for (int j = lane; j < n; j += NT) rec[rev_trace_rcx(m, n) + j] += 1;
                    for (int i = lane; i < m; i += NT) {
                        rec[rev_trace_y(m, n) + i] += 1;
                        rec[rev_trace_rcs(m, n) + i] += 1;
                        rec[rev_trace_u(m, n) + i] += 1;
                        rec[rev_trace_ratios(m, n) + i] += 1;
                        rec[rev_trace_basis_pre(m, n) + i] += 1;
                        rec[rev_trace_xb(m, n) + i] += 1;
                    }
                    if (lane == 0)
                        for (int s = 0; s < kRevTraceScalars; ++s) rec[s] += 1;
                }
                // rev_trace_tables: the basis after the pivot, B^-1 A, B^-1
                for (int i = lane; i < m; i += NT) rec[rev_trace_basis_post(m, n) + i] += 1;
                lane_ij(NT, m, n, lane, [&](int x, int i, int j) {
                    if (i < 0 || i >= m || j < 0 || j >= n || x != i * n + j) std::abort();
                    rec[rev_trace_binva(m, n) + x] += 1;
                });
                lane_ij(NT, m, m, lane, [&](int x, int i, int j) {
                    if (i < 0 || i >= m || j < 0 || j >= m || x != i * m + j) std::abort();
                    rec[rev_trace_binv(m, n) + x] += 1;
                });
            }
        }
        // every cell of every kept record exactly once, nothing past them
        const long long kept = records < cap ? records : cap;
        for (int64_t t = 0; t < (int64_t)cap * stride; ++t) {
            const unsigned char want = t < kept * stride ? 1 : 0;
            if (trec[t] != want)
                return fail(want ? "a cell of a kept record is not written exactly once"
                                 : "a cell past the kept records is written",
                            k, (long long)(t / stride));
        }
        // lpr_rev_batch_trace_read's range rule: [first, first + cnt) inside the kept records
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
    // every small shape, alone, in every lane count, below, at and past the cap
    for (int m = 1; m <= 9; ++m)
        for (int n = 1; n <= 11; ++n)
            for (int NT : {64, 256})
                for (int cap : {1, 2, 5}) {
                    bad += check_batch({Lp{m, n, 0, true}}, cap, NT);
                    bad += check_batch({Lp{m, n, 3, true}, Lp{m, n, 4, false}}, cap, NT);
                    batches += 2;
                }
    // mixed shapes and strides as neighbours: m = 1, n = 1, odd sizes, no multiple of the lanes,
    // LPs with no record, at the cap and past it
    const std::vector<Lp> mixed = {{1, 1, 1, true},   {1, 12, 2, true},  {8, 1, 0, false},
                                   {3, 4, 3, false},  {65, 63, 2, true}, {1, 1, 0, true},
                                   {33, 20, 9, true}, {70, 12, 1, false}, {257, 130, 1, true},
                                   {2, 2, 4, true}};
    for (int NT : {64, 256})
        for (int cap : {1, 4, 300}) {
            bad += check_batch(mixed, cap, NT);
            ++batches;
        }
    // the H limit: m = 1023 with n + m = 2047, and the shape one row short of it
    bad += check_batch({Lp{1023, 1024, 1, true}, Lp{1, 1, 1, true}, Lp{1022, 1025, 2, false}}, 2,
                       256);
    ++batches;
    std::printf("rev_batch_trace_check: %d batches, %d failures\n", batches, bad);
    return bad ? 1 : 0;
}
