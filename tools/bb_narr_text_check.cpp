// bb_narr_text_check.cpp -- host-only walker over the block layout of a narrated B&B batch's device
// text (lpr_381_group_v22_amd/csrc/bb_narr_text_layout.hpp).  It builds the
// per-record arrays of one IP the way the search kernel does -- tab_off is the cursor before the
// child's first push, ntab the tableaux made after the drop of :392-400, both through kept_push /
// kept_drop of kept_prefix.hpp -- hands them to narr_text_runs, the very text the engine compiles,
// and checks for every cap:
//   - every block's source range lies inside the IP's kept prefix (each block is read, cell by
//     cell, from a buffer allocated at exactly the kept size);
//   - the blocks tile the prefix exactly: in order, back to back, from 0 to `kept`;
//   - a record keeps min(ntab, what the prefix holds of it), and the rounding count follows the
//     child's status.
// Build with a plain host compiler under -fsanitize=address,undefined and run as a program:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I lpr_381_group_v22_amd/csrc \
//       tools/bb_narr_text_check.cpp -o bb_narr_text_check && ./bb_narr_text_check
#include "bb_narr_text_layout.hpp"
#include "kept_prefix.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int g_fail = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
            ++g_fail;                                      \
        }                                                  \
    } while (0)

constexpr int kStride = 5;  // integers per record as the device keeps them: depth at 2, status at 4

// One child LP: its depth, the pivots it took, whether the last tableau is dropped (:392-400), and
// how it ended (0 solved, 1 infeasible, 2 failed).
struct Child {
    int depth, piv;
    bool drop;
    int status;
};

struct Records {
    std::vector<int32_t> ints;  // kStride per record; record 0 is the root
    std::vector<int64_t> tab_off;
    std::vector<int32_t> ntab;
    lpr::KeptPrefix kp{};
};

// The kernel's bookkeeping of one IP with `cap` doubles reserved.
Records run(int R0, int C0, const std::vector<Child>& kids, int64_t cap) {
    Records r;
    r.kp.cap = cap;
    lpr::kept_rewind(r.kp);
    r.ints.assign(kStride, 0);
    r.ints[0] = -1;
    r.tab_off.push_back(0);
    r.ntab.push_back(0);
    for (const Child& c : kids) {
        const int64_t n = (int64_t)(R0 + c.depth) * (C0 + c.depth);
        const int64_t first = r.kp.cur, made0 = r.kp.made_n;
        for (int i = 0; i <= c.piv; ++i) (void)lpr::kept_push(r.kp, n);
        if (c.drop) lpr::kept_drop(r.kp, n);
        const int32_t e[kStride] = {0, 1, c.depth, 0, c.status};
        r.ints.insert(r.ints.end(), e, e + kStride);
        r.tab_off.push_back(first);
        r.ntab.push_back((int32_t)(r.kp.made_n - made0));
    }
    return r;
}

int64_t need_of(int R0, int C0, const std::vector<Child>& kids) {
    return run(R0, C0, kids, INT64_MAX / 2).kp.made_d;
}

void walk(const char* what, int R0, int C0, const std::vector<Child>& kids, int64_t cap) {
    const Records r = run(R0, C0, kids, cap);
    const int64_t nrec = (int64_t)r.ntab.size(), kept = r.kp.cur;
    CHECK(kept <= cap, "%s cap %lld: keeps %lld", what, (long long)cap, (long long)kept);
    std::vector<lpr::NarrTextRun> runs((size_t)nrec);
    const int64_t blocks = lpr::narr_text_runs(R0, C0, nrec, r.ints.data() + 2, r.ints.data() + 4,
                                               kStride, r.tab_off.data(), r.ntab.data(), kept,
                                               runs.data());
    CHECK(blocks == r.kp.kept_n, "%s cap %lld: %lld blocks, the cursor kept %lld tableaux", what,
          (long long)cap, (long long)blocks, (long long)r.kp.kept_n);
    // exactly sized: a block that reaches past the prefix is an AddressSanitizer report
    double* slice = static_cast<double*>(std::malloc((size_t)(kept ? kept : 1) * sizeof(double)));
    for (int64_t x = 0; x < kept; ++x) slice[x] = (double)x;
    int64_t at = 0, seen = 0;
    bool cut = false;  // a record kept fewer than it made: nothing after it is kept
    for (int64_t rid = 0; rid < nrec; ++rid) {
        const lpr::NarrTextRun& q = runs[(size_t)rid];
        const int depth = r.ints[(size_t)(rid * kStride + 2)];
        CHECK(q.rows == R0 + depth && q.cols == C0 + depth, "%s record %lld: shape", what,
              (long long)rid);
        CHECK(q.count >= 0 && q.count <= r.ntab[(size_t)rid], "%s record %lld: count %d of %d",
              what, (long long)rid, q.count, r.ntab[(size_t)rid]);
        CHECK(!(cut && q.count > 0), "%s record %lld: blocks after a cut record", what,
              (long long)rid);
        cut = cut || q.count < r.ntab[(size_t)rid];
        CHECK(q.round4 == (r.ints[(size_t)(rid * kStride + 4)] == 0 ? 2 : 1),
              "%s record %lld: round4 %d", what, (long long)rid, q.round4);
        const int64_t each = (int64_t)q.rows * q.cols;
        for (int32_t i = 0; i < q.count; ++i) {
            const int64_t lo = q.off + i * each;
            CHECK(lo == at, "%s record %lld block %d: starts at %lld, the tiling is at %lld", what,
                  (long long)rid, i, (long long)lo, (long long)at);
            CHECK(lo >= 0 && lo + each <= kept, "%s record %lld block %d: [%lld, %lld) of %lld",
                  what, (long long)rid, i, (long long)lo, (long long)(lo + each), (long long)kept);
            double sum = 0.0;
            for (int64_t x = 0; x < each; ++x) sum += slice[lo + x];  // the kernels' loads
            CHECK(sum == (double)each * (double)(2 * lo + each - 1) / 2.0 || each > (1 << 20),
                  "%s record %lld block %d: cells", what, (long long)rid, i);
            at = lo + each;
            ++seen;
        }
    }
    CHECK(at == kept && seen == blocks, "%s cap %lld: blocks end at %lld, the prefix at %lld", what,
          (long long)cap, (long long)at, (long long)kept);
    if (cap >= r.kp.made_d)
        CHECK(!cut && blocks == r.kp.made_n, "%s: the exact need keeps all", what);
    std::free(slice);
}

void caps(const char* what, int R0, int C0, const std::vector<Child>& kids) {
    const int64_t need = need_of(R0, C0, kids);
    const int64_t first = (int64_t)(R0 + kids[0].depth) * (C0 + kids[0].depth);
    for (int64_t cap : {(int64_t)0, first - 1, first, need - 1, need, need + 7}) walk(what, R0, C0, kids, cap);
    // every boundary between two tableaux, and one double to either side of it
    if (need < 200000) {
        const Records all = run(R0, C0, kids, need);
        for (size_t rid = 1; rid < all.ntab.size(); ++rid)
            for (int64_t d = -1; d <= 1; ++d)
                if (all.tab_off[rid] + d >= 0) walk(what, R0, C0, kids, all.tab_off[rid] + d);
    }
}

}  // namespace

int main() {
    // the sample model's shape: solved children with and without the step back, an infeasible
    // child with several tableaux, a failed child (no pivot, its one tableau dropped)
    caps("sample", 8, 14,
         {{1, 2, false, 0}, {1, 3, true, 0}, {2, 2, false, 1}, {2, 0, true, 2}, {2, 1, false, 0},
          {3, 0, false, 1}, {3, 4, true, 0}});
    // a dropped tableau larger than everything after it
    caps("deep drop, shallow rest", 8, 14,
         {{9, 3, true, 0}, {1, 0, false, 1}, {2, 2, true, 0}, {1, 1, false, 0}});
    // a 1 x 2 root: the smallest tableaux
    caps("tiny", 1, 2, {{1, 0, false, 1}, {1, 1, false, 0}, {2, 5, true, 0}});
    // the H limit: children of 1024 x 2048 at full depth
    caps("H limit", 1024 - 20, 2048 - 20, {{20, 2, true, 0}, {19, 1, false, 1}});
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::puts("bb_narr_text_check: ok");
    return 0;
}
