// bb_narr_check.cpp -- host-only walker over the record layout of a narrated B&B batch
// (lpr_381_group_v22_amd/csrc/bb_narr_layout.hpp).  It replays the cursor
// rules the search kernel uses (kept_push / kept_drop of kept_prefix.hpp and narr_rewind, the very
// text the kernel compiles) over a slab allocated at exactly the reserved size, writes every cell
// of every kept tableau as the kernel's lanes would, and checks against a model that keeps plain
// lists:
//   - kept tableaux are compact and in order, from the slice start;
//   - the drop of :392-400 steps back by exactly the last tableau, kept or not;
//   - once a tableau does not fit, no later one is written (a prefix), and the totals stay exact;
//   - every cell of every kept tableau is written exactly once, none past the slice or in a
//     neighbour's slice.
// Build with a plain host compiler under -fsanitize=address,undefined and run as a program:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I lpr_381_group_v22_amd/csrc \
//       tools/bb_narr_check.cpp -o bb_narr_check && ./bb_narr_check
#include "bb_narr_layout.hpp"
#include "kept_prefix.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using lpr::BBNarrDesc;

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

struct Event {
    int64_t n;   // doubles of the tableau pushed; 0: drop the last one made
};

// One child LP at depth `dep` of an R0 x C0 root: AddConstraint's tableau, `piv` pivots, and the
// drop of the last one where `drop`.
void child(std::vector<Event>& ev, int R0, int C0, int dep, int piv, bool drop) {
    const int64_t n = (int64_t)(R0 + dep) * (C0 + dep);
    for (int i = 0; i <= piv; ++i) ev.push_back({n});
    if (drop) ev.push_back({0});
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t mod) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % mod);
}

// A DFS-like run: children of varying depth, so a later tableau may be smaller than a dropped one.
std::vector<Event> search(int R0, int C0, int node_cap, int max_piv) {
    std::vector<Event> ev;
    for (int pop = 0; pop < node_cap; ++pop) {
        const int dep = 1 + (int)rnd((uint32_t)node_cap);
        for (int side = 0; side < 2; ++side) {
            const int piv = (int)rnd((uint32_t)max_piv + 1);
            child(ev, R0, C0, dep, piv, piv > 0 && rnd(3) == 0);
        }
    }
    return ev;
}

// The exact need of a run: the doubles of the tableaux that remain.
int64_t need_of(const std::vector<Event>& ev) {
    std::vector<int64_t> live;
    for (const Event& e : ev) {
        if (e.n) live.push_back(e.n);
        else live.pop_back();
    }
    int64_t s = 0;
    for (int64_t n : live) s += n;
    return s;
}

struct Ip {
    std::vector<Event> ev;
    int64_t cap;
};

// Replays every IP over one slab of exactly sum(cap) doubles.
void walk(const char* what, const std::vector<Ip>& ips) {
    int64_t total = 0;
    std::vector<BBNarrDesc> desc(ips.size());
    for (size_t k = 0; k < ips.size(); ++k) {
        desc[k] = BBNarrDesc{};
        desc[k].slab_off = total;
        desc[k].kp.cap = ips[k].cap;
        desc[k].kp.cur = 77;  // stale state of an earlier run: the rewind clears it
        desc[k].kp.made_n = 5;
        total += ips[k].cap;
    }
    // exactly sized: one write past the end is an AddressSanitizer report
    double* slab = static_cast<double*>(std::malloc((size_t)(total ? total : 1) * sizeof(double)));
    unsigned char* hits = static_cast<unsigned char*>(std::calloc((size_t)(total ? total : 1), 1));
    for (size_t k = 0; k < ips.size(); ++k) {
        BBNarrDesc& c = desc[k];
        lpr::narr_rewind(c);
        struct Made { int64_t n, at; };
        std::vector<Made> model;  // the list DoDualSimplex-es build, with where each was kept
        bool model_full = false;  // some live tableau is not kept
        int64_t model_kept = 0;
        int64_t last_n = 0;
        for (const Event& e : ips[k].ev) {
            if (e.n) {
                const int64_t at = lpr::kept_push(c.kp, e.n);
                const bool keep = !model_full && model_kept + e.n <= c.kp.cap;
                CHECK((at >= 0) == keep, "%s IP %zu: push of %lld kept=%d, model %d", what, k,
                      (long long)e.n, at >= 0, keep);
                if (keep) {
                    CHECK(at == model_kept, "%s IP %zu: not compact (%lld, want %lld)", what, k,
                          (long long)at, (long long)model_kept);
                    model_kept += e.n;
                } else {
                    model_full = true;
                }
                model.push_back({e.n, at});
                if (at >= 0) {
                    CHECK(at + e.n <= c.kp.cap, "%s IP %zu: past the slice", what, k);
                    double* rec = slab + c.slab_off + at;
                    for (int64_t x = 0; x < e.n; ++x) {  // the lanes' second stores
                        rec[x] = (double)x;
                        ++hits[c.slab_off + at + x];
                    }
                }
                last_n = e.n;
            } else {
                const Made m = model.back();
                model.pop_back();
                CHECK(m.n == last_n, "%s: the walker drops only the tableau just made", what);
                lpr::kept_drop(c.kp, m.n);
                if (m.at >= 0) {
                    model_kept -= m.n;
                    for (int64_t x = 0; x < m.n; ++x) --hits[c.slab_off + m.at + x];
                }
                model_full = false;
                for (const Made& q : model) model_full = model_full || q.at < 0;
            }
            int64_t md = 0;
            for (const Made& q : model) md += q.n;
            CHECK(c.kp.made_n == (int64_t)model.size() && c.kp.made_d == md &&
                      c.kp.cur == model_kept,
                  "%s IP %zu: totals (%lld %lld %lld), model (%zu %lld %lld)", what, k,
                  (long long)c.kp.made_n, (long long)c.kp.made_d, (long long)c.kp.cur,
                  model.size(), (long long)md, (long long)model_kept);
        }
        // what is kept is a prefix of what was made
        bool gap = false;
        int64_t kept_t = 0;
        for (const Made& q : model) {
            CHECK(!(gap && q.at >= 0), "%s IP %zu: a tableau kept after one that was not", what, k);
            gap = gap || q.at < 0;
            kept_t += q.at >= 0;
        }
        CHECK(c.kp.kept_n == kept_t, "%s IP %zu: kept_t", what, k);
        if (c.kp.cap >= need_of(ips[k].ev))
            CHECK(!gap && c.kp.cur == c.kp.made_d, "%s IP %zu: the exact need keeps all", what, k);
        for (int64_t x = 0; x < c.kp.cap; ++x)
            if (hits[c.slab_off + x] != (x < c.kp.cur ? 1 : 0)) {
                CHECK(false, "%s IP %zu: cell %lld written %d times (kept %lld)", what, k,
                      (long long)x, hits[c.slab_off + x], (long long)c.kp.cur);
                break;
            }
    }
    std::free(slab);
    std::free(hits);
}

}  // namespace

int main() {
    // the sample model's shape, several runs with their exact needs, side by side
    {
        std::vector<Ip> ips;
        for (int k = 0; k < 6; ++k) {
            std::vector<Event> ev = search(8, 14, 20, 4);
            ips.push_back({ev, need_of(ev)});
        }
        walk("exact", ips);
        for (Ip& ip : ips) ip.cap -= 1;
        walk("one double short of the need", ips);
        for (Ip& ip : ips) ip.cap = 0;
        walk("cap 0", ips);
        for (Ip& ip : ips) ip.cap = ip.ev.front().n - 1;
        walk("one double short of a tableau", ips);
        for (Ip& ip : ips) ip.cap = ip.ev.front().n;
        walk("one tableau", ips);
        for (size_t k = 0; k < ips.size(); ++k) ips[k].cap = (int64_t)rnd(16000);
        walk("mixed caps", ips);
    }
    // a dropped tableau larger than everything after it: the exact need still keeps all
    {
        std::vector<Event> ev;
        child(ev, 8, 14, 9, 3, true);
        child(ev, 8, 14, 1, 0, false);
        child(ev, 8, 14, 2, 2, true);
        child(ev, 8, 14, 1, 1, false);
        walk("deep drop, shallow rest", {{ev, need_of(ev)}, {ev, need_of(ev) - 1}, {ev, 0}});
    }
    // the H limit: children of 1024 x 2048 at full depth
    {
        std::vector<Event> ev;
        child(ev, 1024 - 20, 2048 - 20, 20, 2, true);
        child(ev, 1024 - 20, 2048 - 20, 19, 1, false);
        const int64_t need = need_of(ev);
        walk("H limit", {{ev, need}, {ev, need - 1}, {ev, (int64_t)1024 * 2048 - 1}, {ev, 0}});
    }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::puts("bb_narr_check: ok");
    return 0;
}
