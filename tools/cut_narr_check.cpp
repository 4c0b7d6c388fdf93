// cut_narr_check.cpp -- host-only walker over the record layout of a narrated cutting-plane batch
// (DESIGN.md section 24).  It includes csrc/cut_narr_layout.hpp and the cursor it embeds
// (csrc/kept_prefix.hpp), replays the push rule (kept_push, the text the kernels compile) and the
// lane walk of cut_batch_body.hpp for 256 lanes -- the cut row by its `j += 256` loop, the
// tableau after a pivot by the four-in-flight update walk, lane `tid` of pass u at element
// base + u * 256 + tid with its (i, j) advanced by (256 / C, 256 % C) -- over a data buffer of
// exactly the reserved size, and checks that every cell of every kept block is written exactly
// once, by the (i, j) the walk claims for it, and none past the item's slice.  Built with the
// address and undefined-behaviour sanitizers and run as a program (tests/test_cut_batch_narr_cpu.py):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <csrc> \
//       tools/cut_narr_check.cpp -o cut_narr_check && ./cut_narr_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cut_narr_layout.hpp"
#include "kept_prefix.hpp"

using namespace lpr;

namespace {

constexpr int NT = 256;

[[noreturn]] void fail(const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "cut_narr_check: FAILED: %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}

struct Item {
    CutNarrDesc c;
    std::vector<int32_t> ev;       // exactly 4 * ev_cap
    std::vector<double> data;      // exactly cap: the sanitizer sees any store past it
    std::vector<uint8_t> written;  // per double
    int64_t need = 0;              // doubles an unlimited item keeps
    std::vector<int64_t> starts;   // block starts of the list model
};

void event(Item& it, int kind, int a, int b, int rows_now) {
    const int64_t at = cut_narr_event(it.c);
    if (at >= 0) {
        if (at >= it.c.ev_cap) fail("event index past ev_cap", at, it.c.ev_cap);
        int32_t* e = it.ev.data() + 4 * at;
        e[0] = kind;
        e[1] = a;
        e[2] = b;
        e[3] = rows_now;
    }
}

void store(Item& it, int64_t at, int64_t x, double v) {
    const int64_t p = at + x;
    if (p < 0 || p >= it.c.kp.cap) fail("store past the slice", p, it.c.kp.cap);
    if (it.written[(size_t)p]) fail("cell written twice", p, x);
    it.written[(size_t)p] = 1;
    it.data[(size_t)p] = v;
}

// the value the walk must give element (i, j) of block `blk`
double cell(int64_t blk, int i, int j) { return (double)blk * 1e7 + (double)i * 4096.0 + j; }

// block 0 (k_cut_batch_narr_first) and the cut row: lane tid stores x = tid, tid + 256, ...
void strided_block(Item& it, int64_t n, int row, int C) {
    const int64_t blk = it.c.kp.made_n;
    const int64_t at = kept_push(it.c.kp, n);
    it.starts.push_back(it.need);
    it.need += n;
    if (at < 0) return;
    for (int tid = 0; tid < NT; ++tid)
        for (int64_t x = tid; x < n; x += NT)
            store(it, at, x, row >= 0 ? cell(blk, row, (int)x) : cell(blk, (int)(x / C), (int)(x % C)));
}

// the tableau after a pivot: the update walk of cut_batch_body.hpp, four elements in flight
void pivot_block(Item& it, int R, int C) {
    const int64_t blk = it.c.kp.made_n;
    const int64_t n = (int64_t)R * C;
    const int64_t at = kept_push(it.c.kp, n);
    it.starts.push_back(it.need);
    it.need += n;
    if (at < 0) return;
    constexpr int U = 4;
    const int RC = R * C;
    const int di = NT / C, dj = NT - (NT / C) * C;
    for (int tid = 0; tid < NT; ++tid) {
        int i = tid / C, j = tid - (tid / C) * C;
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
                const int x = base + u * NT + tid;
                if (x < RC) {
                    if ((int64_t)ii[u] * C + jj[u] != x) fail("(i, j) is not element x", x, ii[u]);
                    store(it, at, x, cell(blk, ii[u], jj[u]));
                }
            }
        }
    }
}

// One item: R0 x C, `cuts` cuts, each followed by its pivot and `solver_pivots` more, under
// `cap` doubles and `ev_cap` events.  Returns the doubles an unlimited run makes.
int64_t run(int R0, int C, int cuts, int solver_pivots, int64_t cap, int ev_cap) {
    Item it;
    it.c = CutNarrDesc();
    it.c.kp.cap = cap;
    it.c.ev_cap = ev_cap;
    it.ev.assign((size_t)4 * ev_cap, -1);
    it.data.assign((size_t)cap, -1.0);
    it.written.assign((size_t)cap, 0);
    std::vector<int32_t> kinds, rows;  // the list model of the events
    auto ev = [&](int kind, int a, int b, int rows_now) {
        kinds.push_back(kind);
        rows.push_back(rows_now);
        event(it, kind, a, b, rows_now);
    };
    int R = R0;
    strided_block(it, (int64_t)R * C, -1, C);  // block 0
    ev(kCutEvCall, 0, 1, R);
    for (int c = 0; c < cuts; ++c) {
        ev(kCutEvLevel, 0, 0, R);
        ev(kCutEvCut, 0, 0, R + 1);
        strided_block(it, C, R, C);
        R += 1;  // rows grow by one per cut
        ev(kCutEvPivot + 2, R - 2, 0, R);
        pivot_block(it, R, C);
        ev(kCutEvSolveBegin, 0, 0, R);
        for (int p = 0; p < solver_pivots; ++p) {
            ev(kCutEvPivot + (p & 1), 0, 0, R);
            pivot_block(it, R, C);
        }
        ev(kCutEvSolveEnd, 0, 0, R);
    }
    ev(kCutEvExit, 6, 0, R);

    // ---- against the list model
    const int64_t n_ev = (int64_t)kinds.size();
    if (it.c.ev_n != n_ev) fail("ev_n is not exact", it.c.ev_n, n_ev);
    for (int64_t e = 0; e < n_ev && e < ev_cap; ++e)
        if (it.ev[(size_t)(4 * e)] != kinds[(size_t)e] || it.ev[(size_t)(4 * e + 3)] != rows[(size_t)e])
            fail("a kept event differs", e);
    // offsets are the prefix sum of cut_narr_event_doubles over the events, after block 0
    int64_t off = (int64_t)R0 * C;
    size_t blk = 1;
    for (int64_t e = 0; e < n_ev; ++e) {
        const int64_t n = cut_narr_event_doubles(kinds[(size_t)e], rows[(size_t)e], C);
        if (n == 0) continue;
        if (blk >= it.starts.size() || it.starts[blk] != off) fail("block offset is not the prefix sum", e, off);
        off += n;
        ++blk;
    }
    if (blk != it.starts.size() || off != it.need) fail("block count / need", (long long)blk, off);
    if (it.c.kp.made_d != it.need || it.c.kp.made_n != (int64_t)it.starts.size())
        fail("made counts are not exact", it.c.kp.made_d, it.c.kp.made_n);
    // what is kept is the longest prefix of whole blocks that fits
    int64_t kept_b = 0, kept_d = 0;
    for (size_t q = 0; q < it.starts.size(); ++q) {
        const int64_t end = q + 1 < it.starts.size() ? it.starts[q + 1] : it.need;
        if (end > cap) break;
        kept_b = (int64_t)q + 1;
        kept_d = end;
    }
    if (it.c.kp.kept_n != kept_b || it.c.kp.cur != kept_d) fail("kept is not the whole-block prefix", it.c.kp.kept_n, kept_b);
    // every cell of every kept block written exactly once with its own value; nothing behind
    for (int64_t p = 0; p < cap; ++p) {
        const bool want = p < kept_d;
        if ((it.written[(size_t)p] != 0) != want) fail("cell coverage", p, want);
    }
    for (size_t q = 0; q < (size_t)kept_b; ++q) {
        const int64_t end = q + 1 < it.starts.size() ? it.starts[q + 1] : it.need;
        const int64_t n = end - it.starts[q];
        for (int64_t x = 0; x < n; ++x) {
            // a cut row (n == C behind block 0) sits in row `rows at that time`; its value was
            // made with the row index, so only the column part is checked through the modulus
            const double v = it.data[(size_t)(it.starts[q] + x)];
            const double col = v - (double)q * 1e7;
            const long long j = (long long)col % 4096;
            if (j != x % C) fail("cell holds another cell's value", (long long)q, x);
        }
    }
    return it.need;
}

void shape(int R0, int C, int cuts, int solver_pivots) {
    run(R0, C, cuts, solver_pivots, 1, 1);                                   // cap 1: nothing fits
    const int64_t full = run(R0, C, cuts, solver_pivots, 0, 1);             // caps 0: only counts
    const int ev_need = 2 + cuts * (5 + solver_pivots);
    if (run(R0, C, cuts, solver_pivots, full, ev_need) != full) fail("need changed with the cap");
    run(R0, C, cuts, solver_pivots, full - 1, ev_need - 1);                  // one double short of the last block
    run(R0, C, cuts, solver_pivots, (int64_t)R0 * C - 1, ev_need);           // one short of block 0
    run(R0, C, cuts, solver_pivots, (int64_t)R0 * C + C - 1, ev_need);       // one short of the first cut row
    run(R0, C, cuts, solver_pivots, (int64_t)R0 * C + C + (int64_t)(R0 + 1) * C - 1, ev_need);  // ... of the first pivot block
}

}  // namespace

int main() {
    static_assert(cut_narr_event_doubles(kCutEvCut, 7, 5) == 5, "a cut adds its row");
    static_assert(cut_narr_event_doubles(kCutEvPivot + 2, 7, 5) == 35, "a pivot adds the tableau");
    static_assert(cut_narr_event_doubles(kCutEvSolveEnd, 7, 5) == 0, "the rest adds nothing");
    static_assert(cut_narr_event_doubles(kCutEvPivot, 1024, 2048) == (int64_t)1024 * 2048, "64-bit");
    shape(3, 5, 2, 1);       // R C < 256
    shape(2, 2, 1, 0);       // the smallest
    shape(12, 21, 3, 2);     // R C < 1024, C does not divide 256
    shape(41, 101, 3, 2);    // R C not a multiple of 1024, C does not divide 256
    shape(40, 64, 2, 1);     // C divides 256
    shape(7, 300, 2, 1);     // C > 256
    shape(5, 2048, 1, 1);    // the widest
    shape(1021, 2048, 3, 0); // rows growing to the H limit 1024 x 2048
    std::puts("cut_narr_check: ok");
    return 0;
}
