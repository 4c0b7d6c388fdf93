// primal_plan_check.cpp -- stand-alone host program (its own main, no HIP, no GPU) that holds
// primal_plan() of csrc/primal_plan.hpp against a table of expected plans.  Every path stores the
// same bits, so nothing else in the suite would notice a wrong decision: only the speed would
// change.  The expectations are written by hand from the documentation of lpr_solve_opts
// (include/lpr_engine.h) and DESIGN.md section 4b "Control"; each row names the sentence it comes
// from.  They are never generated from primal_plan itself.
//   c++ -std=c++17 -fsanitize=address,undefined tools/primal_plan_check.cpp && ./a.out
#include <cstdio>
#include <cstring>

#include "../lpr_381_group_v22_amd/csrc/primal_plan.hpp"

using namespace lpr;

namespace {

struct Shape { int rows, cols; };  // ld = cols rounded up to 16 doubles

constexpr Shape kOneRow{1, 10};
constexpr Shape kSmallFits{1024, 2032};   // ld 2048, 16 MB: the largest the small path takes
constexpr Shape kSmallTall{1025, 2032};   // one row too many for it; 16.8 MB
constexpr Shape kFused1MiB{32, 4096};     // ld too wide for small; exactly 1 MiB
constexpr Shape kOver1MiB{33, 4096};
constexpr Shape k80MiB{2560, 4096};       // exactly 80 MiB
constexpr Shape kOver80MiB{2561, 4096};
constexpr Shape kHeadline{4097, 12289};   // bench.py: m = 4096, n = 8192; 403 MB
constexpr Shape kWide{400, 40000};        // 128 MB, more than 32767 columns
constexpr Shape kSquare{4000, 4000};      // 128 MB, cols - rows = 0: no resident column
constexpr Shape kM8{9, 2000000};          // 144 MB, m = 8
constexpr Shape kM16{17, 1000000};        // 136 MB, m = 16

struct Want {
    PrimalPath path;
    int K;
    int tile;             // K-pivot paths only (0: not checked)
    int update_variant;   // one-pivot path only (-1: not checked)
    int condensed;        // two-stream only: 1 / 0 (-1: not checked)
    int buffers;          // two-stream only: 1 / 0 (-1: not checked)
    int spares;           // (0: not checked)
    OvForm form;          // always checked; the default is the form of variant bits 16..24 == 0
    bool poll_ahead = true;
};

struct Row {
    const char* from;  // the sentence of the documentation this row states
    Shape shape;
    int64_t max_pivots;
    int time_kernels, variant, block, hook;
    Want want;
};

OvForm form_with(void (*set)(OvForm&)) {
    OvForm f;
    set(f);
    return f;
}

const PrimalPath S = PrimalPath::Small, F = PrimalPath::Fused, T2 = PrimalPath::TwoStream,
                 IP = PrimalPath::InPlace, P1 = PrimalPath::OnePivot;

const Row kRows[] = {
    // ---- the shapes, default options ----------------------------------------------------------
    {"rows = 1: no constraint row, never the small path (it needs rows >= 2); up to kFusedBytes one "
     "k_pivot_fused launch per pivot", kOneRow, 0, 0, 0, 0, 0, {F, 1, 0, -1, -1, -1, 0, {}}},
    {"rows = 1 with block 16: 'pivots decided ahead' need a constraint row, K = 1; block >= 2 rules "
     "the fused path out", kOneRow, 0, 0, 0, 16, 0, {P1, 1, 0, -1, -1, -1, 0, {}}},
    {"DESIGN 4b: cache-resident path, R <= 1024 and ld <= 2048, the default wherever it fits",
     kSmallFits, 0, 0, 0, 0, 0, {S, 16, 0, -1, -1, -1, 0, {}}},
    {"1025 rows do not fit the small path; above 1 MiB and up to 80 MiB: heads then in-place sweep, "
     "block 0 = auto (16), 8-row chunks", kSmallTall, 0, 0, 0, 0, 0, {IP, 16, kTile8, -1, -1, -1, 0, {}}},
    {"ld 4096 is too wide for small; a tableau of exactly kFusedBytes (1 MiB) is still fused",
     kFused1MiB, 0, 0, 0, 0, 0, {F, 1, 0, -1, -1, -1, 0, {}}},
    {"one row above 1 MiB: the K-pivot path, in place", kOver1MiB, 0, 0, 0, 0, 0,
     {IP, 16, kTile8, -1, -1, -1, 0, {}}},
    {"exactly kOverlapBytes (80 MiB) is still heads-then-sweep: the two-stream path runs ABOVE it",
     k80MiB, 0, 0, 0, 0, 0, {IP, 16, kTile8, -1, -1, -1, 0, {}}},
    {"above 80 MiB: two-stream overlap; 'by default a call with a budget of 1 024 pivots or more, or "
     "none, works on buffers that leave out the unit columns'; spares m / 8 - 1 = 319",
     kOver80MiB, 0, 0, 0, 0, 0, {T2, 16, kTile8, -1, 1, 1, 319, {}}},
    {"the headline size: two-stream, condensed, S = 4096 / 8 - 1 = 511 (DESIGN 4b)", kHeadline, 0, 0,
     0, 0, 0, {T2, 16, kTile8, -1, 1, 1, 511, {}}},
    // ---- opts.block: '0 auto (16), 1 one pivot per sweep, 2..16 that many' ------------------------
    {"block 1: one pivot per sweep, tile by size: the tallest row tile that still gives 256 CUs 8 "
     "workgroups each -- 8 column tiles x 81 (32 rows) = 648, x 161 = 1 288, x 321 (8 rows) = 2 568 "
     ">= 2 048: variant 1, serpentine (| 0x100)",
     kOver80MiB, 0, 0, 0, 1, 0, {P1, 1, 0, 0x101, -1, -1, 0, {}}},
    {"block 2", kOver80MiB, 0, 0, 0, 2, 0, {T2, 2, kTile8, -1, 1, 1, 0, {}}},
    {"block 16", kOver80MiB, 0, 0, 0, 16, 0, {T2, 16, kTile8, -1, 1, 1, 0, {}}},
    {"block 17: above the range, clipped to 16", kOver80MiB, 0, 0, 0, 17, 0,
     {T2, 16, kTile8, -1, 1, 1, 0, {}}},
    {"block -1: below the range, read as 1", kOver80MiB, 0, 0, 0, -1, 0,
     {P1, 1, 0, 0x101, -1, -1, 0, {}}},
    {"block 2 on a 1 MiB tableau: the K-pivots-per-sweep path was asked for explicitly", kFused1MiB,
     0, 0, 0, 2, 0, {IP, 2, kTile8, -1, -1, -1, 0, {}}},
    {"block 2 on a tableau that fits the small path: small is the default for block 0 only",
     kSmallFits, 0, 0, 0, 2, 0, {IP, 2, kTile8, -1, -1, -1, 0, {}}},
    // ---- opts.variant, low 16 bits ------------------------------------------------------------------
    {"variant 1: a k_update tile variant (index variant - 1 = 0), the one-pivot path", kOver80MiB, 0,
     0, 1, 0, 0, {P1, 1, 0, 0, -1, -1, 0, {}}},
    {"variant 11: k_update tile variant 10", kSmallTall, 0, 0, 11, 0, 0,
     {P1, 1, 0, 10, -1, -1, 0, {}}},
    {"variant 0x0106: tile variant 5 with the serpentine bit", kOver80MiB, 0, 0, 0x0106, 0, 0,
     {P1, 1, 0, 0x105, -1, -1, 0, {}}},
    {"variant 1 on a tableau that fits small / fused: still the one-pivot path", kFused1MiB, 0, 0, 1,
     0, 0, {P1, 1, 0, 0, -1, -1, 0, {}}},
    {"0x20xx forces the cache-resident path where it fits, whatever the block", kSmallFits, 0, 0,
     0x2000, 4, 0, {S, 16, 0, -1, -1, -1, 0, {}}},
    {"0x20xx where it does not fit: 'any other non-zero value' -- the one-pivot path", kSmallTall, 0,
     0, 0x2000, 0, 0, {P1, 1, 0, 0x1fff, -1, -1, 0, {}}},
    {"0x3004: two-stream overlap, 4-row chunks, forced below 80 MiB too; forced: no buffers ahead of "
     "the call, the call itself is condensed (no budget)", kSmallTall, 0, 0, 0x3004, 0, 0,
     {T2, 16, kTile4, -1, 1, 0, 127, {}}},
    {"0x3008", kOver80MiB, 0, 0, 0x3008, 0, 0, {T2, 16, kTile8, -1, 1, 0, 0, {}}},
    {"0x3010: 16-row chunks", kOver80MiB, 0, 0, 0x3010, 0, 0, {T2, 16, kTile16, -1, 1, 0, 0, {}}},
    {"0x3024: 4-row chunks, two in flight", kOver80MiB, 0, 0, 0x3024, 0, 0,
     {T2, 16, kTile4x2, -1, 1, 0, 0, {}}},
    {"0x3028: 8-row chunks, two in flight; on a tableau that fits small: forced all the same",
     kSmallFits, 0, 0, 0x3028, 0, 0, {T2, 16, kTile8x2, -1, 1, 0, 0, {}}},
    {"0x4008: heads then in-place sweep, forced above 80 MiB", kOver80MiB, 0, 0, 0x4008, 0, 0,
     {IP, 16, kTile8, -1, -1, -1, 0, {}}},
    {"0x5008: a retired form, accepted as an alias of 0x3008", kSmallTall, 0, 0, 0x5008, 0, 0,
     {T2, 16, kTile8, -1, 1, 0, 0, {}}},
    {"0x6008 with block 12: alias of 0x4008, 'now runs `block` pivots per sweep, where it used to cap "
     "them at 8'", kOver80MiB, 0, 0, 0x6008, 12, 0, {IP, 12, kTile8, -1, -1, -1, 0, {}}},
    {"0x7ffe forces the fused path, above 1 MiB too", kSmallTall, 0, 0, 0x7ffe, 0, 0,
     {F, 1, 0, -1, -1, -1, 0, {}}},
    {"0x7fff forces the two-kernel one-pivot path, tile by size (4 column tiles x 257 (4 rows) = "
     "1 028, x 513 (2 rows) = 2 052 >= 2 048: variant 9 | 0x100)",
     kSmallTall, 0, 0, 0x7fff, 0, 0, {P1, 1, 0, 0x109, -1, -1, 0, {}}},
    {"0x7fff on a tableau that fits small", kSmallFits, 0, 0, 0x7fff, 0, 0,
     {P1, 1, 0, 0x109, -1, -1, 0, {}}},
    // ---- opts.time_kernels ----------------------------------------------------------------------------
    {"time_kernels 'launch eagerly and bracket rank-1 update / sweep launches': no fused path; by "
     "size the K-pivot path in place", kFused1MiB, 0, 1, 0, 0, 0, {IP, 16, kTile8, -1, -1, -1, 0, {}}},
    {"time_kernels does not keep a tableau off the small path", kSmallFits, 0, 1, 0, 0, 0,
     {S, 16, 0, -1, -1, -1, 0, {}}},
    // ---- bits 16..24, each alone ------------------------------------------------------------------------
    {"0x10000 diagnostic time stamps of the loop heads; the diagnostic build exists for the full "
     "layout only (the buffers still come by size)", kOver80MiB, 0, 0, 0x10000, 0, 0,
     {T2, 16, kTile8, -1, 0, 1, 0, form_with([](OvForm& f) { f.stamps = true; })}},
    {"0x20000 loop heads not confined to one XCD: memory-side hand-offs, nothing for the sweep to "
     "leave", kOver80MiB, 0, 0, 0x20000, 0, 0,
     {T2, 16, kTile8, -1, 1, 1, 0,
      form_with([](OvForm& f) { f.spread = true; f.no_l2 = true; f.avoid = 0; })}},
    {"0x40000 confined but hand-offs through the memory side", kOver80MiB, 0, 0, 0x40000, 0, 0,
     {T2, 16, kTile8, -1, 1, 1, 0, form_with([](OvForm& f) { f.no_l2 = true; f.avoid = 0; })}},
    {"0x80000 the sweep does not leave the heads' XCD to them", kOver80MiB, 0, 0, 0x80000, 0, 0,
     {T2, 16, kTile8, -1, 1, 1, 0, form_with([](OvForm& f) { f.avoid = 0; })}},
    {"0x100000 it does so only once this launch's heads have said where they are", kOver80MiB, 0, 0,
     0x100000, 0, 0, {T2, 16, kTile8, -1, 1, 1, 0, form_with([](OvForm& f) { f.avoid = 1; })}},
    {"0x200000 the heads wait on a device flag: synchronous polls, full layout only", kOver80MiB, 0,
     0, 0x200000, 0, 0,
     {T2, 16, kTile8, -1, 0, 1, 0, form_with([](OvForm& f) { f.heads_on_device = true; }), false}},
    {"0x400000 the sweep asks the heads' completion word: synchronous polls, full layout only",
     kOver80MiB, 0, 0, 0x400000, 0, 0,
     {T2, 16, kTile8, -1, 0, 1, 0, form_with([](OvForm& f) { f.sweep_on_device = true; }), false}},
    {"0x200000 | 0x400000: no poll-ahead, never condensed", kOver80MiB, 0, 0, 0x600000, 0, 0,
     {T2, 16, kTile8, -1, 0, 1, 0,
      form_with([](OvForm& f) { f.heads_on_device = true; f.sweep_on_device = true; }), false}},
    {"0x800000 every tile of the two-stream sweep non-temporal", kOver80MiB, 0, 0, 0x800000, 0, 0,
     {T2, 16, kTile8, -1, 1, 1, 0, form_with([](OvForm& f) { f.ic_tiles = false; })}},
    {"0x1000000 no 64-row tiles at the head of the queue", kOver80MiB, 0, 0, 0x1000000, 0, 0,
     {T2, 16, kTile8, -1, 1, 1, 0, form_with([](OvForm& f) { f.tall_tiles = false; })}},
    {"flag bits do not name a path: 0x20000 alone on a tableau that fits small stays small",
     kSmallFits, 0, 0, 0x20000, 0, 0,
     {S, 16, 0, -1, -1, -1, 0,
      form_with([](OvForm& f) { f.spread = true; f.no_l2 = true; f.avoid = 0; })}},
    {"flag bits beside a path: 0x4008 | 0x10000, the diagnostic heads in place", kSmallTall, 0, 0,
     0x14008, 0, 0,
     {IP, 16, kTile8, -1, -1, -1, 0, form_with([](OvForm& f) { f.stamps = true; })}},
    // ---- bits 25..26 and the pivot budget ---------------------------------------------------------------
    {"0x2000000: the two-stream path never uses the condensed working layout", kOver80MiB, 0, 0,
     0x2000000, 0, 0, {T2, 16, kTile8, -1, 0, 0, 0, {}}},
    {"0x4000000: 'it uses it whatever the size of the tableau or the length of the call'",
     kSmallTall, 1, 0, 0x4003008, 0, 0, {T2, 16, kTile8, -1, 1, 1, 0, {}}},
    {"a budget of 1 023 pivots stays on the full layout (the buffers still come by size)",
     kOver80MiB, 1023, 0, 0, 0, 0, {T2, 16, kTile8, -1, 0, 1, 0, {}}},
    {"a budget of 1 024 pivots or more is condensed", kOver80MiB, 1024, 0, 0, 0, 0,
     {T2, 16, kTile8, -1, 1, 1, 0, {}}},
    {"more than 32 767 columns: an entering candidate no longer packs into an int, full layout",
     kWide, 0, 0, 0, 0, 0, {T2, 16, kTile8, -1, 0, 0, 0, {}}},
    {"more than 32 767 columns, bit 26: still the full layout", kWide, 0, 0, 0x4000000, 0, 0,
     {T2, 16, kTile8, -1, 0, 0, 0, {}}},
    {"cols - rows < 1: no resident column, full layout", kSquare, 0, 0, 0, 0, 0,
     {T2, 16, kTile8, -1, 0, 0, 0, {}}},
    // ---- spare columns ---------------------------------------------------------------------------------------
    {"test hook LPR_TEST_OV_SPARES = 1", kOver80MiB, 0, 0, 0, 0, 1, {T2, 16, kTile8, -1, 1, 1, 1, {}}},
    {"the hook outside 1..4096 is ignored", kOver80MiB, 0, 0, 0, 0, 4097,
     {T2, 16, kTile8, -1, 1, 1, 319, {}}},
    {"m = 8: m / 8 - 1 = 0, at least one spare", kM8, 0, 0, 0, 0, 0, {T2, 16, kTile8, -1, 0, 0, 1, {}}},
    {"m = 16: m / 8 - 1 = 1", kM16, 0, 0, 0, 0, 0, {T2, 16, kTile8, -1, 0, 0, 1, {}}},
    {"m = 4096: 511, the 403 MB tableau condensed to 8 704 of its 12 304 columns", kHeadline, 0, 0,
     0x3008, 0, 0, {T2, 16, kTile8, -1, 1, 0, 511, {}}},
};

const char* name(PrimalPath p) {
    switch (p) {
        case PrimalPath::Small: return "small";
        case PrimalPath::Fused: return "fused";
        case PrimalPath::TwoStream: return "two-stream";
        case PrimalPath::InPlace: return "in-place";
        case PrimalPath::OnePivot: return "one-pivot";
    }
    return "?";
}

bool same(const OvForm& a, const OvForm& b) {
    return a.stamps == b.stamps && a.spread == b.spread && a.no_l2 == b.no_l2 &&
           a.avoid == b.avoid && a.heads_on_device == b.heads_on_device &&
           a.sweep_on_device == b.sweep_on_device && a.ic_tiles == b.ic_tiles &&
           a.tall_tiles == b.tall_tiles;
}

}  // namespace

int main() {
    // the numbers the documentation gives
    static_assert(kFusedBytes == (1u << 20) && kOverlapBytes == (80u << 20), "1 MiB, 80 MiB");
    static_assert(kDefaultBlock == 16 && kOvMax == 16 && kOvcMinPivots == 1024, "block, budget");
    static_assert(kVarSmall == 0x2000 && kVarTwoStream == 0x3000 && kVarInPlace == 0x4000 &&
                  kVarOneLaunchAlias == 0x5000 && kVarPerHeadAlias == 0x6000 &&
                  kVarFused == 0x7ffe && kVarOnePivot == 0x7fff, "path codes");
    static_assert(kTile4 == 0x04 && kTile8 == 0x08 && kTile16 == 0x10 && kTile4x2 == 0x24 &&
                  kTile8x2 == 0x28, "tile codes");
    static_assert(kVarStamps == 1 << 16 && kVarSpread == 1 << 17 && kVarNoL2 == 1 << 18 &&
                  kVarNoAvoid == 1 << 19 && kVarAvoidLate == 1 << 20 &&
                  kVarHeadsOnDevice == 1 << 21 && kVarSweepOnDevice == 1 << 22 &&
                  kVarNoIcTiles == 1 << 23 && kVarNoTallTiles == 1 << 24 &&
                  kVarNeverCondensed == 1 << 25 && kVarAlwaysCondensed == 1 << 26, "flag bits");
    int bad = 0, rows = 0;
    for (const Row& r : kRows) {
        lpr_solve_opts o;
        std::memset(&o, 0, sizeof o);
        o.max_pivots = r.max_pivots;
        o.time_kernels = r.time_kernels;
        o.variant = r.variant;
        o.block = r.block;
        const int ld = align_up(r.shape.cols, kLdAlign);
        const PrimalPlan p = primal_plan(o, r.shape.rows, r.shape.cols, ld, r.hook);
        const Want& w = r.want;
        const bool kp = w.path == PrimalPath::TwoStream || w.path == PrimalPath::InPlace;
        bool ok = p.path == w.path && p.K == w.K && same(p.form, w.form) &&
                  p.poll_ahead == w.poll_ahead;
        if (kp && w.tile) ok = ok && ov_tile_code(p.tile) == w.tile && p.tile == w.tile;
        if (w.update_variant >= 0) ok = ok && p.update_variant == w.update_variant;
        if (w.condensed >= 0) ok = ok && p.condensed == (w.condensed != 0);
        if (w.buffers >= 0) ok = ok && p.condensed_buffers == (w.buffers != 0);
        if (w.spares) ok = ok && p.spares == w.spares;
        // a plan off the two-stream path is never condensed
        if (p.path != PrimalPath::TwoStream) ok = ok && !p.condensed && !p.condensed_buffers;
        ++rows;
        if (!ok) {
            ++bad;
            std::printf("FAIL %d x %d variant 0x%x block %d budget %lld timed %d hook %d: got %s K %d "
                        "tile 0x%x update %#x condensed %d buffers %d spares %d ahead %d\n  (%s)\n",
                        r.shape.rows, r.shape.cols, (unsigned)r.variant, r.block,
                        (long long)r.max_pivots, r.time_kernels, r.hook, name(p.path), p.K,
                        (unsigned)p.tile, (unsigned)p.update_variant, (int)p.condensed,
                        (int)p.condensed_buffers, p.spares, (int)p.poll_ahead, r.from);
        }
    }
    std::printf("primal_plan_check: %d rows, %d failures\n", rows, bad);
    return bad ? 1 : 0;
}
