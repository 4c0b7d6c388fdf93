// primal_plan.hpp -- which path lpr_primal_solve takes for given options on a given shape, decided
// in ONE place: the names of every value of lpr_solve_opts::variant, the size thresholds, and
// primal_plan(), a pure function of the options, three integers and one test hook.  Every path
// stores the same bits, so a mistake here would only change the speed: tools/primal_plan_check.cpp
// holds the rule against a table written from the documentation of lpr_solve_opts.
// No HIP in here: a plain host compiler takes it.  Not part of the ABI (include/lpr_engine.h is).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/lpr_engine.h"

namespace lpr {

constexpr int kLdAlign = 16;  // tableau rows padded to 16 doubles = 128 B
inline int align_up(int x, int a) { return (x + a - 1) / a * a; }

// ---- opts.variant, low 16 bits: path + tile ------------------------------------------------------
constexpr int kVarPathMask = 0xff00, kVarTileMask = 0x00ff;
constexpr int kVarSmall = 0x2000;      // 0x20xx: the cache-resident path, where it fits
constexpr int kVarTwoStream = 0x3000;  // 0x30tr: out-of-place sweep, the next heads beside it
constexpr int kVarInPlace = 0x4000;    // 0x40tr: the heads of a block, then its sweep in place
// retired forms, kept as aliases: 0x50tr (the overlap in one launch) runs as 0x30tr, 0x60tr (one
// launch per loop head, K <= 8) as 0x40tr
constexpr int kVarOneLaunchAlias = 0x5000, kVarPerHeadAlias = 0x6000;
constexpr int kVarFused = 0x7ffe;     // forces one k_pivot_fused launch per pivot
constexpr int kVarOnePivot = 0x7fff;  // forces the two-kernel one-pivot path, default tile
constexpr int kVarUpdateTileEnd = 0x7000;  // any other v in 1 .. 0x6fff: one-pivot, k_update tile v - 1
// tr of 0x30tr / 0x40tr: rows per chunk of a sweep tile, + 0x20 = two chunks in flight
constexpr int kTile4 = 0x04, kTile8 = 0x08, kTile16 = 0x10, kTile4x2 = 0x24, kTile8x2 = 0x28;
inline int ov_tile_code(int tr) {  // anything else sweeps as kTile8
    return (tr == kTile4 || tr == kTile16 || tr == kTile4x2 || tr == kTile8x2) ? tr : kTile8;
}
// ---- bits 16..24: placement of the loop heads / order of the sweep (K-pivot paths) ---------------
constexpr int kVarStamps = 0x10000;         // diagnostic time stamps of the loop heads
constexpr int kVarSpread = 0x20000;         // loop heads not confined to one XCD
constexpr int kVarNoL2 = 0x40000;           // confined, but hand-offs through the memory side
constexpr int kVarNoAvoid = 0x80000;        // the sweep does not leave the heads' XCD to them
constexpr int kVarAvoidLate = 0x100000;     // it does so by this launch's word only (no hint)
constexpr int kVarHeadsOnDevice = 0x200000; // heads wait for the previous sweep on a device flag
constexpr int kVarSweepOnDevice = 0x400000; // the sweep asks the heads' completion word itself
constexpr int kVarNoIcTiles = 0x800000;     // every tile of the two-stream sweep non-temporal
constexpr int kVarNoTallTiles = 0x1000000;  // no 64-row tiles at the head of its queue
// ---- bits 25..26: the condensed working layout of the two-stream path ----------------------------
constexpr int kVarNeverCondensed = 0x2000000, kVarAlwaysCondensed = 0x4000000;

// ---- limits of the kernels (each file includes this header for its own) --------------------------
// small_kernels.hip: pivots per block, rows (one per lane), padded columns (one pair per lane),
// dynamic LDS of the block's factor columns
constexpr int kSmallK = 16, kSmallMaxR = 1024, kSmallMaxLd = 2048;
constexpr size_t kSmallLdsBytes = (size_t)140 << 10;
inline bool small_fits(int rows, int ld) {
    return rows >= 2 && rows <= kSmallMaxR && ld <= kSmallMaxLd &&
           (size_t)kSmallK * (size_t)align_up(rows, 16) * sizeof(double) <= kSmallLdsBytes;
}
// overlap_kernels.hip: pivots per block and head workgroups (upper bounds), threads per workgroup
constexpr int kOvMax = 16, kOvGroups = 64, kOvNT = 256;

// ---- thresholds ------------------------------------------------------------------------------------
// Up to kFusedBytes a tableau too wide for the small path takes one k_pivot_fused launch per pivot,
// ping-pong between T and T2.  (round 2, pivots/s K-pivot path vs that one: m = 256 (1.6 MB) 143.6 k
// vs 137.9 k, m = 320 141.9 k vs 121.0 k, m = 512 137.7 k vs 99.7 k.  Below ~1 MB a solve is a few
// dozen pivots and the start-up of the K-pivot path -- prologue, a fill and a drain step -- counts.)
constexpr size_t kFusedBytes = (size_t)1 << 20;
// Above kOverlapBytes the K-pivot path takes the two-stream form.  (round 2, tools/size_sweep.sh:
// with 8-10 us loop heads it wins from ~80 MB: 67 MB 99.6 k vs 104.2 k pivots/s for
// heads-then-sweep, 101 MB 98.7 k vs 92.2 k, 227 MB 93.6 k vs 78.6 k)
constexpr size_t kOverlapBytes = (size_t)80 << 20;
constexpr int kDefaultBlock = 16;  // opts.block == 0
// A call with a pivot budget below kOvcMinPivots stays on the full layout: condensing and expanding
// cost one pass over the tableau each (the measured break-even).
constexpr int64_t kOvcMinPivots = 1024;

inline size_t tableau_bytes(int rows, int ld) { return (size_t)rows * ld * sizeof(double); }

// Spare columns of the condensed layout: an omitted variable that leaves takes one, and when none
// is left the driver expands and condenses again.  m / 8 - 1 (255 .. 4095 measured at
// m = 4096; 511 makes the buffers 17 column strips of the sweep exactly): a narrower sweep also
// leaves the heads beside it more of the chip, which outweighs expanding and condensing again every
// few hundred pivots.  hook: the value of LPR_TEST_OV_SPARES (1..4096 holds; anything else: none).
inline int ovc_spares(int rows, int hook) {
    if (hook >= 1 && hook <= 4096) return hook;
    const int s = (rows - 1) / 8 - 1;
    return s < 1 ? 1 : s;
}
// physical width of the condensed buffers
inline int ovc_width(int rows, int cols, int spares) {
    return align_up(cols - rows + spares + 1, kLdAlign);
}
// can this shape use the condensed layout at all, with `spares` spare columns?
inline bool ovc_fits(int rows, int cols, int spares) {
    const int nres = cols - rows;
    if (rows < 2 || nres < 1 || spares < 1) return false;
    // an entering candidate is {original column << 16 | slot} in a non-negative int
    if (cols > 32767) return false;
    const long Wp = ovc_width(rows, cols, spares);
    // every column pair has a lane of its own in the loop heads
    return Wp <= 32767 && Wp / 2 <= (long)kOvGroups * kOvNT;
}

// One-pivot path, tile shape by size: the tallest row tile (more loads in flight per lane,
// pivot-row slice reused over more rows) that still gives the 256 CUs >= 8 workgroups each;
// measured on the 4097 x 12289 tableau TR=32 is the fastest (profiles/).  The serpentine sweep
// (bit 8) reverses the tile order on alternate pivots so the tail of one sweep is re-read from the
// 256 MiB Infinity Cache.
inline int default_update_variant(int rows, int ld) {
    const long ctiles = (ld / 2 + 255) / 256;
    const struct { int tr; int idx; } opts[] = {{32, 5}, {16, 0}, {8, 1}, {4, 8}, {2, 9}, {1, 10}};
    for (const auto& o : opts) {
        const long blocks = ctiles * ((rows + o.tr - 1) / o.tr);
        if (blocks >= 2048 || o.tr == 1) return o.idx | 0x100;
    }
    return 0x100;
}

// ---- the plan ----------------------------------------------------------------------------------------
enum class PrimalPath { Small, Fused, TwoStream, InPlace, OnePivot };

// How the launchers of overlap_kernels.hip put the heads and the sweep of a step on the device.
struct OvForm {
    bool stamps = false;  // the diagnostic build of the heads
    bool spread = false;  // one head workgroup per group, anywhere on the chip
    bool no_l2 = false;   // hand-offs between the heads through the memory side
    int avoid = 2;        // the sweep leaves the heads' XCD to them: 2 = by the previous launch's hint
                          // and this launch's word, 1 = by this launch's word only, 0 = never
    bool heads_on_device = false;  // heads follow their predecessor at once, wait on a device flag
    bool sweep_on_device = false;  // the sweep follows at once, asks the heads' completion word
    bool ic_tiles = true;    // tiles at both ends of the sweep's queue keep the default cache policy
    bool tall_tiles = true;  // 64-row tiles at the head of the queue
};

struct PrimalPlan {
    PrimalPath path = PrimalPath::OnePivot;
    int K = 1;               // pivots per sweep (res->block)
    int tile = kTile8;       // K-pivot paths: the sweep's tile code
    int update_variant = 0;  // one-pivot path: the k_update tile variant
    OvForm form;
    int spares = 1;          // condensed layout: spare columns
    bool condensed = false;  // two-stream: this call is eligible for the condensed layout
    bool condensed_buffers = false;  // two-stream: the handle gets its condensed buffers now
    bool poll_ahead = true;  // K-pivot driver: snapshots ahead of the queue's end
};

// What can fail at run time is the driver's: a two-stream plan whose second buffer cannot be had
// runs as InPlace (and is then neither condensed nor given condensed buffers).
inline PrimalPlan primal_plan(const lpr_solve_opts& o, int rows, int cols, int ld,
                              int spares_hook) {
    PrimalPlan p;
    int v = o.variant & 0xffff;
    if ((v & kVarPathMask) == kVarOneLaunchAlias) v = kVarTwoStream | (v & kVarTileMask);
    if ((v & kVarPathMask) == kVarPerHeadAlias) v = kVarInPlace | (v & kVarTileMask);
    const int path = v & kVarPathMask;
    const size_t bytes = tableau_bytes(rows, ld);

    OvForm& f = p.form;
    f.stamps = (o.variant & kVarStamps) != 0;
    f.spread = (o.variant & kVarSpread) != 0;
    f.no_l2 = f.spread || (o.variant & kVarNoL2) != 0;
    f.avoid = (f.no_l2 || (o.variant & kVarNoAvoid)) ? 0 : ((o.variant & kVarAvoidLate) ? 1 : 2);
    f.heads_on_device = (o.variant & kVarHeadsOnDevice) != 0;
    f.sweep_on_device = (o.variant & kVarSweepOnDevice) != 0;
    f.ic_tiles = (o.variant & kVarNoIcTiles) == 0;
    f.tall_tiles = (o.variant & kVarNoTallTiles) == 0;
    // (the opt-in forms whose kernels order themselves on the device keep the synchronous polls:
    // ov2_launch_step's consistency argument is made for the event form)
    p.poll_ahead = !f.heads_on_device && !f.sweep_on_device;
    p.spares = ovc_spares(rows, spares_hook);
    p.update_variant =
        (v > 0 && v < kVarUpdateTileEnd) ? v - 1 : default_update_variant(rows, ld);

    // the cache-resident path: the default for every tableau that fits, or forced
    if (small_fits(rows, ld) && (path == kVarSmall || (v == 0 && o.block == 0))) {
        p.path = PrimalPath::Small;
        p.K = kSmallK;
        return p;
    }
    // (opts.block >= 2 asks for the K-pivots-per-sweep path explicitly)
    if (!o.time_kernels && o.block < 2 && v != kVarOnePivot &&
        (v == kVarFused || (v == 0 && bytes <= kFusedBytes))) {
        p.path = PrimalPath::Fused;
        return p;
    }
    // any other non-zero variant names a one-pivot update kernel
    if (v != 0 && path != kVarTwoStream && path != kVarInPlace) return p;
    int k = o.block == 0 ? kDefaultBlock : o.block;
    if (k > kOvMax) k = kOvMax;
    if (k < 1 || rows < 2) k = 1;
    if (k == 1) return p;
    p.K = k;
    p.tile = path ? (v & kVarTileMask) : kTile8;
    // measured (tools/size_sweep.sh): up to ~80 MB the heads-then-sweep form is faster (9.1-9.6 us
    // per pivot), above it hiding the sweep behind the next heads wins
    const bool big = path == 0 && bytes > kOverlapBytes;
    if (path != kVarTwoStream && !big) {
        p.path = PrimalPath::InPlace;
        return p;
    }
    p.path = PrimalPath::TwoStream;
    const bool never = (o.variant & kVarNeverCondensed) != 0;
    const bool always = (o.variant & kVarAlwaysCondensed) != 0;
    const bool fits = ovc_fits(rows, cols, p.spares);
    const bool narrower = ovc_width(rows, cols, p.spares) < ld;
    // the buffers of the condensed layout come with the handle's first two-stream call by size (or
    // forced), whichever layout that call itself uses
    p.condensed_buffers = (big || always) && !never && fits && narrower;
    // the diagnostic build of the heads and the opt-in forms that order themselves on the device
    // exist for the full layout only
    p.condensed = !never && !f.stamps && p.poll_ahead && fits &&
                  (always || (!(o.max_pivots > 0 && o.max_pivots < kOvcMinPivots) && narrower));
    return p;
}

}  // namespace lpr
