// knapsack_common.hpp -- definitions shared by knapsack_kernels.hip (device) and
// knapsack_engine.hip (C ABI driver) for menu option 5 (Program.cs:430-470).  Not part of the ABI.
#pragma once

#include "engine_common.hpp"

#include <algorithm>
#include <cmath>

namespace lpr {

// ---- 0/1 DP ----------------------------------------------------------------------------------
// A blocked pass owns kKnapTile output cells per workgroup and keeps kKnapHalo cells below them
// in LDS, so a block of items whose weights sum to S <= kKnapHalo is applied with one HBM read
// and one HBM write of the row.  (kKnapHalo + kKnapTile) int64 = 80 KiB: two workgroups per CU.
constexpr int kKnapTile = 4096;
constexpr int kKnapHalo = 6144;
constexpr int kKnapDpThreads = 256;
constexpr int kKnapDpCells = 4;  // cells per thread per chunk: 4 LDS reads in flight per barrier
constexpr int kKnapDpChunk = kKnapDpThreads * kKnapDpCells;

// ---- branch-and-bound ------------------------------------------------------------------------
enum : int32_t { kKnapFractional = 0, kKnapPruned = 1, kKnapIntegral = 2, kKnapInfeasible = 3 };
constexpr int kKnapMaxItems = 8192;
constexpr int kKnapEvalWaves = 4;  // nodes per k_knap_eval workgroup (one wave each)

// incumbent, kept on the device across levels
struct KnapInc {
    int64_t z;      // Z* (valid when found)
    int32_t found;
    int32_t stop;   // rank position where its greedy walk stopped (n: took every free item)
    int64_t gid;    // its record index
};
// the one record the host reads per level
struct KnapLevel {
    int64_t next_width;  // children to evaluate next (2 x branched parents)
    int64_t z;
    int32_t found;
    int32_t pad;
};
// node log of a narrated solve (structure of arrays, record index = evaluation order)
struct KnapLog {
    int64_t cap;
    int32_t *par, *br, *st, *kp;
    double* bd;
    int64_t* V;
};

void knap_launch_dp_block(hipStream_t s, const int64_t* in, int64_t* out, int64_t cells,
                          const int32_t* w, const int32_t* v, int j0, int j1, int S);
void knap_launch_dp_stream(hipStream_t s, const int64_t* in, int64_t* out, int64_t cells,
                           int64_t w, int64_t v, int num_cus);
void knap_launch_eval(hipStream_t s, const uint64_t* nodes, int nw, int n, int64_t C,
                      const int64_t* w, const int64_t* v, int64_t W, int32_t* st, int32_t* kp,
                      int32_t* stop, int64_t* V, double* bd);
void knap_launch_level(hipStream_t s, int64_t W, int64_t base, const uint64_t* nodes, int nw,
                       const int32_t* par, const int32_t* br, int32_t* st, const int32_t* kp,
                       const int32_t* stop, const int64_t* V, const double* bd, int32_t* pos,
                       KnapInc* inc, uint64_t* inc_bits, KnapLevel* lvl, KnapLog log);
void knap_launch_children(hipStream_t s, int64_t W, int64_t base, const uint64_t* nodes, int nw,
                          const int32_t* pos, const int32_t* kp, uint64_t* next,
                          int32_t* next_par, int32_t* next_br);

// ---- what the single engine and the batch (knapsack_batch_*.hip) share --
// B&B inputs: integral doubles, 1 <= w <= 2^31-1, 0 <= v <= 2^31-1
inline bool knap_integral_in(double x, double lo) {
    return std::isfinite(x) && x == std::floor(x) && x >= lo && x <= 2147483647.0;
}
// The items of one instance; `where` opens the message ("call" or "call: instance k").
inline bool knap_items_ok(const char* where, const double* weights, const double* values,
                          int32_t n) {
    for (int32_t i = 0; i < n; ++i) {
        if (!knap_integral_in(weights[i], 1.0)) {
            set_error("%s: weights[%d] = %.17g is not an integer in 1..2^31-1", where, i,
                      weights[i]);
            return false;
        }
        if (!knap_integral_in(values[i], 0.0)) {
            set_error("%s: values[%d] = %.17g is not an integer in 0..2^31-1", where, i,
                      values[i]);
            return false;
        }
    }
    return true;
}
// rank[p] = original index of rank position p: v/w descending as exact cross products (< 2^62),
// ties to the lower original index.  ow, ov: n words of working space (the items as integers).
inline void knap_rank_items(const double* weights, const double* values, int n, uint64_t* ow,
                            uint64_t* ov, int32_t* rank) {
    for (int i = 0; i < n; ++i) {
        ow[i] = (uint64_t)weights[i];
        ov[i] = (uint64_t)values[i];
        rank[i] = i;
    }
    std::sort(rank, rank + n, [&](int32_t i, int32_t j) {
        const uint64_t a = ov[i] * ow[j], b = ov[j] * ow[i];
        return a != b ? a > b : i < j;
    });
}

#if defined(__HIPCC__)
__device__ __forceinline__ int64_t knap_pack(int lo, int hi) {
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t shfl_xor64(int64_t x, int m) {
    return knap_pack(__shfl_xor((int)x, m, kWave), __shfl_xor((int)(x >> 32), m, kWave));
}
__device__ __forceinline__ int64_t shfl_up64(int64_t x, int d) {
    return knap_pack(__shfl_up((int)x, d, kWave), __shfl_up((int)(x >> 32), d, kWave));
}
__device__ __forceinline__ int64_t shfl64(int64_t x, int lane) {
    return knap_pack(__shfl((int)x, lane, kWave), __shfl((int)(x >> 32), lane, kWave));
}
__device__ __forceinline__ int64_t wave_sum64(int64_t x) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) x += shfl_xor64(x, m);
    return x;
}
__device__ __forceinline__ int64_t wave_scan64(int64_t x, int lane) {  // inclusive
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int64_t y = shfl_up64(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// What the relaxation of one node gives.
struct KnapEval {
    int32_t st;    // kKnapFractional / kKnapIntegral / kKnapInfeasible
    int32_t kp;    // the critical item's rank position, -1 when there is none to report
    int32_t stop;  // where the greedy walk stopped (n: it took every free item)
    int64_t V;
    double bd;
};
// The three roundings of the bound, spelled once: q = R / w_k (IEEE), t = v_k * q, V + t.
__device__ __forceinline__ double knap_bound(int64_t R, int64_t V, int64_t wk, int64_t vk) {
    const double q = ieee_div((double)R, (double)wk);
    const double t = (double)vk * q;
    return (double)V + t;
}
__device__ __forceinline__ KnapEval knap_eval_close(int n, int k, int64_t R, int64_t V,
                                                    int64_t wk, int64_t vk) {
    if (k < 0 || R == 0) return KnapEval{kKnapIntegral, -1, k < 0 ? n : k, V, (double)V};
    return KnapEval{kKnapFractional, k, k, V, knap_bound(R, V, wk, vk)};
}
// One wave evaluates one node: F1 / F0 are its bitmaps over rank positions (nw words each), w, v
// the items in rank order (any integer type up to 2^31-1).  Every lane gets the result.
template <class Item>
__device__ __forceinline__ KnapEval knap_eval_wave(const uint64_t* F1, const uint64_t* F0, int nw,
                                                   int n, int64_t C, const Item* w, const Item* v,
                                                   int lane) {
    int64_t w1 = 0, v1 = 0;
    for (int c = 0; c < nw; ++c) {
        const int p = c * kWave + lane;
        if (p < n && ((F1[c] >> lane) & 1ull)) {
            w1 += (int64_t)w[p];
            v1 += (int64_t)v[p];
        }
    }
    w1 = wave_sum64(w1);
    v1 = wave_sum64(v1);
    int64_t R = C - w1, V = v1;
    if (R < 0) return KnapEval{kKnapInfeasible, -1, n, 0, 0.0};
    int k = -1;
    for (int c = 0; c < nw; ++c) {
        const int p = c * kWave + lane;
        const bool fr = p < n && !(((F1[c] | F0[c]) >> lane) & 1ull);
        const int64_t fw = fr ? (int64_t)w[p] : 0, fv = fr ? (int64_t)v[p] : 0;
        const int64_t pw = wave_scan64(fw, lane);
        // the first free item whose weight exceeds what is left after the free items before it
        const uint64_t hit = __ballot(fr && pw > R);
        if (hit) {
            const int kl = __builtin_ctzll(hit);
            R -= shfl64(pw - fw, kl);
            V += wave_sum64(lane < kl ? fv : 0);
            k = c * kWave + kl;
            break;
        }
        R -= shfl64(pw, kWave - 1);
        V += wave_sum64(fv);
    }
    return knap_eval_close(n, k, R, V, k < 0 ? 1 : (int64_t)w[k], k < 0 ? 0 : (int64_t)v[k]);
}
#endif  // __HIPCC__

}  // namespace lpr
