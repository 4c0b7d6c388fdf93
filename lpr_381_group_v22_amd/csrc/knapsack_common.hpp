// knapsack_common.hpp -- definitions shared by knapsack_kernels.hip (device) and
// knapsack_engine.hip (C ABI driver) for menu option 5 (Program.cs:430-470).  Not part of the ABI.
#pragma once

#include "engine_common.hpp"

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

}  // namespace lpr
