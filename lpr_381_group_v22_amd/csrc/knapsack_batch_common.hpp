// knapsack_batch_common.hpp -- definitions shared by the knapsack batch:
// knapsack_batch_engine.hip (host) and knapsack_batch_kernels.hip.  Not part of the ABI
// (include/lpr_engine.h is).
#pragma once

#include "batch_common.hpp"
#include "knapsack_common.hpp"

namespace lpr {

constexpr int64_t kKnapBatchDefaultCap = 1024;         // node_cap NULL or <= 0
constexpr int64_t kKnapBatchMaxCap = (int64_t)1 << 22; // the single engine's default
// lpr_knap_batch_dp: an instance needs capacity + 1 int64 cells; above this many it is refused
// (form H keeps two global rows of them) and goes through lpr_knap_dp alone.
constexpr int64_t kKnapBatchDpMaxCells = (int64_t)1 << 22;
// DP chunk: cells per lane read before any lane writes (NT * kKnapBatchDpCells cells per chunk).
constexpr int kKnapBatchDpCells = 4;
// Form-H DP: cell updates one instance may perform per launch (whole items; at least one).
constexpr int64_t kKnapBatchDpWork = (int64_t)1 << 26;

// Nodes an instance may evaluate per launch, by form, checked at level boundaries (a level is
// never split, so one launch evaluates at most chunk - 1 + node_cap nodes of an instance).
constexpr int kKnapBatchChunk[kNumForms] = {4096, 16384, 4096};
static_assert(sizeof(kKnapBatchChunk) / sizeof(int) == kNumForms, "one chunk per form");

// ---- footprint (next to batch_footprint: the bytes batch_pick_form sees) -----------------------
// A node of the frontier is two bitmaps over rank positions (F1, F0: nw words each) and its
// parent's record index; there are two frontier buffers of node_cap nodes.  The evaluation of a
// level keeps V (int64), the bound (double), the stop position and the status per node.  The
// ranked items are kept as 32-bit words (w, v <= 2^31 - 1).
inline int knap_words(int n) { return (n + kWave - 1) / kWave; }
inline size_t knap_batch_node_bytes(int n) {
    return 2 * ((size_t)2 * knap_words(n) * sizeof(uint64_t) + sizeof(int32_t)) +
           (sizeof(int64_t) + sizeof(double) + 2 * sizeof(int32_t));
}
inline size_t knap_batch_items_bytes(int n) { return (size_t)n * 2 * sizeof(uint32_t); }
inline size_t knap_batch_footprint(int n, int64_t node_cap) {
    return (size_t)node_cap * knap_batch_node_bytes(n) + knap_batch_items_bytes(n);
}

// The node storage of one instance: node_cap * knap_batch_node_bytes(n) bytes, in LDS (W, G) or
// in the instance's slice of the global slab (H, and the frontier a W / G instance parks there
// between launches).  64-bit arrays first, so every array is aligned where the block is.
struct KnapStore {
    int64_t* V;
    double* bd;
    uint64_t* bits[2];
    int32_t* par[2];
    int32_t* stop;
    int32_t* st;
};
__host__ __device__ inline KnapStore knap_store_at(void* base, int nw, int64_t cap) {
    KnapStore s;
    s.V = reinterpret_cast<int64_t*>(base);
    s.bd = reinterpret_cast<double*>(s.V + cap);
    s.bits[0] = reinterpret_cast<uint64_t*>(s.bd + cap);
    s.bits[1] = s.bits[0] + cap * 2 * nw;
    s.par[0] = reinterpret_cast<int32_t*>(s.bits[1] + cap * 2 * nw);
    s.par[1] = s.par[0] + cap;
    s.stop = s.par[1] + cap;
    s.st = s.stop + cap;
    return s;
}

// One instance, in device memory.  The host owns the offsets and resets the rest at every solve;
// a launch updates the search state when it ends.
struct KnapBatchDesc {
    int64_t s_off;      // node storage: bytes into the slab (a multiple of 8)
    int64_t item_off;   // items: the ranked and the original arrays are packed by n
    int64_t bits_off;   // incumbent bitmaps: 2 * nw words at inc_bits + bits_off
    int64_t log_off;    // node records: narrate entries at every log array + log_off
    int64_t C;
    int64_t cap;        // node_cap
    int64_t evaluated;  // nodes evaluated so far = record index of the level's first node
    int64_t width;      // nodes of the level to evaluate next, in buffer `cur`
    int64_t widest;
    int64_t inc_z;      // Z* (valid when inc_found)
    int64_t inc_gid;    // the incumbent's record index
    int64_t dp_row;     // form-H DP: two rows of C + 1 cells at rows + dp_row
    int32_t n, nw;
    int32_t narrate;    // records kept
    int32_t levels;
    int32_t cur;        // the buffer the level to evaluate next is in
    int32_t status;     // kRunning, LPR_OK_OPTIMAL or LPR_BB_NODE_CAP
    int32_t inc_found;
    int32_t inc_stop;   // where the incumbent's greedy walk stopped
    int32_t dp_item;    // form-H DP: the next item
    int32_t dp_cur;     // ... and the row that holds the values so far
};

// What the kernels get besides the descriptors.
struct KnapBatchBufs {
    KnapBatchDesc* desc;
    unsigned char* slab;
    const uint32_t *rw, *rv;  // ranked items
    const uint32_t *ow, *ov;  // items in input order (the DP applies them in that order)
    uint64_t* inc_bits;
    KnapLog log;              // cap unused: every instance has its own narrate
};

int knap_batch_launch(int form, hipStream_t s, const KnapBatchBufs& B, size_t slot_bytes,
                      const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out,
                      int chunk);
int knap_batch_launch_dp(int form, hipStream_t s, const KnapBatchBufs& B, size_t slot_bytes,
                         const int32_t* idx, int n_in, int64_t* rows, int64_t* best);

}  // namespace lpr
