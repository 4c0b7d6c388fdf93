// bb_batch_common.hpp -- definitions shared by the batched Branch & Bound (bb_batch_engine.hip,
// host) and its kernels (bb_batch_kernels.hip).  Not part of the ABI (include/lpr_engine.h is).
#pragma once

#include "batch_common.hpp"
#include "bb_narr_layout.hpp"

namespace lpr {

// The forms and their limits are those of the LP batch (BatchForm, batch_common.hpp; DESIGN.md
// sections 12 and 13).  The host picks one per IP by the footprint of its working pair at full
// depth: two tableaux of (R + c) x (C + c) doubles and the staged factor column of R + c doubles,
// c the node cap.  W and G keep the pair in LDS; H keeps it in the IP's slice of the global work
// slab and the factor column in LDS, for shapes at full depth up to kBatchMaxRowsH x
// kBatchMaxColsH.

// Node cap: <= 0 means the reference's 20 (:1038); more than kBBBatchMaxNodeCap is refused.
constexpr int kBBBatchDefaultNodeCap = 20;
constexpr int kBBBatchMaxNodeCap = 64;
// Pops per IP per launch, by form: a launch stays within a few milliseconds.
constexpr int kBBBatchChunk[kNumForms] = {32, 16, 4};
static_assert(sizeof(kBBBatchChunk) / sizeof(int) == kNumForms, "one chunk per form");
// Pivots one child LP may take before its IP ends with LPR_PIVOT_LIMIT (0 in the options): the
// `1 << 16` guard of bb_expand.
constexpr int kBBBatchMaxChildPivots = 1 << 16;
// Pivot-trace quads kept per IP when the caller passes trace_cap = 0.
constexpr int kBBBatchTraceDefault = 1024;

// Integers per node record (parent, kind, depth, var, status); two doubles (bound, z) go with them.
constexpr int kBBRecInts = 5;

// One IP of a batch, in device memory.  The host owns the offsets and the options; the kernels own
// the search state between launches.
struct BBBatchDesc {
    int64_t stack_off;  // doubles: node_cap + 2 slots of slot_n(), slot node_cap + 1 = the root
    int64_t work_off;   // doubles of the work slab (form H): two tableaux + the factor column
    int64_t x_off;      // nvars doubles: incumbent x, and as many of node scratch (decision values)
    int64_t rec_off;    // records: 1 + 2 node_cap of them
    int64_t pop_off;    // pop order: node_cap ids
    int64_t trace_off;  // trace_cap quads
    int64_t int_off;    // 2 (cols + node_cap) ints: basic-column keys and their sorted list
    int64_t stk_off;    // 2 (node_cap + 1) ints: the DFS stack's (record id, depth) per slot
    int64_t pivots;     // pivot-trace entries (exact; the trace keeps the first trace_cap)
    int64_t processed;  // branchCount (:1045)
    double best_z;      // optimalValue (:1024)
    int32_t rows, cols, nvars, node_cap, trace_cap;
    int32_t status;     // kRunning or LPR_OK_OPTIMAL / LPR_BB_NODE_CAP / LPR_PIVOT_LIMIT
    int32_t sp;         // nodes on the stack
    int32_t iteration;  // :1036
    int32_t nrec;       // node records
    int32_t found;      // an incumbent exists
    int32_t best_node;  // its record id, -1 if none
    int32_t enable_pruning;
    int32_t max_child_pivots;
    int32_t pad;
    __host__ __device__ int64_t slot_n() const {
        return (int64_t)(rows + node_cap) * (cols + node_cap);
    }
};

// Device buffers of a batch, passed by value to the kernels.
struct BBBatchBufs {
    BBBatchDesc* desc;
    double* stack;   // per IP (node_cap + 2) * slot_n doubles
    double* work;    // form H working pairs
    double* x;       // incumbent x, packed by nvars
    double* vals;    // decision values of the popped node, packed by nvars
    int32_t* rec_i;  // kBBRecInts per record
    double* rec_d;   // 2 per record
    int32_t* pops;
    int32_t* trace;  // 4 per quad
    int32_t* ints;
    int32_t* stk;
};

// What a narrated batch adds (the layout is stated in bb_narr_layout.hpp),
// passed by value to k_bb_batch_narr.  Records and pops are addressed with the IP's rec_off /
// pop_off; its pop values start at node_cap * x_off.
struct BBNarr {
    BBNarrDesc* desc;
    double* slab;        // child tableaux, compact per IP
    double* best;        // incumbent tableaux: slot_n doubles per IP
    int64_t* tab_off;    // per record
    int32_t* ntab;       // per record
    double* pop_z;       // per pop
    int32_t* pop_flags;  // per pop
    double* pop_vals;    // nvars per pop
};

// Doubles of LDS (or of the work slab) one IP needs: the working pair at full depth and the factor
// column.
inline size_t bb_batch_footprint(int rows, int cols, int node_cap) {
    const size_t r = (size_t)rows + node_cap, c = (size_t)cols + node_cap;
    return 2 * r * c + r;
}

// bb_batch_kernels.hip and, narrated, bb_batch_narr_kernels.hip: the launchers bb_batch_engine.hip
// calls
int bb_batch_launch(int form, hipStream_t s, const BBBatchBufs& B, const int32_t* idx_in,
                    int n_in, int32_t* idx_out, int32_t* n_out, int chunk, int slot_doubles,
                    int max_rows);
void bb_batch_launch_load(hipStream_t s, const BBBatchDesc* desc, int count, const double* src,
                          const int64_t* src_off, double* stack);
void bb_batch_launch_reset(hipStream_t s, const BBBatchBufs& B, int count);
int bb_batch_narr_launch(int form, hipStream_t s, const BBBatchBufs& B, const BBNarr& narr,
                         const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out,
                         int chunk, int slot_doubles, int max_rows);
void bb_batch_narr_launch_reset(hipStream_t s, const BBBatchBufs& B, const BBNarr& narr,
                                int count);

}  // namespace lpr
