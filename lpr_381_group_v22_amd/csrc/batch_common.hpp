// batch_common.hpp -- definitions shared by the batched primal simplex (batch_engine.hip, host)
// and its kernels (batch_body.hpp, instantiated by batch_kernels.hip and, traced, by
// batch_trace_kernels.hip), and what the four batch engines (LP, B&B: bb_batch_*,
// scenarios: sens_batch_*, cutting plane: cut_batch_*) have in common on the host: the forms and the rule that picks one, the
// running-list driver, the one form launcher (batch_launch, which asks raise_dynamic_lds of engine_common.hpp
// once per kernel instantiation) and the handle plumbing.  The device side of what
// they share is batch_device.hpp.  Not part of the ABI (include/lpr_engine.h is).
#pragma once

#include <cstdint>

namespace lpr {

// One record of a traced primal batch (lpr_batch_trace_*), in doubles,
// indices stored as doubles: record i of an LP is its state after i pivots,
//   [0] leavingRow of pivot i (1-based, PrimalSimplexSolver.cs:138)  [1] enteringCol of pivot i
//   T[rows x cols] row-major: the tableau after pivot i
// Record 0 is the tableau as built or uploaded, its header -1, -1.  LP k's records are at
// trace + trace_off[k], batch_trace_stride apart, the first trace_cap kept.  This part of the
// header needs no HIP: with LPR_BATCH_LAYOUT_ONLY defined a plain host compiler takes it
// (tools/batch_trace_check.cpp).
constexpr int64_t batch_trace_row() { return 0; }
constexpr int64_t batch_trace_col() { return 1; }
constexpr int64_t batch_trace_tab() { return 2; }
constexpr int64_t batch_trace_stride(int rows, int cols) {
    return batch_trace_tab() + (int64_t)rows * cols;
}
static_assert(batch_trace_stride(3, 4) == 14, "header, then the tableau");

// Where a traced batch keeps its records.
struct BatchTrace {
    double* slab;        // every LP's records
    const int64_t* off;  // per LP, doubles
    int32_t cap;         // records kept per LP; a record index >= cap is counted, not written
};

}  // namespace lpr

#ifndef LPR_BATCH_LAYOUT_ONLY

#include "engine_common.hpp"

#include <utility>

namespace lpr {

// Forms of one item (LP, IP, scenario batch) in a batch.  The host picks
// one per item by its LDS footprint; for an LP that is (rows * cols + rows) doubles: the tableau,
// compact, and the staged factor column.
enum BatchForm : int { kFormW = 0, kFormG = 1, kFormH = 2, kNumForms = 3 };

// Every workgroup keeps kBatchWgScratch bytes of LDS for itself (the reduction slots).
constexpr size_t kBatchWgScratch = (size_t)1 << 10;
// W: one wave per LP, four LPs per 256-lane workgroup, each in a quarter of the 64 KiB a
// workgroup gets without the dynamic-LDS attribute.
constexpr size_t kBatchWgLdsW = (size_t)64 << 10;
constexpr size_t kBatchMaxLdsW = (kBatchWgLdsW - kBatchWgScratch) / 4;
// G: one workgroup per LP, the tableau in dynamic LDS: 160 KiB less the workgroup's scratch.
constexpr size_t kBatchMaxLdsG = ((size_t)160 << 10) - kBatchWgScratch;
// H: one workgroup per LP, the tableau in its slice of the global slab; factor column and pivot
// row staged in LDS.  The limit of DESIGN.md section 4c.
constexpr int kBatchMaxRowsH = 1024;
constexpr int kBatchMaxColsH = 2048;
// Pivots per LP per launch, by form: a launch stays within a few milliseconds, and no launch runs
// without a bound, even on an LP that cycles.
constexpr int kBatchChunk[kNumForms] = {256, 128, 16};
static_assert(sizeof(kBatchChunk) / sizeof(int) == kNumForms, "one chunk per form");
// Pivot-log pairs kept per LP when the caller passes log_cap = 0: 4 * (rows + cols), at most 4096.
constexpr int kBatchLogDefaultMax = 4096;

// One LP of a batch, in device memory.  The host owns the offsets; the kernels update status,
// iter and log_fill at the end of every launch.
struct BatchDesc {
    int64_t t_off;     // tableau: rows x cols row-major, compact, at slab + t_off (doubles)
    int64_t b_off;     // basis: rows - 1 entries at basis + b_off
    int64_t log_off;   // pivot log: log_cap (row, col) pairs at log + 2 * log_off
    int64_t x_off;     // solution: n entries at x + x_off (lpr_batch_solution_read)
    int64_t iter;      // pivots performed so far (exact; the log keeps the first log_cap)
    int64_t max_iter;  // this call stops when iter reaches it (<= 0: no limit)
    int32_t rows, cols;
    int32_t n;         // decision variables (columns 0 .. n-1 of ExtractSolution)
    int32_t log_cap;
    int32_t status;    // kRunning or an lpr_status
    int32_t log_fill;  // pairs kept: min(iter, log_cap)
};
// lpr_sens_batch_from_batch and lpr_bb_batch_from_batch read it through batch_view: a traced
// batch keeps its trace beside the descriptors (BatchTrace), not in them.
static_assert(sizeof(BatchDesc) == 72, "BatchDesc is 72 bytes");

// Inputs of lpr_batch_from_lps per LP: offsets into the packed arrays.
struct BatchBuild {
    int64_t obj_off;  // objective: n entries
    int64_t a_off;    // A: m x n row-major
    int64_t row_off;  // ncoef, relation, rhs: m entries
};

inline size_t batch_footprint(int rows, int cols) {  // doubles of LDS one LP needs
    return (size_t)rows * cols + rows;
}

// The form of one item by the bytes of LDS it needs: the smallest that holds it, or the forced
// one (opts.variant 1/2/3) if the item fits it.  allow_w = false: the engine builds no form W.
inline int batch_pick_form(size_t bytes, int variant, bool allow_w = true) {
    const bool fitW = allow_w && bytes <= kBatchMaxLdsW, fitG = bytes <= kBatchMaxLdsG;
    if (variant == 1 && fitW) return kFormW;
    if (variant == 2 && fitG) return kFormG;
    if (variant == 3) return kFormH;
    return fitW ? kFormW : (fitG ? kFormG : kFormH);
}

// hipMalloc of `elems` elements into *p unless an earlier one has failed (*rc); on failure *p is
// null and *rc is what oom(what, elems) returns after it has set the message.
template <class T, class Oom>
void dev_alloc(T** p, int64_t elems, const char* what, int* rc, Oom oom) {
    if (*rc != LPR_OK_OPTIMAL) return;
    if (hipMalloc(reinterpret_cast<void**>(p), (size_t)elems * sizeof(T)) != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        *rc = oom(what, elems);
    }
}

// The running lists of a batch and the launch rounds over them.  The items still running are
// listed per form, one contiguous range per form in the `in` half of idx.  A round zeroes the
// counters, launches one bounded kernel per non-empty form (W, G, H) -- an item that is still
// running when its chunk is used up appends itself to the `out` range of its form and counts
// itself -- reads the counters into pinned memory, synchronises and swaps in and out.  The rounds
// end when no item is left.
struct BatchRunLists {
    int32_t* idx = nullptr;         // 2 x count: the running lists, in and out, per form
    int32_t* counters = nullptr;    // kNumForms running counts (device)
    int32_t* h_counters = nullptr;  // pinned
    int32_t count = 0;
    int32_t off[kNumForms] = {0, 0, 0}, live[kNumForms] = {0, 0, 0};

    template <class Oom>
    void alloc(int32_t n, int* rc, Oom oom) {
        count = n;
        dev_alloc(&idx, 2 * (int64_t)n, "running lists", rc, oom);
        dev_alloc(&counters, kNumForms, "counters", rc, oom);
        if (*rc == LPR_OK_OPTIMAL &&
            hipHostMalloc(&h_counters, kNumForms * sizeof(int32_t)) != hipSuccess)
            *rc = oom("counters", kNumForms);
    }
    void release() {
        hipFree(idx);
        hipFree(counters);
        if (h_counters) hipHostFree(h_counters);
        idx = counters = h_counters = nullptr;
    }
    // The host lists into the `in` half.  The engine uploads its descriptors after this.
    int upload(hipStream_t s, const std::vector<int32_t> (&lists)[kNumForms]) {
        for (int f = 0, at = 0; f < kNumForms; ++f) {
            off[f] = at;
            live[f] = (int32_t)lists[f].size();
            if (live[f] > 0)
                LPR_HIP(hipMemcpyAsync(idx + at, lists[f].data(), (size_t)live[f] * sizeof(int32_t),
                                       hipMemcpyHostToDevice, s));
            at += live[f];
        }
        return LPR_OK_OPTIMAL;
    }
    // The rounds.  launch is int(int form, const int32_t* in, int n_in, int32_t* out,
    // int32_t* n_out); a launch that fails ends the rounds with its code.
    template <class Launch>
    int rounds(hipStream_t s, Launch launch, int* launches) {
        int32_t* in = idx;
        int32_t* out = idx + count;
        while (live[kFormW] + live[kFormG] + live[kFormH] > 0) {
            LPR_HIP(hipMemsetAsync(counters, 0, kNumForms * sizeof(int32_t), s));
            for (int f = 0; f < kNumForms; ++f) {
                if (live[f] == 0) continue;
                const int rc = launch(f, in + off[f], live[f], out + off[f], counters + f);
                if (rc != LPR_OK_OPTIMAL) return rc;
                ++*launches;
            }
            LPR_HIP(hipMemcpyAsync(h_counters, counters, kNumForms * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, s));
            LPR_HIP(hipStreamSynchronize(s));
            for (int f = 0; f < kNumForms; ++f) live[f] = h_counters[f];
            std::swap(in, out);
        }
        return LPR_OK_OPTIMAL;
    }
};

// hipGetLastError after a launch, as a return code and a message.
inline int launch_checked(const char* name) {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return LPR_OK_OPTIMAL;
    set_error("%s failed to launch: %s", name, hipGetErrorString(err));
    return LPR_DEVICE_ERROR;
}

// The launch of one form's kernel of any batch engine: n_in items (`noun`: "LPs", "IPs", ...) in
// 256-lane workgroups, four per workgroup in form W, one in forms G and H, with `lds` bytes of
// dynamic LDS; above 64 KiB the kernel first gets the attribute, attr_bytes, once per device.  The
// kernel is a template argument, so every instantiation has a mask of its own: one bit per device
// on which its attribute is set.  An empty list launches nothing.  noun = nullptr: `name` is the
// ABI call, and the message gives the LDS bytes in place of the count (the knapsack batch).
template <auto kKernel, class... Args>
int batch_launch(const char* name, const char* noun, int form, hipStream_t s, int n_in,
                 size_t lds, size_t attr_bytes, Args... args) {
    static unsigned long long mask = 0;
    if (n_in <= 0) return LPR_OK_OPTIMAL;
    if (lds > ((size_t)64 << 10)) {
        const int rc = raise_dynamic_lds(reinterpret_cast<const void*>(kKernel), attr_bytes,
                                         &mask);
        if (rc != LPR_OK_OPTIMAL) return rc;
    }
    hipLaunchKernelGGL(kKernel, dim3(form == kFormW ? (n_in + 3) / 4 : n_in), dim3(256), lds, s,
                       args...);
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return LPR_OK_OPTIMAL;
    if (noun)
        set_error("%s (form %d, %d %s) failed to launch: %s", name, form, n_in, noun,
                  hipGetErrorString(err));
    else
        set_error("%s: launch of form %d failed (%zu bytes of LDS): %s", name, form, lds,
                  hipGetErrorString(err));
    return LPR_DEVICE_ERROR;
}

// A batch handle leaves its engine's list of live ones (the *_destroy calls).
template <class H>
void unlist(std::vector<H*>& live, H* h) {
    for (size_t q = 0; q < live.size(); ++q)
        if (live[q] == h) {
            live.erase(live.begin() + q);
            break;
        }
}

// batch_engine.hip: what an engine that starts from a solved LP batch reads of it: its engine (null
// once orphaned, or with no handle), the descriptors' host mirror and the tableau slab
lpr_engine* batch_view(lpr_batch* b, const std::vector<BatchDesc>** desc, const double** slab);
// batch_engine.hip: what lpr_batch_trace_text reads besides: the trace slab, every LP's offset into
// it and the records kept per LP (0: the batch is not traced)
int32_t batch_trace_view(lpr_batch* b, const double** trace, const std::vector<int64_t>** off);

// batch_kernels.hip and, traced, batch_trace_kernels.hip: the launchers batch_engine.hip calls
int batch_launch_simplex(int form, hipStream_t s, BatchDesc* desc, double* slab, int32_t* basis,
                         int32_t* logs, const int32_t* idx_in, int n_in, int32_t* idx_out,
                         int32_t* n_out, int chunk, int slot_doubles, int max_rows, int max_cols);
int batch_trace_launch_simplex(int form, hipStream_t s, BatchDesc* desc, double* slab,
                               int32_t* basis, int32_t* logs, const int32_t* idx_in, int n_in,
                               int32_t* idx_out, int32_t* n_out, int chunk, int slot_doubles,
                               int max_rows, int max_cols, BatchTrace tr);
void batch_trace_launch_first(hipStream_t s, const BatchDesc* desc, int count, const double* slab,
                              BatchTrace tr);
void batch_launch_build(hipStream_t s, const BatchDesc* desc, const BatchBuild* bd, int count,
                        double* slab, int32_t* basis, const double* obj, const double* A,
                        const int32_t* ncoef, const int8_t* rel, const double* rhs,
                        const int8_t* is_max);
void batch_launch_extract(hipStream_t s, const BatchDesc* desc, int count, const double* slab,
                          double* x, double* z);

}  // namespace lpr

// Entry check of every call on a batch handle; noun names the kind of batch in the message.
#define LPR_LIVE_HANDLE(b, noun)                                                            \
    do {                                                                                    \
        if (!(b) || !(b)->eng) {                                                            \
            ::lpr::set_error(noun " handle is null or orphaned: its engine has been closed"); \
            return LPR_BAD_ARGUMENT;                                                        \
        }                                                                                   \
        LPR_HIP(hipSetDevice((b)->eng->device));                                            \
    } while (0)

#endif  // LPR_BATCH_LAYOUT_ONLY
