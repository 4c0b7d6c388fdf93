// bb_batch_engine.hip -- host side of the batched Branch & Bound (include/lpr_engine.h,
// lpr_bb_batch_*).  Every IP of a batch runs ExecuteBranchAndBound on the
// device; the host only picks each IP's form, relaunches the bounded search kernels while IPs are
// still running (BatchRunLists of batch_common.hpp) and copies results out.
#include "bb_batch_common.hpp"
#include "bb_narr_text_layout.hpp"
#include "text_common.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace lpr;

struct lpr_bb_batch {
    lpr_engine* eng = nullptr;
    int32_t count = 0;
    int32_t node_cap = 0;
    std::vector<BBBatchDesc> h_desc;  // host mirror, current after every create / run
    BBBatchBufs d{};                  // device buffers (d.work grows on demand)
    int64_t work_n = 0;               // doubles allocated at d.work
    BatchRunLists run;                // the running lists and their counters
    int64_t x_total = 0, rec_total = 0, trace_total = 0;
    bool ran = false;
    // narrated (lpr_bb_batch_narrate_reserve, section 23): narr.desc != nullptr
    BBNarr narr{};
    std::vector<BBNarrDesc> h_narr;  // host mirror, current after every reserve / run
    int64_t narr_n = 0;              // doubles of narr.slab
    bool narr_ran = false;           // a run since the last reserve
};

namespace {

int bbb_oom(const char* what, int64_t n, size_t elem) {
    set_error("lpr_bb_batch: cannot allocate %s (%lld elements, %.3f GB)", what, (long long)n,
              (double)n * (double)elem / 1e9);
    return LPR_OUT_OF_MEMORY;
}

void bbb_release_narr(lpr_bb_batch* b) {
    hipFree(b->narr.desc);
    hipFree(b->narr.slab);
    hipFree(b->narr.best);
    hipFree(b->narr.tab_off);
    hipFree(b->narr.ntab);
    hipFree(b->narr.pop_z);
    hipFree(b->narr.pop_flags);
    hipFree(b->narr.pop_vals);
    b->narr = BBNarr{};
    b->narr_n = 0;
    b->narr_ran = false;
}

void bbb_release_device(lpr_bb_batch* b) {
    bbb_release_narr(b);
    hipFree(b->d.desc);
    hipFree(b->d.stack);
    hipFree(b->d.work);
    hipFree(b->d.x);
    hipFree(b->d.vals);
    hipFree(b->d.rec_i);
    hipFree(b->d.rec_d);
    hipFree(b->d.pops);
    hipFree(b->d.trace);
    hipFree(b->d.ints);
    hipFree(b->d.stk);
    b->run.release();
    b->d = BBBatchBufs{};
    b->work_n = 0;
}

// A root of rows x cols with nvars decision columns whose shape at full depth stays within form H.
bool bbb_shape_ok(const char* where, int32_t k, int64_t rows, int64_t cols, int64_t nvars,
                  int node_cap) {
    if (rows < 1 || cols < 2 || nvars < 0 || nvars > cols - 1) {
        set_error("%s: IP %d has a %lld x %lld root with nvars=%lld; it needs rows >= 1, "
                  "cols >= 2 and 0 <= nvars <= cols - 1",
                  where, k, (long long)rows, (long long)cols, (long long)nvars);
        return false;
    }
    if (rows + node_cap > kBatchMaxRowsH || cols + node_cap > kBatchMaxColsH) {
        set_error("%s: IP %d has a %lld x %lld root, %lld x %lld at the full depth of node cap %d: "
                  "beyond the batch limit of %d x %d (form H); run it alone with lpr_bb_run",
                  where, k, (long long)rows, (long long)cols, (long long)(rows + node_cap),
                  (long long)(cols + node_cap), node_cap, kBatchMaxRowsH, kBatchMaxColsH);
        return false;
    }
    return true;
}

bool bbb_caps_ok(const char* where, int32_t node_cap, int32_t* cap_out, int32_t trace_cap,
                 int32_t* tcap_out) {
    const int32_t c = node_cap <= 0 ? kBBBatchDefaultNodeCap : node_cap;
    if (c > kBBBatchMaxNodeCap) {
        set_error("%s: node_cap %d is above the batch maximum of %d", where, node_cap,
                  kBBBatchMaxNodeCap);
        return false;
    }
    *cap_out = c;
    *tcap_out = trace_cap <= 0 ? kBBBatchTraceDefault : trace_cap;
    return true;
}

// Offsets and device memory for `count` IPs of the given shapes.  On failure nothing is left.
int bbb_alloc(lpr_engine* e, int32_t count, const std::vector<int32_t>& R,
              const std::vector<int32_t>& Cc, const std::vector<int32_t>& nv, int32_t node_cap,
              int32_t trace_cap, lpr_bb_batch** out) {
    lpr_bb_batch* b = new (std::nothrow) lpr_bb_batch();
    if (!b) return bbb_oom("handle", 1, sizeof(lpr_bb_batch));
    b->eng = e;
    b->count = count;
    b->node_cap = node_cap;
    try {
        b->h_desc.resize((size_t)count);
    } catch (...) {
        delete b;
        return bbb_oom("descriptors", count, sizeof(BBBatchDesc));
    }
    int64_t st = 0, x = 0, rec = 0, pop = 0, tr = 0, in = 0, stk = 0;
    for (int32_t k = 0; k < count; ++k) {
        BBBatchDesc& d = b->h_desc[(size_t)k];
        std::memset(&d, 0, sizeof d);
        d.rows = R[(size_t)k];
        d.cols = Cc[(size_t)k];
        d.nvars = nv[(size_t)k];
        d.node_cap = node_cap;
        d.trace_cap = trace_cap;
        d.stack_off = st;
        d.x_off = x;
        d.rec_off = rec;
        d.pop_off = pop;
        d.trace_off = tr;
        d.int_off = in;
        d.stk_off = stk;
        d.status = LPR_OK_OPTIMAL;  // not run yet: no search state
        d.best_node = -1;
        d.best_z = -INFINITY;
        st += (int64_t)(node_cap + 2) * d.slot_n();
        x += d.nvars;
        rec += 1 + 2 * node_cap;
        pop += node_cap;
        tr += trace_cap;
        in += 2 * (int64_t)(d.cols + node_cap);
        stk += 2 * (int64_t)(node_cap + 1);
    }
    b->x_total = x;
    b->rec_total = rec;
    b->trace_total = tr;
    auto one = [](int64_t n) { return std::max<int64_t>(n, 1); };
    int rc = LPR_OK_OPTIMAL;
    BBBatchBufs& D = b->d;
    // the message gives n entries of elem bytes each (one figure for buffers that go together)
    auto gb = [](int64_t n, size_t elem) {
        return [=](const char* what, int64_t) { return bbb_oom(what, n, elem); };
    };
    dev_alloc(&D.desc, count, "descriptors", &rc, gb(count, sizeof(BBBatchDesc)));
    dev_alloc(&D.stack, one(st),
              "DFS stack slab: (node_cap + 2) (rows + node_cap) (cols + node_cap) doubles per IP",
              &rc, gb(st, sizeof(double)));
    dev_alloc(&D.x, one(x), "incumbents", &rc, gb(2 * x, sizeof(double)));
    dev_alloc(&D.vals, one(x), "incumbents", &rc, gb(2 * x, sizeof(double)));
    const size_t rec_elem = kBBRecInts * sizeof(int32_t) + 2 * sizeof(double);
    dev_alloc(&D.rec_i, one(rec) * kBBRecInts, "node records", &rc, gb(rec, rec_elem));
    dev_alloc(&D.rec_d, one(rec) * 2, "node records", &rc, gb(rec, rec_elem));
    dev_alloc(&D.pops, one(pop), "pop orders", &rc, gb(pop, sizeof(int32_t)));
    dev_alloc(&D.trace, one(tr) * 4, "pivot traces", &rc, gb(tr, 4 * sizeof(int32_t)));
    dev_alloc(&D.ints, one(in), "scratch", &rc, gb(in + stk, sizeof(int32_t)));
    dev_alloc(&D.stk, one(stk), "scratch", &rc, gb(in + stk, sizeof(int32_t)));
    b->run.alloc(count, &rc,
                 [](const char* what, int64_t n) { return bbb_oom(what, n, sizeof(int32_t)); });
    if (rc == LPR_OK_OPTIMAL &&
        hipMemcpy(D.desc, b->h_desc.data(), (size_t)count * sizeof(BBBatchDesc),
                  hipMemcpyHostToDevice) != hipSuccess) {
        set_error("lpr_bb_batch: descriptor upload failed");
        rc = LPR_DEVICE_ERROR;
    }
    if (rc != LPR_OK_OPTIMAL) {
        bbb_release_device(b);
        delete b;
        return rc;
    }
    *out = b;
    return LPR_OK_OPTIMAL;
}

// The roots into their stack slots: src on the device, src_off[k] the start of root k there.
int bbb_load(lpr_bb_batch* b, const double* d_src, const std::vector<int64_t>& src_off) {
    hipStream_t s = b->eng->stream;
    int64_t* d_off = nullptr;
    if (hipMalloc(&d_off, (size_t)b->count * sizeof(int64_t)) != hipSuccess)
        return bbb_oom("root offsets", b->count, sizeof(int64_t));
    hipError_t err = hipMemcpyAsync(d_off, src_off.data(), (size_t)b->count * sizeof(int64_t),
                                    hipMemcpyHostToDevice, s);
    if (err == hipSuccess) {
        bb_batch_launch_load(s, b->d.desc, b->count, d_src, d_off, b->d.stack);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    hipFree(d_off);
    if (err != hipSuccess) {
        set_error("lpr_bb_batch: loading the roots failed: %s", hipGetErrorString(err));
        return LPR_DEVICE_ERROR;
    }
    return LPR_OK_OPTIMAL;
}

}  // namespace

namespace lpr {
void bb_batch_orphan(lpr_bb_batch* b) {  // lpr_engine_close
    bbb_release_device(b);
    b->eng = nullptr;
}
}  // namespace lpr

extern "C" {

// BranchAndBoundAdapter.SolveFromPrimal's set-up (:9-24) per IP, from host tableaux
int lpr_bb_batch_create(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                        const double* tableaux, const int32_t* nvars, int32_t node_cap,
                        int32_t trace_cap, lpr_bb_batch** out) {
    static const char* W = "lpr_bb_batch_create";
    if (!e || !out || count < 1 || !rows || !cols || !tableaux || !nvars) {
        set_error("%s: bad arguments (count=%d, or a null engine / handle / rows / cols / "
                  "tableaux / nvars)", W, count);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    int32_t cap = 0, tcap = 0;
    if (!bbb_caps_ok(W, node_cap, &cap, trace_cap, &tcap)) return LPR_BAD_ARGUMENT;
    std::vector<int32_t> R((size_t)count), Cc((size_t)count), nv((size_t)count);
    std::vector<int64_t> off((size_t)count);
    int64_t total = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (!bbb_shape_ok(W, k, rows[k], cols[k], nvars[k], cap)) return LPR_BAD_ARGUMENT;
        R[(size_t)k] = rows[k];
        Cc[(size_t)k] = cols[k];
        nv[(size_t)k] = nvars[k];
        off[(size_t)k] = total;
        total += (int64_t)rows[k] * cols[k];
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_bb_batch* b = nullptr;
    int rc = bbb_alloc(e, count, R, Cc, nv, cap, tcap, &b);
    if (rc != LPR_OK_OPTIMAL) return rc;
    double* d_src = nullptr;
    if (hipMalloc(&d_src, (size_t)total * sizeof(double)) != hipSuccess) {
        rc = bbb_oom("root upload", total, sizeof(double));
    } else if (hipMemcpy(d_src, tableaux, (size_t)total * sizeof(double),
                         hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: root upload failed", W);
        rc = LPR_DEVICE_ERROR;
    } else {
        rc = bbb_load(b, d_src, off);
    }
    hipFree(d_src);
    if (rc != LPR_OK_OPTIMAL) {
        bbb_release_device(b);
        delete b;
        return rc;
    }
    e->live_bb_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

// SolveFromPrimal (:9-24) per LP of a solved lpr_batch: FinalTableau (:11-14) device to device,
// SetNumVars(SolutionVector?.Count ?? InferNumVariables(finalTable)) (:20)
int lpr_bb_batch_from_batch(lpr_batch* lps, int32_t node_cap, int32_t trace_cap,
                            lpr_bb_batch** out) {
    static const char* W = "lpr_bb_batch_from_batch";
    const std::vector<BatchDesc>* bd = nullptr;
    const double* slab = nullptr;
    lpr_engine* e = batch_view(lps, &bd, &slab);
    if (!e || !out) {
        set_error("%s: the LP batch is null or orphaned (its engine has been closed), or a null "
                  "handle", W);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    int32_t cap = 0, tcap = 0;
    if (!bbb_caps_ok(W, node_cap, &cap, trace_cap, &tcap)) return LPR_BAD_ARGUMENT;
    const int32_t count = (int32_t)bd->size();
    std::vector<int32_t> R((size_t)count), Cc((size_t)count), nv((size_t)count);
    std::vector<int64_t> off((size_t)count);
    for (int32_t k = 0; k < count; ++k) {
        const BatchDesc& d = (*bd)[(size_t)k];
        if (d.status != LPR_OK_OPTIMAL && d.status != LPR_UNBOUNDED) {
            set_error("%s: LP %d has no FinalTableau (status %d: %s); \"Primal simplex has not "
                      "been solved yet.\" (BranchAndBoundAdapter.cs:11-14)",
                      W, k, d.status,
                      d.status == LPR_PIVOT_LIMIT ? "stopped at its pivot limit" : "not solved");
            return LPR_BAD_ARGUMENT;
        }
        const int32_t n = d.status == LPR_OK_OPTIMAL ? d.n : std::max(1, d.cols - 1);
        if (!bbb_shape_ok(W, k, d.rows, d.cols, n, cap)) return LPR_BAD_ARGUMENT;
        R[(size_t)k] = d.rows;
        Cc[(size_t)k] = d.cols;
        nv[(size_t)k] = n;
        off[(size_t)k] = d.t_off;
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_bb_batch* b = nullptr;
    int rc = bbb_alloc(e, count, R, Cc, nv, cap, tcap, &b);
    if (rc != LPR_OK_OPTIMAL) return rc;
    rc = bbb_load(b, slab, off);  // synchronous: the LP batch may go right after
    if (rc != LPR_OK_OPTIMAL) {
        bbb_release_device(b);
        delete b;
        return rc;
    }
    e->live_bb_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

int lpr_bb_batch_destroy(lpr_bb_batch* b) {
    if (!b) return LPR_BAD_ARGUMENT;
    if (b->eng) {
        hipSetDevice(b->eng->device);
        hipStreamSynchronize(b->eng->stream);
        bbb_release_device(b);
        unlist(b->eng->live_bb_batch, b);
    }
    delete b;
    return LPR_OK_OPTIMAL;
}

// ExecuteBranchAndBound (:1006-1233) for every IP, from its root
int lpr_bb_batch_run(lpr_bb_batch* b, const lpr_bb_batch_opts* opts, lpr_bb_batch_result* res) {
    static const char* W = "lpr_bb_batch_run";
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!res) {
        set_error("%s: null result", W);
        return LPR_BAD_ARGUMENT;
    }
    lpr_bb_batch_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (o.variant < 0 || o.variant > 3 || o.chunk < 0 || o.max_child_pivots < 0) {
        set_error("%s: variant %d (0 auto, 1 W, 2 G, 3 H) / chunk %d (>= 0) / max_child_pivots "
                  "%d (>= 0)", W, o.variant, o.chunk, o.max_child_pivots);
        return LPR_BAD_ARGUMENT;
    }
    std::memset(res, 0, sizeof *res);
    hipStream_t s = b->eng->stream;
    const int32_t count = b->count;
    std::vector<int32_t> lists[kNumForms];
    int slot[kNumForms] = {0, 0, 0};
    int max_rows = 0;
    int64_t work = 0;
    for (int32_t k = 0; k < count; ++k) {
        BBBatchDesc& d = b->h_desc[(size_t)k];
        d.enable_pruning = o.enable_pruning ? 1 : 0;
        d.max_child_pivots = o.max_child_pivots > 0 ? o.max_child_pivots : kBBBatchMaxChildPivots;
        const int64_t fp = (int64_t)bb_batch_footprint(d.rows, d.cols, d.node_cap);
        const int f = batch_pick_form((size_t)fp * sizeof(double), o.variant);
        lists[f].push_back(k);
        if (f == kFormH) {
            d.work_off = work;
            work += fp;
            max_rows = std::max(max_rows, d.rows + d.node_cap);
        } else {
            d.work_off = 0;
            slot[f] = std::max(slot[f], (int)((fp + 1) & ~1LL));
        }
    }
    if (work > b->work_n) {
        hipFree(b->d.work);
        b->d.work = nullptr;
        b->work_n = 0;
        if (hipMalloc(&b->d.work, (size_t)work * sizeof(double)) != hipSuccess)
            return bbb_oom("form H working pairs", work, sizeof(double));
        b->work_n = work;
    }
    int rc = b->run.upload(s, lists);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->d.desc, b->h_desc.data(), (size_t)count * sizeof(BBBatchDesc),
                           hipMemcpyHostToDevice, s));
    bb_batch_launch_reset(s, b->d, count);
    LPR_HIP(hipGetLastError());
    const bool narrated = b->narr.desc != nullptr;
    if (narrated) {
        bb_batch_narr_launch_reset(s, b->d, b->narr, count);
        LPR_HIP(hipGetLastError());
    }
    int launches = 0;
    rc = b->run.rounds(s, [&](int f, const int32_t* in, int n_in, int32_t* out, int32_t* n_out) {
        const int chunk = o.chunk > 0 ? o.chunk : kBBBatchChunk[f];
        if (narrated)
            return bb_batch_narr_launch(f, s, b->d, b->narr, in, n_in, out, n_out, chunk, slot[f],
                                        max_rows);
        return bb_batch_launch(f, s, b->d, in, n_in, out, n_out, chunk, slot[f], max_rows);
    }, &launches);
    if (rc != LPR_OK_OPTIMAL) return rc;
    if (narrated) {
        LPR_HIP(hipMemcpyAsync(b->h_narr.data(), b->narr.desc, (size_t)count * sizeof(BBNarrDesc),
                               hipMemcpyDeviceToHost, s));
        b->narr_ran = true;
    }
    LPR_HIP(hipMemcpyAsync(b->h_desc.data(), b->d.desc, (size_t)count * sizeof(BBBatchDesc),
                           hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    b->ran = true;
    for (const BBBatchDesc& d : b->h_desc) {
        res->done += d.status == LPR_OK_OPTIMAL;
        res->node_cap += d.status == LPR_BB_NODE_CAP;
        res->pivot_limit += d.status == LPR_PIVOT_LIMIT;
        res->pops += d.processed;
        res->pivots += d.pivots;
    }
    res->launches = launches;
    return LPR_OK_OPTIMAL;
}

// lpr_bb_result's fields (:1006-1233's outputs) per IP
int lpr_bb_batch_result_read(lpr_bb_batch* b, int32_t* status, int32_t* found, int64_t* processed,
                             int32_t* best_node, double* z, int64_t* pivots,
                             int64_t* nodes_created) {
    LPR_LIVE_HANDLE(b, "B&B batch");
    for (int32_t k = 0; k < b->count; ++k) {
        const BBBatchDesc& d = b->h_desc[(size_t)k];
        if (status) status[k] = d.status;
        if (found) found[k] = d.found;
        if (processed) processed[k] = d.processed;
        if (best_node) best_node[k] = d.best_node;
        if (z) z[k] = d.best_z;
        if (pivots) pivots[k] = d.pivots;
        if (nodes_created) nodes_created[k] = d.nrec;
    }
    return LPR_OK_OPTIMAL;
}

// optimalSolution (:1059-1066) of every IP, packed by nvars
int lpr_bb_batch_solution_read(lpr_bb_batch* b, double* x) {
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!x) {
        set_error("lpr_bb_batch_solution_read: null x");
        return LPR_BAD_ARGUMENT;
    }
    if (b->x_total == 0) return LPR_OK_OPTIMAL;
    if (!b->ran) {
        std::fill(x, x + b->x_total, 0.0);
        return LPR_OK_OPTIMAL;
    }
    LPR_HIP(hipMemcpyAsync(x, b->d.x, (size_t)b->x_total * sizeof(double), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

static int bbb_ip(lpr_bb_batch* b, const char* where, int32_t k, int64_t cap, int64_t* count) {
    if (k < 0 || k >= b->count || cap < 0 || !count) {
        set_error("%s: IP %d out of range (0..%d), cap %lld or null count", where, k,
                  b->count - 1, (long long)cap);
        return LPR_BAD_ARGUMENT;
    }
    return LPR_OK_OPTIMAL;
}

// Node records of IP k, as lpr_bb_records_read
int lpr_bb_batch_records_read(lpr_bb_batch* b, int32_t k, int32_t* parent, int32_t* kind,
                              int32_t* depth, int32_t* var, double* bound, int32_t* status,
                              double* z, int64_t cap, int64_t* count) {
    LPR_LIVE_HANDLE(b, "B&B batch");
    int rc = bbb_ip(b, "lpr_bb_batch_records_read", k, cap, count);
    if (rc != LPR_OK_OPTIMAL) return rc;
    const BBBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t n = b->ran ? std::min<int64_t>(d.nrec, cap) : 0;
    *count = n;
    if (n == 0) return LPR_OK_OPTIMAL;
    std::vector<int32_t> ri((size_t)n * kBBRecInts);
    std::vector<double> rd((size_t)n * 2);
    LPR_HIP(hipMemcpyAsync(ri.data(), b->d.rec_i + (int64_t)kBBRecInts * d.rec_off,
                           ri.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipMemcpyAsync(rd.data(), b->d.rec_d + 2 * d.rec_off, rd.size() * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    for (int64_t q = 0; q < n; ++q) {
        const int32_t* e = ri.data() + kBBRecInts * q;
        if (parent) parent[q] = e[0];
        if (kind) kind[q] = e[1];
        if (depth) depth[q] = e[2];
        if (var) var[q] = e[3];
        if (status) status[q] = e[4];
        if (bound) bound[q] = rd[(size_t)(2 * q)];
        if (z) z[q] = rd[(size_t)(2 * q + 1)];
    }
    return LPR_OK_OPTIMAL;
}

// Record ids of IP k in pop order, as lpr_bb_pop_order_read
int lpr_bb_batch_pop_order_read(lpr_bb_batch* b, int32_t k, int32_t* ids, int64_t cap,
                                int64_t* count) {
    LPR_LIVE_HANDLE(b, "B&B batch");
    int rc = bbb_ip(b, "lpr_bb_batch_pop_order_read", k, cap, count);
    if (rc != LPR_OK_OPTIMAL) return rc;
    const BBBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t n = b->ran ? std::min<int64_t>(d.processed, cap) : 0;
    *count = n;
    if (n == 0 || !ids) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(ids, b->d.pops + d.pop_off, (size_t)n * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// Pivot trace of IP k, as lpr_bb_trace_read
int lpr_bb_batch_trace_read(lpr_bb_batch* b, int32_t k, int32_t* quads, int64_t cap,
                            int64_t* count) {
    LPR_LIVE_HANDLE(b, "B&B batch");
    int rc = bbb_ip(b, "lpr_bb_batch_trace_read", k, cap, count);
    if (rc != LPR_OK_OPTIMAL) return rc;
    const BBBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t n = b->ran ? std::min<int64_t>(std::min<int64_t>(d.pivots, d.trace_cap), cap)
                             : 0;
    *count = n;
    if (n == 0 || !quads) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(quads, b->d.trace + 4 * d.trace_off, (size_t)n * 4 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// ------------------------------------------------------------------------------------------
// Narration: what ExecuteBranchAndBound writes to the console, as numbers.

static bool bbb_narrated(const char* where, const lpr_bb_batch* b) {
    if (b->narr.desc) return true;
    set_error("%s: the batch is not narrated (call lpr_bb_batch_narrate_reserve first)", where);
    return false;
}

static bool bbb_narr_ip(const char* where, const lpr_bb_batch* b, int32_t k) {
    if (k >= 0 && k < b->count) return true;
    set_error("%s: IP %d out of range (0..%d)", where, k, b->count - 1);
    return false;
}

// Makes the handle narrated: room for cap_doubles[k] doubles of child tableaux (the lists
// DoDualSimplex returns, :292 / :341 / :388) per IP, and the per-pop and incumbent buffers
int lpr_bb_batch_narrate_reserve(lpr_bb_batch* b, const int64_t* cap_doubles) {
    static const char* W = "lpr_bb_batch_narrate_reserve";
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!cap_doubles) {
        set_error("%s: null cap_doubles", W);
        return LPR_BAD_ARGUMENT;
    }
    const int32_t count = b->count;
    for (int32_t k = 0; k < count; ++k)
        if (cap_doubles[k] < 0) {
            set_error("%s: cap_doubles[%d] = %lld < 0", W, k, (long long)cap_doubles[k]);
            return LPR_BAD_ARGUMENT;
        }
    std::vector<BBNarrDesc> nd;
    try {
        nd.resize((size_t)count);
    } catch (...) {
        return bbb_oom("narration descriptors", count, sizeof(BBNarrDesc));
    }
    static const char* kSlab = "narration slab: the reserved doubles of child tableaux per IP";
    int64_t total = 0, best = 0;
    for (int32_t k = 0; k < count; ++k) {
        BBNarrDesc& c = nd[(size_t)k];
        std::memset(&c, 0, sizeof c);
        c.slab_off = total;
        c.kp.cap = cap_doubles[k];
        c.best_off = best;
        c.best_depth = -1;
        if (total > INT64_MAX / (int64_t)sizeof(double) - c.kp.cap) {
            set_error("lpr_bb_batch: cannot allocate %s (more than 2^63 bytes at IP %d of %d)",
                      kSlab, k, count);
            return LPR_OUT_OF_MEMORY;
        }
        total += c.kp.cap;
        best += b->h_desc[(size_t)k].slot_n();
    }
    hipStream_t s = b->eng->stream;
    LPR_HIP(hipStreamSynchronize(s));
    bbb_release_narr(b);  // the old slab goes first: the two need not fit side by side
    auto one = [](int64_t n) { return std::max<int64_t>(n, 1); };
    auto gb = [](int64_t n, size_t elem) {
        return [=](const char* what, int64_t) { return bbb_oom(what, n, elem); };
    };
    const int64_t pop = (int64_t)count * b->node_cap;
    const int64_t pv = (int64_t)b->node_cap * b->x_total;
    int rc = LPR_OK_OPTIMAL;
    BBNarr& D = b->narr;
    dev_alloc(&D.slab, one(total), kSlab, &rc, gb(total, sizeof(double)));
    dev_alloc(&D.best, one(best), "incumbent tableaux", &rc, gb(best, sizeof(double)));
    dev_alloc(&D.tab_off, one(b->rec_total), "child tableau offsets", &rc,
              gb(b->rec_total, sizeof(int64_t) + sizeof(int32_t)));
    dev_alloc(&D.ntab, one(b->rec_total), "child tableau offsets", &rc,
              gb(b->rec_total, sizeof(int64_t) + sizeof(int32_t)));
    dev_alloc(&D.pop_z, one(pop), "pop scores", &rc, gb(pop, sizeof(double) + sizeof(int32_t)));
    dev_alloc(&D.pop_flags, one(pop), "pop scores", &rc,
              gb(pop, sizeof(double) + sizeof(int32_t)));
    dev_alloc(&D.pop_vals, one(pv), "pop decision values", &rc, gb(pv, sizeof(double)));
    dev_alloc(&D.desc, count, "narration descriptors", &rc, gb(count, sizeof(BBNarrDesc)));
    auto fill = [&]() -> int {
        LPR_HIP(hipMemcpyAsync(D.desc, nd.data(), (size_t)count * sizeof(BBNarrDesc),
                               hipMemcpyHostToDevice, s));
        // what no record reaches reads as +0.0
        LPR_HIP(hipMemsetAsync(D.slab, 0, (size_t)one(total) * sizeof(double), s));
        LPR_HIP(hipMemsetAsync(D.pop_vals, 0, (size_t)one(pv) * sizeof(double), s));
        LPR_HIP(hipStreamSynchronize(s));
        return LPR_OK_OPTIMAL;
    };
    if (rc == LPR_OK_OPTIMAL) rc = fill();
    if (rc != LPR_OK_OPTIMAL) {
        bbb_release_narr(b);  // usable, and un-narrated
        return rc;
    }
    b->h_narr.swap(nd);
    b->narr_n = total;
    return LPR_OK_OPTIMAL;
}

// Per IP: tableaux and doubles the child LPs of the last run made (exact), doubles kept (a
// prefix of those made), and where the IP's slice starts in the slab; any may be NULL
int lpr_bb_batch_narrate_info(lpr_bb_batch* b, int64_t* tableaux, int64_t* doubles_made,
                              int64_t* doubles_kept, int64_t* offset) {
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!bbb_narrated("lpr_bb_batch_narrate_info", b)) return LPR_BAD_ARGUMENT;
    for (int32_t k = 0; k < b->count; ++k) {
        const BBNarrDesc& c = b->h_narr[(size_t)k];
        if (tableaux) tableaux[k] = c.kp.made_n;
        if (doubles_made) doubles_made[k] = c.kp.made_d;
        if (doubles_kept) doubles_kept[k] = c.kp.cur;
        if (offset) offset[k] = c.slab_off;
    }
    return LPR_OK_OPTIMAL;
}

// The pops of IP k in pop order (:1045-1076): flags (bit 0 scored, bit 1 every decision value
// integer, bit 2 became the incumbent), objVal, and nvars decision values per pop
int lpr_bb_batch_narrate_pops_read(lpr_bb_batch* b, int32_t k, int32_t* flags, double* z,
                                   double* vals, int64_t cap, int64_t* count) {
    static const char* W = "lpr_bb_batch_narrate_pops_read";
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!bbb_narrated(W, b)) return LPR_BAD_ARGUMENT;
    int rc = bbb_ip(b, W, k, cap, count);
    if (rc != LPR_OK_OPTIMAL) return rc;
    const BBBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t n = b->narr_ran ? std::min<int64_t>(d.processed, cap) : 0;
    *count = n;
    if (n == 0) return LPR_OK_OPTIMAL;
    hipStream_t s = b->eng->stream;
    if (flags)
        LPR_HIP(hipMemcpyAsync(flags, b->narr.pop_flags + d.pop_off, (size_t)n * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
    if (z)
        LPR_HIP(hipMemcpyAsync(z, b->narr.pop_z + d.pop_off, (size_t)n * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    if (vals && d.nvars > 0)
        LPR_HIP(hipMemcpyAsync(vals, b->narr.pop_vals + (int64_t)d.node_cap * d.x_off,
                               (size_t)(n * d.nvars) * sizeof(double), hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    return LPR_OK_OPTIMAL;
}

// Per record of IP k: where its child LP's tableaux start (doubles from the IP's slice start) and
// how many DoDualSimplex's list holds (:292, :341, :388, after the drop of :392-400)
int lpr_bb_batch_narrate_children_read(lpr_bb_batch* b, int32_t k, int64_t* tab_off,
                                       int32_t* ntab, int64_t cap, int64_t* count) {
    static const char* W = "lpr_bb_batch_narrate_children_read";
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!bbb_narrated(W, b)) return LPR_BAD_ARGUMENT;
    int rc = bbb_ip(b, W, k, cap, count);
    if (rc != LPR_OK_OPTIMAL) return rc;
    const BBBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t n = b->narr_ran ? std::min<int64_t>(d.nrec, cap) : 0;
    *count = n;
    if (n == 0) return LPR_OK_OPTIMAL;
    hipStream_t s = b->eng->stream;
    if (tab_off)
        LPR_HIP(hipMemcpyAsync(tab_off, b->narr.tab_off + d.rec_off, (size_t)n * sizeof(int64_t),
                               hipMemcpyDeviceToHost, s));
    if (ntab)
        LPR_HIP(hipMemcpyAsync(ntab, b->narr.ntab + d.rec_off, (size_t)n * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    return LPR_OK_OPTIMAL;
}

// Doubles [first_double, first_double + n) of IP k's slice: the tableaux DisplayTableau prints
// (:623-640), unrounded
int lpr_bb_batch_narrate_tableaux_read(lpr_bb_batch* b, int32_t k, int64_t first_double,
                                       int64_t n, double* out) {
    static const char* W = "lpr_bb_batch_narrate_tableaux_read";
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!bbb_narrated(W, b) || !bbb_narr_ip(W, b, k)) return LPR_BAD_ARGUMENT;
    const BBNarrDesc& c = b->h_narr[(size_t)k];
    const int64_t kept = b->narr_ran ? c.kp.cur : 0;
    if (first_double < 0 || n < 0 || first_double > kept || n > kept - first_double) {
        set_error("%s: doubles [%lld, %lld + %lld) of IP %d, which keeps %lld of %lld made", W,
                  (long long)first_double, (long long)first_double, (long long)n, k,
                  (long long)kept, (long long)c.kp.made_d);
        return LPR_BAD_ARGUMENT;
    }
    if (n == 0) return LPR_OK_OPTIMAL;
    if (!out) {
        set_error("%s: null output", W);
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipMemcpyAsync(out, b->narr.slab + c.slab_off + first_double,
                           (size_t)n * sizeof(double), hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// The whole slab in one copy (every IP's child tableaux); cap_doubles is what `out` holds
int lpr_bb_batch_narrate_read_all(lpr_bb_batch* b, double* out, int64_t cap_doubles) {
    static const char* W = "lpr_bb_batch_narrate_read_all";
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!bbb_narrated(W, b)) return LPR_BAD_ARGUMENT;
    if (cap_doubles < b->narr_n || (!out && b->narr_n > 0)) {
        set_error("%s: null output, or cap_doubles %lld below the slab's %lld doubles", W,
                  (long long)cap_doubles, (long long)b->narr_n);
        return LPR_BAD_ARGUMENT;
    }
    if (b->narr_n == 0) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(out, b->narr.slab, (size_t)b->narr_n * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// bestTableau of IP k (:935-983, printed at :1221): the incumbent's node as popped, rows x cols;
// out may be NULL to ask for the shape
int lpr_bb_batch_narrate_best_read(lpr_bb_batch* b, int32_t k, double* out, int32_t* rows,
                                   int32_t* cols) {
    static const char* W = "lpr_bb_batch_narrate_best_read";
    LPR_LIVE_HANDLE(b, "B&B batch");
    if (!bbb_narrated(W, b) || !bbb_narr_ip(W, b, k)) return LPR_BAD_ARGUMENT;
    const BBNarrDesc& c = b->h_narr[(size_t)k];
    const BBBatchDesc& d = b->h_desc[(size_t)k];
    if (!b->narr_ran || c.best_depth < 0) {
        set_error("%s: IP %d has no incumbent (\"No integer solution found\", :1229)", W, k);
        return LPR_BAD_ARGUMENT;
    }
    const int32_t r = d.rows + c.best_depth, cc = d.cols + c.best_depth;
    if (rows) *rows = r;
    if (cols) *cols = cc;
    if (!out) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(out, b->narr.best + c.best_off, (size_t)r * cc * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// DisplayTableau (:623-640) of every kept child tableau and of the incumbent's tableau of every
// IP, written on the device: one block per kept tableau in record-id order,
// list order within a record (bb_narr_text_layout.hpp), then the incumbent's where there is one.
// The descriptors come from three bulk reads -- the records' integers, tab_off, ntab -- and the
// host mirrors of the last run; the text owns its bytes.
int lpr_bb_batch_narrate_text(lpr_bb_batch* b, int64_t* first_block, lpr_text** out) {
    static const char* W = "lpr_bb_batch_narrate_text";
    if (!b || !b->eng) {
        set_error("%s: B&B batch handle is null or orphaned: its engine has been closed", W);
        return LPR_BAD_ARGUMENT;
    }
    if (!bbb_narrated(W, b)) return LPR_BAD_ARGUMENT;
    if (!b->narr_ran) {
        set_error("%s: the batch has not run since its last lpr_bb_batch_narrate_reserve", W);
        return LPR_BAD_ARGUMENT;
    }
    if (!out) {
        set_error("%s: null out", W);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    LPR_HIP(hipSetDevice(b->eng->device));
    hipStream_t s = b->eng->stream;
    const int64_t nrec_all = b->rec_total;
    std::vector<int32_t> ri, nt;
    std::vector<int64_t> off;
    std::vector<NarrTextRun> runs;
    std::vector<TextBlock> blk;
    try {
        ri.resize((size_t)(nrec_all * kBBRecInts));
        nt.resize((size_t)nrec_all);
        off.resize((size_t)nrec_all);
        runs.resize((size_t)(1 + 2 * b->node_cap));
    } catch (...) {
        return bbb_oom("record mirrors (host)", nrec_all, kBBRecInts * sizeof(int32_t) + 12);
    }
    if (nrec_all > 0) {
        LPR_HIP(hipMemcpyAsync(ri.data(), b->d.rec_i, ri.size() * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(off.data(), b->narr.tab_off, off.size() * sizeof(int64_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(nt.data(), b->narr.ntab, nt.size() * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipStreamSynchronize(s));
    }
    try {
        for (int32_t k = 0; k < b->count; ++k) {
            const BBBatchDesc& d = b->h_desc[(size_t)k];
            const BBNarrDesc& c = b->h_narr[(size_t)k];
            if (first_block) first_block[k] = (int64_t)blk.size();
            const int64_t nrec = std::min<int64_t>(d.nrec, (int64_t)runs.size());
            const int32_t* e = ri.data() + (int64_t)kBBRecInts * d.rec_off;
            (void)narr_text_runs(d.rows, d.cols, nrec, e + 2, e + 4, kBBRecInts,
                                 off.data() + d.rec_off, nt.data() + d.rec_off, c.kp.cur,
                                 runs.data());
            TextBlock tb{};
            tb.nvars = d.nvars;
            for (int64_t rid = 0; rid < nrec; ++rid) {
                const NarrTextRun& r = runs[(size_t)rid];
                tb.rows = r.rows;
                tb.cols = r.cols;
                tb.round4 = (int16_t)r.round4;
                for (int32_t i = 0; i < r.count; ++i) {
                    tb.src = b->narr.slab + c.slab_off + r.off + (int64_t)i * r.rows * r.cols;
                    blk.push_back(tb);
                }
            }
            if (c.best_depth >= 0) {
                tb.rows = d.rows + c.best_depth;
                tb.cols = d.cols + c.best_depth;
                tb.round4 = (int16_t)kNarrTextIncumbentRound4;
                tb.src = b->narr.best + c.best_off;
                blk.push_back(tb);
            }
        }
    } catch (...) {
        return bbb_oom("block descriptors (host)", (int64_t)blk.size(), sizeof(TextBlock));
    }
    if (first_block) first_block[b->count] = (int64_t)blk.size();
    if (blk.empty()) {
        set_error("%s: nothing to format: no IP of the batch keeps a child tableau or has an "
                  "incumbent", W);
        return LPR_BAD_ARGUMENT;
    }
    return text_format_blocks(W, b->eng, blk, out);
}

}  // extern "C"
