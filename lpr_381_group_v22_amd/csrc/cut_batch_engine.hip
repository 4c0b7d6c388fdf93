// cut_batch_engine.hip -- host side of the batched cutting plane (include/lpr_engine.h,
// lpr_cut_batch_*).  Every item runs the whole CuttingPlaneSolution
// recursion (or one DualSimplexSolver.Solve / PrimalSimplexSolver2.Solve) on the device; the host
// copies tableaux in, relaunches the bounded kernel while items are still running (BatchRunLists
// of batch_common.hpp, forms mixed per call) and copies results out.
#include "cut_batch_common.hpp"

#include <algorithm>
#include <new>

using namespace lpr;

struct lpr_cut_batch {
    lpr_engine* eng = nullptr;
    int32_t count = 0;
    std::vector<CutBatchDesc> h_desc;  // host mirror, current after create and every run
    std::vector<int32_t> last_cuts;    // cuts of the last call per item (0 before the first)
    CutBatchDesc* desc = nullptr;      // device
    double* slab = nullptr;            // every tableau at capacity: rcap x cols per item
    int32_t* logs = nullptr;           // packed by log_cap triples
    BatchRunLists run;
    // narration: set by lpr_cut_batch_narrate_reserve, before the first run
    bool ran = false;                 // lpr_cut_batch_run has been called
    bool narrated = false;
    CutNarr narr;                     // device
    std::vector<CutNarrDesc> h_narr;  // host mirror, current after reserve and every run
    int64_t narr_doubles = 0;         // the data slab: the sum of the caps
    int64_t narr_events = 0;          // the event buffer: count * ev_cap quads
};

namespace {

int cb_oom(const char* what, int64_t n) {
    set_error("lpr_cut_batch: cannot allocate %s (%lld elements)", what, (long long)n);
    return LPR_OUT_OF_MEMORY;
}

void cb_release_narr(lpr_cut_batch* b) {
    hipFree(b->narr.desc);
    hipFree(b->narr.ev);
    hipFree(b->narr.data);
    b->narr = CutNarr();
    b->narrated = false;
}

void cb_release_device(lpr_cut_batch* b) {
    cb_release_narr(b);
    hipFree(b->desc);
    hipFree(b->slab);
    hipFree(b->logs);
    b->run.release();
    b->desc = nullptr;
    b->slab = nullptr;
    b->logs = nullptr;
}

int cb_fail(lpr_cut_batch* b, int rc) {
    cb_release_device(b);
    delete b;
    return rc;
}

// rows >= 2 (ArgumentException :68), cols >= 2, and the tableau at full row capacity within
// form H.
bool cb_shape_ok(const char* where, int32_t k, int64_t rows, int64_t cols, int max_cuts) {
    if (rows < 2 || cols < 2) {
        set_error("%s: item %d has a %lld x %lld tableau; it needs an objective row and at least "
                  "one constraint row (rows >= 2) and cols >= 2", where, k, (long long)rows,
                  (long long)cols);
        return false;
    }
    if (rows + max_cuts > kBatchMaxRowsH || cols > kBatchMaxColsH) {
        set_error("%s: item %d has a %lld x %lld tableau, %lld x %lld with max_cuts %d: beyond "
                  "the batch limit of %d x %d (form H); run it alone with lpr_cutting_plane",
                  where, k, (long long)rows, (long long)cols, (long long)(rows + max_cuts),
                  (long long)cols, max_cuts, kBatchMaxRowsH, kBatchMaxColsH);
        return false;
    }
    return true;
}

// Offsets and device memory for `count` items of the given shapes.  On failure nothing is left.
int cb_alloc(lpr_engine* e, int32_t count, const std::vector<int32_t>& R,
             const std::vector<int32_t>& Cc, int max_cuts, int32_t log_cap, lpr_cut_batch** out) {
    lpr_cut_batch* b = new (std::nothrow) lpr_cut_batch();
    if (!b) return cb_oom("handle", 1);
    b->eng = e;
    b->count = count;
    try {
        b->h_desc.resize((size_t)count);
        b->last_cuts.assign((size_t)count, 0);
    } catch (...) {
        delete b;
        return cb_oom("descriptors", count);
    }
    int64_t t = 0, lg = 0;
    for (int32_t k = 0; k < count; ++k) {
        CutBatchDesc& d = b->h_desc[(size_t)k];
        std::memset(&d, 0, sizeof d);
        d.rows = R[(size_t)k];
        d.cols = Cc[(size_t)k];
        d.rcap = d.rows + max_cuts;
        d.log_cap = log_cap > 0 ? log_cap
                                : std::min<int32_t>(kBatchLogDefaultMax, 4 * (d.rcap + d.cols));
        d.t_off = t;
        d.log_off = lg;
        d.phase = kCutPhaseAdd;
        d.code = LPR_OK_OPTIMAL;  // not run yet
        t += (int64_t)d.rcap * d.cols;  // below 2^21 each, count below 2^31: no overflow
        lg += d.log_cap;
    }
    int rc = LPR_OK_OPTIMAL;
    dev_alloc(&b->desc, count, "descriptors", &rc, cb_oom);
    dev_alloc(&b->slab, t, "tableau slab: (rows + max_cuts) x cols doubles per item", &rc, cb_oom);
    dev_alloc(&b->logs, lg * 3, "logs", &rc, cb_oom);
    b->run.alloc(count, &rc, cb_oom);
    if (rc == LPR_OK_OPTIMAL &&
        hipMemcpy(b->desc, b->h_desc.data(), (size_t)count * sizeof(CutBatchDesc),
                  hipMemcpyHostToDevice) != hipSuccess) {
        set_error("lpr_cut_batch: descriptor upload failed");
        rc = LPR_DEVICE_ERROR;
    }
    if (rc != LPR_OK_OPTIMAL) return cb_fail(b, rc);
    *out = b;
    return LPR_OK_OPTIMAL;
}

// The tableaux into their slices: src on the device, src_off[k] the start of item k there.
// Synchronous; the descriptors come back with z set.
int cb_load(lpr_cut_batch* b, const double* d_src, const std::vector<int64_t>& src_off) {
    hipStream_t s = b->eng->stream;
    int64_t* d_off = nullptr;
    if (hipMalloc(&d_off, (size_t)b->count * sizeof(int64_t)) != hipSuccess)
        return cb_oom("tableau offsets", b->count);
    hipError_t err = hipMemcpyAsync(d_off, src_off.data(), (size_t)b->count * sizeof(int64_t),
                                    hipMemcpyHostToDevice, s);
    int rc = LPR_OK_OPTIMAL;
    if (err == hipSuccess) rc = cut_batch_launch_load(s, b->desc, b->count, d_src, d_off, b->slab);
    if (err == hipSuccess && rc == LPR_OK_OPTIMAL)
        err = hipMemcpyAsync(b->h_desc.data(), b->desc, (size_t)b->count * sizeof(CutBatchDesc),
                             hipMemcpyDeviceToHost, s);
    if (err == hipSuccess && rc == LPR_OK_OPTIMAL) err = hipStreamSynchronize(s);
    hipFree(d_off);
    if (err != hipSuccess) {
        set_error("lpr_cut_batch: loading the tableaux failed: %s", hipGetErrorString(err));
        return LPR_DEVICE_ERROR;
    }
    return rc;
}

bool cb_item_ok(const char* where, const lpr_cut_batch* b, int32_t k) {
    if (k >= 0 && k < b->count) return true;
    set_error("%s: item %d out of range (0..%d)", where, k, b->count - 1);
    return false;
}

}  // namespace

namespace lpr {
void cut_batch_orphan(lpr_cut_batch* b) {  // lpr_engine_close
    cb_release_device(b);
    b->eng = nullptr;
}
}  // namespace lpr

extern "C" {

// objectiveRow + constraintRows per item (CuttingPlaneSolver.cs:64-70), from host tableaux
int lpr_cut_batch_create(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                         const double* tableaux, int32_t max_cuts, int32_t log_cap,
                         lpr_cut_batch** out) {
    static const char* W = "lpr_cut_batch_create";
    if (!e || !out || count < 1 || !rows || !cols || !tableaux || log_cap < 0) {
        set_error("%s: bad arguments (count=%d, log_cap=%d, or a null engine / handle / rows / "
                  "cols / tableaux)", W, count, log_cap);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    if (max_cuts <= 0) max_cuts = kCutBatchDefaultMaxCuts;
    std::vector<int32_t> R((size_t)count), Cc((size_t)count);
    std::vector<int64_t> off((size_t)count);
    int64_t total = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (!cb_shape_ok(W, k, rows[k], cols[k], max_cuts)) return LPR_BAD_ARGUMENT;
        R[(size_t)k] = rows[k];
        Cc[(size_t)k] = cols[k];
        off[(size_t)k] = total;
        total += (int64_t)rows[k] * cols[k];
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_cut_batch* b = nullptr;
    int rc = cb_alloc(e, count, R, Cc, max_cuts, log_cap, &b);
    if (rc != LPR_OK_OPTIMAL) return rc;
    double* d_src = nullptr;
    if (hipMalloc(&d_src, (size_t)total * sizeof(double)) != hipSuccess) {
        rc = cb_oom("tableau upload", total);
    } else if (hipMemcpy(d_src, tableaux, (size_t)total * sizeof(double),
                         hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: tableau upload failed", W);
        rc = LPR_DEVICE_ERROR;
    } else {
        rc = cb_load(b, d_src, off);
    }
    hipFree(d_src);
    if (rc != LPR_OK_OPTIMAL) return cb_fail(b, rc);
    e->live_cut_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

// ... from the FinalTableau of every LP of a solved lpr_batch, device to device
int lpr_cut_batch_from_batch(lpr_batch* lps, int32_t max_cuts, int32_t log_cap,
                             lpr_cut_batch** out) {
    static const char* W = "lpr_cut_batch_from_batch";
    const std::vector<BatchDesc>* bd = nullptr;
    const double* slab = nullptr;
    lpr_engine* e = batch_view(lps, &bd, &slab);
    if (!e || !out || log_cap < 0) {
        set_error("%s: the LP batch is null or orphaned (its engine has been closed), a null "
                  "handle, or log_cap=%d", W, log_cap);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    if (max_cuts <= 0) max_cuts = kCutBatchDefaultMaxCuts;
    const int32_t count = (int32_t)bd->size();
    std::vector<int32_t> R((size_t)count), Cc((size_t)count);
    std::vector<int64_t> off((size_t)count);
    for (int32_t k = 0; k < count; ++k) {
        const BatchDesc& d = (*bd)[(size_t)k];
        if (d.status == kRunning || d.status == LPR_PIVOT_LIMIT) {
            set_error("%s: LP %d has no FinalTableau (status %d: %s)", W, k, d.status,
                      d.status == LPR_PIVOT_LIMIT ? "stopped at its pivot limit" : "not solved");
            return LPR_BAD_ARGUMENT;
        }
        if (!cb_shape_ok(W, k, d.rows, d.cols, max_cuts)) return LPR_BAD_ARGUMENT;
        R[(size_t)k] = d.rows;
        Cc[(size_t)k] = d.cols;
        off[(size_t)k] = d.t_off;
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_cut_batch* b = nullptr;
    int rc = cb_alloc(e, count, R, Cc, max_cuts, log_cap, &b);
    if (rc != LPR_OK_OPTIMAL) return rc;
    rc = cb_load(b, slab, off);  // synchronous: the LP batch may go right after
    if (rc != LPR_OK_OPTIMAL) return cb_fail(b, rc);
    e->live_cut_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_destroy(lpr_cut_batch* b) {
    if (!b) return LPR_BAD_ARGUMENT;
    if (b->eng) {
        hipSetDevice(b->eng->device);
        hipStreamSynchronize(b->eng->stream);
        cb_release_device(b);
        unlist(b->eng->live_cut_batch, b);
    }
    delete b;
    return LPR_OK_OPTIMAL;
}

// CuttingPlaneSolution (:64-229), DualSimplexSolver.Solve (DualSimplex.cs:14-114) or
// PrimalSimplexSolver2.Solve (PrimalSimplexSolver2.cs:46-97) for every item, from the tableau the
// last call left
int lpr_cut_batch_run(lpr_cut_batch* b, const lpr_cut_batch_opts* opts, lpr_cut_batch_result* res) {
    static const char* W = "lpr_cut_batch_run";
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!res) {
        set_error("%s: null result", W);
        return LPR_BAD_ARGUMENT;
    }
    lpr_cut_batch_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (o.mode < kCutModeCuttingPlane || o.mode > kCutModePrimal2) {
        set_error("%s: unknown mode %d (0 cutting plane, 1 dual solve, 2 primal2 solve)", W,
                  o.mode);
        return LPR_BAD_ARGUMENT;
    }
    if ((o.variant != 0 && o.variant != 2 && o.variant != 3) || o.chunk < 0) {
        set_error("%s: variant %d (0 auto, 2 G, 3 H) / chunk %d (>= 0)", W, o.variant, o.chunk);
        return LPR_BAD_ARGUMENT;
    }
    std::memset(res, 0, sizeof *res);
    b->ran = true;
    hipStream_t s = b->eng->stream;
    const int32_t count = b->count;
    CutBatchCall call;
    std::memset(&call, 0, sizeof call);
    call.mode = o.mode;
    call.hard_cap = o.hard_cap;
    if (o.mode == kCutModeCuttingPlane) {
        call.max_iters = kCutBatchInnerIters;  // :190 / :200
        call.print_steps = 1;                  // printSteps: true
    } else {
        call.max_iters = o.max_iters;
        call.print_steps = o.print_steps ? 1 : 0;
    }
    std::vector<int32_t> lists[kNumForms];
    size_t lds[kNumForms] = {0, 0, 0};
    for (int32_t k = 0; k < count; ++k) {
        CutBatchDesc& d = b->h_desc[(size_t)k];
        const int left = d.rcap - d.rows;
        d.code = kRunning;
        d.cuts = 0;
        d.pivots = 0;
        d.iter = 0;
        d.done = 0;
        d.cut_limit = o.mode == kCutModeCuttingPlane
                          ? (o.max_cuts > 0 ? std::min<int32_t>(o.max_cuts, left) : left)
                          : 0;
        d.phase = o.mode == kCutModeCuttingPlane
                      ? kCutPhaseAdd
                      : (o.mode == kCutModeDual ? kCutPhaseDual : kCutPhasePrimal2);
        const size_t fp = cut_batch_footprint_g(d.rcap, d.cols);
        const int form = batch_pick_form(fp, o.variant, false);
        lds[form] = std::max(lds[form], form == kFormG ? fp : cut_batch_aux_bytes(d.rcap, d.cols));
        lists[form].push_back(k);
    }
    const size_t n_form[kNumForms] = {lists[0].size(), lists[1].size(), lists[2].size()};
    int rc = b->run.upload(s, lists);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->desc, b->h_desc.data(), (size_t)count * sizeof(CutBatchDesc),
                           hipMemcpyHostToDevice, s));
    if (b->narrated) {
        rc = cut_batch_narr_launch_call(s, b->desc, b->narr, count, call.mode, call.print_steps);
        if (rc != LPR_OK_OPTIMAL) return rc;
    }
    int launches = 0;
    rc = b->run.rounds(s, [&](int f, const int32_t* in, int n_in, int32_t* out, int32_t* n_out) {
        CutBatchCall c = call;
        c.chunk = o.chunk > 0 ? o.chunk : kCutBatchChunk[f];
        if (b->narrated)
            return cut_batch_narr_launch(f, s, b->desc, b->slab, b->logs, c, b->narr, lds[f], in,
                                         n_in, out, n_out);
        return cut_batch_launch(f, s, b->desc, b->slab, b->logs, c, lds[f], in, n_in, out, n_out);
    }, &launches);
    if (rc != LPR_OK_OPTIMAL) return rc;
    if (b->narrated)
        LPR_HIP(hipMemcpyAsync(b->h_narr.data(), b->narr.desc,
                               (size_t)count * sizeof(CutNarrDesc), hipMemcpyDeviceToHost, s));
    LPR_HIP(hipMemcpyAsync(b->h_desc.data(), b->desc, (size_t)count * sizeof(CutBatchDesc),
                           hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    for (int32_t k = 0; k < count; ++k) {
        const CutBatchDesc& d = b->h_desc[(size_t)k];
        b->last_cuts[(size_t)k] = d.cuts;
        if (d.code >= 0 && d.code < kNumCutExits) res->by_code[d.code] += 1;
        res->cuts += d.cuts;
        res->pivots += d.pivots;
    }
    res->launches = launches;
    res->items_g = (int32_t)n_form[kFormG];
    res->items_h = (int32_t)n_form[kFormH];
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_result_read(lpr_cut_batch* b, int32_t* code, int32_t* cuts, int32_t* rows,
                              int64_t* log_count) {
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    for (int32_t k = 0; k < b->count; ++k) {
        const CutBatchDesc& d = b->h_desc[(size_t)k];
        if (code) code[k] = d.code;
        if (cuts) cuts[k] = b->last_cuts[(size_t)k];
        if (rows) rows[k] = d.rows;
        if (log_count) log_count[k] = d.log_n;
    }
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_shape(lpr_cut_batch* b, int32_t k, int32_t* rows, int32_t* cols,
                        int32_t* row_cap, int32_t* log_cap) {
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!cb_item_ok("lpr_cut_batch_shape", b, k)) return LPR_BAD_ARGUMENT;
    const CutBatchDesc& d = b->h_desc[(size_t)k];
    if (rows) *rows = d.rows;
    if (cols) *cols = d.cols;
    if (row_cap) *row_cap = d.rcap;
    if (log_cap) *log_cap = d.log_cap;
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_tableau_read(lpr_cut_batch* b, int32_t k, double* rowmajor) {
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!cb_item_ok("lpr_cut_batch_tableau_read", b, k)) return LPR_BAD_ARGUMENT;
    if (!rowmajor) {
        set_error("lpr_cut_batch_tableau_read: null output");
        return LPR_BAD_ARGUMENT;
    }
    const CutBatchDesc& d = b->h_desc[(size_t)k];
    LPR_HIP(hipMemcpyAsync(rowmajor, b->slab + d.t_off, (size_t)d.rows * d.cols * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_log_read(lpr_cut_batch* b, int32_t k, int32_t* triples, int64_t cap,
                           int64_t* count) {
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!cb_item_ok("lpr_cut_batch_log_read", b, k)) return LPR_BAD_ARGUMENT;
    if (cap < 0 || !count) {
        set_error("lpr_cut_batch_log_read: cap %lld or null count", (long long)cap);
        return LPR_BAD_ARGUMENT;
    }
    const CutBatchDesc& d = b->h_desc[(size_t)k];
    *count = d.log_n;
    const int64_t n = std::min(std::min<int64_t>(d.log_n, d.log_cap), cap);
    if (n == 0 || !triples) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(triples, b->logs + 3 * d.log_off, (size_t)n * 3 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_z_read(lpr_cut_batch* b, double* z) {
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!z) {
        set_error("lpr_cut_batch_z_read: null output");
        return LPR_BAD_ARGUMENT;
    }
    for (int32_t k = 0; k < b->count; ++k) z[k] = b->h_desc[(size_t)k].z;
    return LPR_OK_OPTIMAL;
}

// ---- narration ---------------------------------------------------------

// What the console text of CuttingPlaneSolution (CuttingPlaneSolver.cs:47-54, 64-229) and of the
// two clean-up solvers under printSteps (DualSimplex.cs:14-114, 193-207; PrimalSimplexSolver2.cs:
// 46-97, 184-189) needs: from now on the handle launches the narrated kernels.
int lpr_cut_batch_narrate_reserve(lpr_cut_batch* b, const int64_t* cap_doubles, int32_t ev_cap) {
    static const char* W = "lpr_cut_batch_narrate_reserve";
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (b->narrated || b->ran || !cap_doubles || ev_cap < 1) {
        set_error("%s: %s", W,
                  b->narrated ? "the handle is narrated already"
                  : b->ran    ? "the handle has run; reserve before the first lpr_cut_batch_run"
                  : !cap_doubles ? "null cap_doubles" : "ev_cap < 1");
        return LPR_BAD_ARGUMENT;
    }
    const int32_t count = b->count;
    int64_t total = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (cap_doubles[k] < 0 || cap_doubles[k] > (INT64_MAX >> 4) - total) {
            set_error("%s: cap_doubles[%d] = %lld", W, k, (long long)cap_doubles[k]);
            return LPR_BAD_ARGUMENT;
        }
        total += cap_doubles[k];
    }
    try {
        b->h_narr.assign((size_t)count, CutNarrDesc());
    } catch (...) {
        return cb_oom("narration cursors", count);
    }
    int64_t off = 0;
    for (int32_t k = 0; k < count; ++k) {
        CutNarrDesc& c = b->h_narr[(size_t)k];
        std::memset(&c, 0, sizeof c);
        c.ev_off = (int64_t)k * ev_cap;
        c.ev_cap = ev_cap;
        c.data_off = off;
        c.kp.cap = cap_doubles[k];
        off += c.kp.cap;
    }
    b->narr_doubles = total;
    b->narr_events = (int64_t)count * ev_cap;
    hipStream_t s = b->eng->stream;
    int rc = LPR_OK_OPTIMAL;
    dev_alloc(&b->narr.desc, count, "narration cursors", &rc, cb_oom);
    dev_alloc(&b->narr.ev, 4 * b->narr_events, "narration events: 4 x ev_cap int32 per item", &rc,
              cb_oom);
    dev_alloc(&b->narr.data, std::max<int64_t>(total, 1),
              "narration data slab: the sum of cap_doubles", &rc, cb_oom);
    if (rc == LPR_OK_OPTIMAL) {
        // The data slab starts as 0xFF bytes (a quiet NaN in every double): what no kept block
        // covers stays that, so a read of it cannot be mistaken for a stored value.
        hipError_t err = hipMemsetAsync(b->narr.data, 0xFF,
                                        (size_t)std::max<int64_t>(total, 1) * sizeof(double), s);
        if (err == hipSuccess)
            err = hipMemcpyAsync(b->narr.desc, b->h_narr.data(),
                                 (size_t)count * sizeof(CutNarrDesc), hipMemcpyHostToDevice, s);
        if (err == hipSuccess)
            rc = cut_batch_narr_launch_first(s, b->desc, b->slab, b->narr, count);
        if (err == hipSuccess && rc == LPR_OK_OPTIMAL)
            err = hipMemcpyAsync(b->h_narr.data(), b->narr.desc,
                                 (size_t)count * sizeof(CutNarrDesc), hipMemcpyDeviceToHost, s);
        if (err == hipSuccess && rc == LPR_OK_OPTIMAL) err = hipStreamSynchronize(s);
        if (err != hipSuccess) {
            set_error("%s: writing block 0 failed: %s", W, hipGetErrorString(err));
            rc = LPR_DEVICE_ERROR;
        }
    }
    if (rc != LPR_OK_OPTIMAL) {  // the handle stays usable and un-narrated
        cb_release_narr(b);
        b->h_narr.clear();
        return rc;
    }
    b->narrated = true;
    return LPR_OK_OPTIMAL;
}

}  // extern "C"

namespace {
bool cb_narrated(const char* where, const lpr_cut_batch* b) {
    if (b->narrated) return true;
    set_error("%s: the handle is not narrated (lpr_cut_batch_narrate_reserve)", where);
    return false;
}
}  // namespace

extern "C" {

// Per item: events made, doubles made, doubles kept, and where its slice starts in what
// lpr_cut_batch_narrate_read_all copies.  Events kept = min(made, ev_cap), at quad k * ev_cap.
int lpr_cut_batch_narrate_info(lpr_cut_batch* b, int64_t* events_made, int64_t* doubles_made,
                               int64_t* doubles_kept, int64_t* data_off) {
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!cb_narrated("lpr_cut_batch_narrate_info", b)) return LPR_BAD_ARGUMENT;
    for (int32_t k = 0; k < b->count; ++k) {
        const CutNarrDesc& c = b->h_narr[(size_t)k];
        if (events_made) events_made[k] = c.ev_n;
        if (doubles_made) doubles_made[k] = c.kp.made_d;
        if (doubles_kept) doubles_kept[k] = c.kp.cur;
        if (data_off) data_off[k] = c.data_off;
    }
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_narrate_events_read(lpr_cut_batch* b, int32_t k, int32_t* quads, int64_t cap,
                                      int64_t* count) {
    static const char* W = "lpr_cut_batch_narrate_events_read";
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!cb_narrated(W, b) || !cb_item_ok(W, b, k)) return LPR_BAD_ARGUMENT;
    if (cap < 0 || !count) {
        set_error("%s: cap %lld or null count", W, (long long)cap);
        return LPR_BAD_ARGUMENT;
    }
    const CutNarrDesc& c = b->h_narr[(size_t)k];
    *count = c.ev_n;
    const int64_t n = std::min(std::min<int64_t>(c.ev_n, c.ev_cap), cap);
    if (n == 0 || !quads) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(quads, b->narr.ev + 4 * c.ev_off, (size_t)n * 4 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

int lpr_cut_batch_narrate_data_read(lpr_cut_batch* b, int32_t k, int64_t first_double, int64_t n,
                                    double* out) {
    static const char* W = "lpr_cut_batch_narrate_data_read";
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!cb_narrated(W, b) || !cb_item_ok(W, b, k)) return LPR_BAD_ARGUMENT;
    const CutNarrDesc& c = b->h_narr[(size_t)k];
    if (first_double < 0 || n < 0 || first_double > c.kp.cur || n > c.kp.cur - first_double ||
        (n > 0 && !out)) {
        set_error("%s: item %d keeps %lld doubles; [%lld, %lld + %lld) is beyond them (or a null "
                  "output)", W, k, (long long)c.kp.cur, (long long)first_double,
                  (long long)first_double, (long long)n);
        return LPR_BAD_ARGUMENT;
    }
    if (n == 0) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(out, b->narr.data + c.data_off + first_double,
                           (size_t)n * sizeof(double), hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// The whole event buffer (count x ev_cap quads) and the whole data slab (the sum of the caps) in
// two copies; either may be NULL.
int lpr_cut_batch_narrate_read_all(lpr_cut_batch* b, int32_t* quads, int64_t cap_quads,
                                   double* data, int64_t cap_doubles) {
    static const char* W = "lpr_cut_batch_narrate_read_all";
    LPR_LIVE_HANDLE(b, "cutting-plane batch");
    if (!cb_narrated(W, b)) return LPR_BAD_ARGUMENT;
    if ((quads && cap_quads < b->narr_events) || (data && cap_doubles < b->narr_doubles)) {
        set_error("%s: the events take %lld quads and the data %lld doubles; %lld / %lld given",
                  W, (long long)b->narr_events, (long long)b->narr_doubles, (long long)cap_quads,
                  (long long)cap_doubles);
        return LPR_BAD_ARGUMENT;
    }
    hipStream_t s = b->eng->stream;
    if (quads)
        LPR_HIP(hipMemcpyAsync(quads, b->narr.ev, (size_t)b->narr_events * 4 * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
    if (data && b->narr_doubles > 0)
        LPR_HIP(hipMemcpyAsync(data, b->narr.data, (size_t)b->narr_doubles * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    return LPR_OK_OPTIMAL;
}

}  // extern "C"
