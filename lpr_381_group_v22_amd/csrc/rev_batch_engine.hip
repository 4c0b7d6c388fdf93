// rev_batch_engine.hip -- host side of the batched revised simplex (include/lpr_engine.h,
// lpr_rev_batch_*).  Every LP of a batch is solved on the device with the
// rules of RevisedPrimalSimplexSolver; the host only picks each LP's form, relaunches the bounded
// solve kernels while LPs are still running (BatchRunLists: one small counter read per launch
// round) and copies results out.  A handle made traced (lpr_rev_batch_trace_*, section 21) launches
// the traced kernels, which also write every CaptureSnapshot of every LP as numbers.
#include "rev_batch_common.hpp"

#include <algorithm>
#include <new>

using namespace lpr;

struct lpr_rev_batch {
    lpr_engine* eng = nullptr;
    int32_t count = 0;
    std::vector<RevBatchDesc> h_desc;  // host mirror, current after create and every solve
    RevBatchDesc* desc = nullptr;      // device
    double* slab = nullptr;            // every LP's slice (RevBatchDesc)
    int32_t* basis = nullptr;          // packed by m
    int32_t* logs = nullptr;           // packed by log_cap triples
    double* xs = nullptr;              // packed by n
    BatchRunLists run;                 // the running lists and their counters
    int64_t slab_n = 0, basis_n = 0, log_n = 0, x_total = 0;
    bool solved = false;               // lpr_rev_batch_solve has run: too late to reserve a trace
    // traced (lpr_rev_batch_trace_reserve): trace_cap records per LP, section 21
    int32_t trace_cap = 0;             // 0: untraced
    double* trace = nullptr;           // device, trace_n doubles
    int64_t* trace_off = nullptr;      // device, per LP
    std::vector<int64_t> h_trace_off;  // LP k's records start at trace + h_trace_off[k]
    int64_t trace_n = 0;
};

namespace {

int rb_oom(const char* what, int64_t n) {
    set_error("lpr_rev_batch: cannot allocate %s (%lld elements)", what, (long long)n);
    return LPR_OUT_OF_MEMORY;
}

void rb_release_device(lpr_rev_batch* b) {
    hipFree(b->desc);
    hipFree(b->slab);
    hipFree(b->basis);
    hipFree(b->logs);
    hipFree(b->xs);
    hipFree(b->trace);
    hipFree(b->trace_off);
    b->trace = nullptr;
    b->trace_off = nullptr;
    b->run.release();
    b->desc = nullptr;
    b->slab = nullptr;
    b->basis = nullptr;
    b->logs = nullptr;
    b->xs = nullptr;
}

int rb_fail(lpr_rev_batch* b, int rc) {
    rb_release_device(b);
    delete b;
    return rc;
}

bool rb_item_ok(const char* where, const lpr_rev_batch* b, int32_t k) {
    if (k >= 0 && k < b->count) return true;
    set_error("%s: LP %d out of range (0..%d)", where, k, b->count - 1);
    return false;
}

}  // namespace

namespace lpr {
void rev_batch_orphan(lpr_rev_batch* b) {  // lpr_engine_close
    rb_release_device(b);
    b->eng = nullptr;
}
}  // namespace lpr

extern "C" {

// new RevisedPrimalSimplexSolver(objective, constraints, isMin) per LP (:41-80), built on the
// device
int lpr_rev_batch_create(lpr_engine* e, int32_t count, const int32_t* n, const int32_t* m,
                         const double* objective, const double* A, const double* b,
                         const int8_t* is_min, int32_t log_cap, lpr_rev_batch** out) {
    static const char* W = "lpr_rev_batch_create";
    if (!e || !out || count < 1 || !n || !m || !objective || !A || !b || !is_min || log_cap < 0) {
        set_error("%s: bad arguments (count=%d, log_cap=%d, or a null engine / handle / n / m / "
                  "objective / A / b / is_min)", W, count, log_cap);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    for (int32_t k = 0; k < count; ++k) {
        if (n[k] < 1 || m[k] < 1) {  // the two ArgumentExceptions of :43-44
            set_error("%s: LP %d has n=%d m=%d; it needs at least one objective coefficient and "
                      "one constraint", W, k, n[k], m[k]);
            return LPR_BAD_ARGUMENT;
        }
        if (m[k] > kRevBatchMaxM || (int64_t)n[k] + m[k] > kRevBatchMaxNM) {
            set_error("%s: LP %d has m=%d n=%d, beyond the batch limit of m <= %d and n + m <= %d "
                      "(form H); solve it alone with lpr_revised_solve", W, k, m[k], n[k],
                      kRevBatchMaxM, kRevBatchMaxNM);
            return LPR_BAD_ARGUMENT;
        }
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_rev_batch* h = new (std::nothrow) lpr_rev_batch();
    if (!h) return rb_oom("handle", 1);
    h->eng = e;
    h->count = count;
    std::vector<RevBatchBuild> bd;
    try {
        h->h_desc.resize((size_t)count);
        bd.resize((size_t)count);
    } catch (...) {
        delete h;
        return rb_oom("descriptors", count);
    }
    int64_t sl = 0, bs = 0, lg = 0, x = 0, sa = 0;
    for (int32_t k = 0; k < count; ++k) {
        RevBatchDesc& d = h->h_desc[(size_t)k];
        std::memset(&d, 0, sizeof d);
        d.n = n[k];
        d.m = m[k];
        d.is_min = is_min[k] != 0;
        d.log_cap = log_cap > 0 ? log_cap
                                : std::min<int32_t>(kBatchLogDefaultMax, 4 * (d.n + 2 * d.m));
        d.s_off = sl;
        d.b_off = bs;
        d.log_off = lg;
        d.x_off = x;
        d.status = kRunning;
        bd[(size_t)k] = RevBatchBuild{x, sa, bs};
        // 64-bit: a slice is below 2^22 doubles and count below 2^31
        sl += rev_batch_slice(d.m, d.n);
        bs += d.m;
        lg += d.log_cap;
        x += d.n;
        sa += (int64_t)d.m * d.n;
    }
    h->slab_n = sl;
    h->basis_n = bs;
    h->log_n = lg;
    h->x_total = x;
    int rc = LPR_OK_OPTIMAL;
    double *d_obj = nullptr, *d_A = nullptr, *d_b = nullptr;
    RevBatchBuild* d_bd = nullptr;
    dev_alloc(&h->desc, count, "descriptors", &rc, rb_oom);
    dev_alloc(&h->slab, sl, "slab: m x m + m x n + 3 m + n doubles per LP", &rc, rb_oom);
    dev_alloc(&h->basis, bs, "bases", &rc, rb_oom);
    dev_alloc(&h->logs, 3 * lg, "pivot logs", &rc, rb_oom);
    dev_alloc(&h->xs, x, "solutions", &rc, rb_oom);
    h->run.alloc(count, &rc, rb_oom);
    dev_alloc(&d_obj, x, "build inputs", &rc, rb_oom);
    dev_alloc(&d_A, sa, "build inputs", &rc, rb_oom);
    dev_alloc(&d_b, bs, "build inputs", &rc, rb_oom);
    dev_alloc(&d_bd, count, "build inputs", &rc, rb_oom);
    hipStream_t s = e->stream;
    auto build = [&]() -> int {
        LPR_HIP(hipMemcpyAsync(h->desc, h->h_desc.data(), (size_t)count * sizeof(RevBatchDesc),
                               hipMemcpyHostToDevice, s));
        LPR_HIP(hipMemcpyAsync(d_bd, bd.data(), (size_t)count * sizeof(RevBatchBuild),
                               hipMemcpyHostToDevice, s));
        LPR_HIP(hipMemcpyAsync(d_obj, objective, (size_t)x * sizeof(double),
                               hipMemcpyHostToDevice, s));
        LPR_HIP(hipMemcpyAsync(d_A, A, (size_t)sa * sizeof(double), hipMemcpyHostToDevice, s));
        LPR_HIP(hipMemcpyAsync(d_b, b, (size_t)bs * sizeof(double), hipMemcpyHostToDevice, s));
        rev_batch_launch_build(s, h->desc, d_bd, count, h->slab, h->basis, h->xs, d_obj, d_A,
                               d_b);
        LPR_HIP(hipGetLastError());
        LPR_HIP(hipStreamSynchronize(s));  // inputs are borrowed
        return LPR_OK_OPTIMAL;
    };
    if (rc == LPR_OK_OPTIMAL) rc = build();
    hipFree(d_obj);
    hipFree(d_A);
    hipFree(d_b);
    hipFree(d_bd);
    if (rc != LPR_OK_OPTIMAL) return rb_fail(h, rc);
    e->live_rev_batch.push_back(h);
    *out = h;
    return LPR_OK_OPTIMAL;
}

int lpr_rev_batch_destroy(lpr_rev_batch* b) {
    if (!b) return LPR_BAD_ARGUMENT;
    if (b->eng) {
        hipSetDevice(b->eng->device);
        hipStreamSynchronize(b->eng->stream);
        rb_release_device(b);
        unlist(b->eng->live_rev_batch, b);
    }
    delete b;
    return LPR_OK_OPTIMAL;
}

// RevisedPrimalSimplexSolver.Solve() (:82-251) and ExtractSolution (:277-287) for every LP that
// is not finished
int lpr_rev_batch_solve(lpr_rev_batch* b, const lpr_rev_batch_opts* opts,
                        lpr_rev_batch_result* res) {
    static const char* W = "lpr_rev_batch_solve";
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!res) {
        set_error("%s: null result", W);
        return LPR_BAD_ARGUMENT;
    }
    lpr_rev_batch_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (o.variant < 0 || o.variant > 3 || o.chunk < 0) {
        set_error("%s: variant %d (0 auto, 1 W, 2 G, 3 H) / chunk %d (>= 0)", W, o.variant,
                  o.chunk);
        return LPR_BAD_ARGUMENT;
    }
    std::memset(res, 0, sizeof *res);
    hipStream_t s = b->eng->stream;
    const int32_t count = b->count;
    std::vector<int32_t> lists[kNumForms];
    size_t slot[kNumForms] = {0, 0, 0};
    int64_t before = 0;
    for (int32_t k = 0; k < count; ++k) {
        RevBatchDesc& d = b->h_desc[(size_t)k];
        before += d.iter;
        if (d.status != kRunning && d.status != LPR_PIVOT_LIMIT) continue;  // finished stays so
        d.status = kRunning;
        d.max_iter = o.max_pivots > 0 ? d.iter + o.max_pivots : 0;
        const size_t fp = rev_batch_footprint(d.m, d.n);
        const int f = batch_pick_form(fp * sizeof(double), o.variant);
        lists[f].push_back(k);
        const size_t need = f == kFormH ? rev_batch_vectors(d.m, d.n) : fp;
        slot[f] = std::max(slot[f], (need + 1) & ~(size_t)1);
    }
    int rc = b->run.upload(s, lists);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->desc, b->h_desc.data(), (size_t)count * sizeof(RevBatchDesc),
                           hipMemcpyHostToDevice, s));
    int launches = 0;
    b->solved = true;
    const RevBatchTrace tr{b->trace, b->trace_off, b->trace_cap};
    rc = b->run.rounds(s, [&](int f, const int32_t* in, int n_in, int32_t* out, int32_t* n_out) {
        const int chunk = o.chunk > 0 ? o.chunk : kRevBatchChunk[f];
        if (b->trace_cap > 0)
            return rev_batch_trace_launch(f, s, b->desc, b->slab, b->basis, b->logs, b->xs, in,
                                          n_in, out, n_out, chunk, (int)slot[f], tr);
        return rev_batch_launch(f, s, b->desc, b->slab, b->basis, b->logs, b->xs, in, n_in, out,
                                n_out, chunk, (int)slot[f]);
    }, &launches);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->h_desc.data(), b->desc, (size_t)count * sizeof(RevBatchDesc),
                           hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    int64_t after = 0;
    for (const RevBatchDesc& d : b->h_desc) {
        after += d.iter;
        if (d.status == LPR_OK_OPTIMAL) res->optimal += 1;
        else if (d.status == LPR_UNBOUNDED) res->unbounded += 1;
        else if (d.status == LPR_INFEASIBLE_BASIS) res->infeasible += 1;
        else if (d.status == LPR_PIVOT_LIMIT) res->limit += 1;
        else res->other += 1;
    }
    res->launches = launches;
    res->iterations = after - before;
    return LPR_OK_OPTIMAL;
}

// Status, iterations (C# `iteration`, :249) and FinalZ (:284; 0 unless optimal) of every LP; any
// may be NULL
int lpr_rev_batch_status_read(lpr_rev_batch* b, int32_t* status, int64_t* iterations, double* z) {
    LPR_LIVE_HANDLE(b, "revised batch");
    for (int32_t k = 0; k < b->count; ++k) {
        const RevBatchDesc& d = b->h_desc[(size_t)k];
        if (status) status[k] = d.status;
        if (iterations) iterations[k] = d.iter;
        if (z) z[k] = d.status == LPR_OK_OPTIMAL ? d.z : 0.0;
    }
    return LPR_OK_OPTIMAL;
}

// SolutionVector (:277-283) of every optimal LP, packed by n[k]; 0 for the others
int lpr_rev_batch_solution_read(lpr_rev_batch* b, double* x) {
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!x) {
        set_error("lpr_rev_batch_solution_read: null x");
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipMemcpyAsync(x, b->xs, (size_t)b->x_total * sizeof(double), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// basicVariables (:28, :195) of every LP, packed by m[k]
int lpr_rev_batch_basis_read(lpr_rev_batch* b, int32_t* basis) {
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!basis) {
        set_error("lpr_rev_batch_basis_read: null basis");
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipMemcpyAsync(basis, b->basis, (size_t)b->basis_n * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// The pivot log of LP k: the first min(iterations, log_cap, cap) (leavingRow :177, enteringIdx
// :122, leavingVar :181) triples
int lpr_rev_batch_log_read(lpr_rev_batch* b, int32_t k, int32_t* row, int32_t* enter,
                           int32_t* leave, int64_t cap, int64_t* count) {
    static const char* W = "lpr_rev_batch_log_read";
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!rb_item_ok(W, b, k)) return LPR_BAD_ARGUMENT;
    if (cap < 0 || !count) {
        set_error("%s: cap %lld < 0 or null count", W, (long long)cap);
        return LPR_BAD_ARGUMENT;
    }
    const RevBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t n = std::min<int64_t>(d.log_fill, cap);
    *count = n;
    if (n == 0) return LPR_OK_OPTIMAL;
    std::vector<int32_t> tmp((size_t)n * 3);
    LPR_HIP(hipMemcpyAsync(tmp.data(), b->logs + 3 * d.log_off, (size_t)n * 3 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    for (int64_t q = 0; q < n; ++q) {
        if (row) row[q] = tmp[(size_t)(3 * q)];
        if (enter) enter[q] = tmp[(size_t)(3 * q + 1)];
        if (leave) leave[q] = tmp[(size_t)(3 * q + 2)];
    }
    return LPR_OK_OPTIMAL;
}

static int rb_slice_read(const char* where, lpr_rev_batch* b, int32_t k, double* out, bool binv) {
    if (!rb_item_ok(where, b, k)) return LPR_BAD_ARGUMENT;
    if (!out) {
        set_error("%s: null output", where);
        return LPR_BAD_ARGUMENT;
    }
    const RevBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t m = d.m;
    const double* src = b->slab + d.s_off + (binv ? 0 : m * m + m * d.n + 2 * m + d.n);
    LPR_HIP(hipMemcpyAsync(out, src, (size_t)(binv ? m * m : m) * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// BInverse (:29) of LP k, m x m row-major
int lpr_rev_batch_binv_read(lpr_rev_batch* b, int32_t k, double* out) {
    LPR_LIVE_HANDLE(b, "revised batch");
    return rb_slice_read("lpr_rev_batch_binv_read", b, k, out, true);
}

// The last x_B = BInverse b (:89) of LP k, m entries
int lpr_rev_batch_xb_read(lpr_rev_batch* b, int32_t k, double* out) {
    LPR_LIVE_HANDLE(b, "revised batch");
    return rb_slice_read("lpr_rev_batch_xb_read", b, k, out, false);
}

// Shape of LP k (n :45, m :46), for callers that size their reads
int lpr_rev_batch_shape(lpr_rev_batch* b, int32_t k, int32_t* n, int32_t* m) {
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!rb_item_ok("lpr_rev_batch_shape", b, k)) return LPR_BAD_ARGUMENT;
    const RevBatchDesc& d = b->h_desc[(size_t)k];
    if (n) *n = d.n;
    if (m) *m = d.m;
    return LPR_OK_OPTIMAL;
}

// ---------------------------------------------------------------- traced batches, section 21

// Records LP k has: one per iteration (:232-247) and the "Optimal" one (:124-146); exact, may
// exceed trace_cap.
static int64_t rb_snapshots(const RevBatchDesc& d) {
    return d.iter + (d.status == LPR_OK_OPTIMAL ? 1 : 0);
}

static bool rb_traced(const char* where, const lpr_rev_batch* b) {
    if (b->trace_cap > 0) return true;
    set_error("%s: the batch is not traced (call lpr_rev_batch_trace_reserve before the first "
              "solve)", where);
    return false;
}

// Makes the handle traced: trace_cap records of rev_trace_stride(m, n) doubles per LP
int lpr_rev_batch_trace_reserve(lpr_rev_batch* b, int32_t trace_cap) {
    static const char* W = "lpr_rev_batch_trace_reserve";
    LPR_LIVE_HANDLE(b, "revised batch");
    if (trace_cap < 1) {
        set_error("%s: trace_cap %d < 1", W, trace_cap);
        return LPR_BAD_ARGUMENT;
    }
    if (b->trace_cap > 0) {
        set_error("%s: the batch is already traced (trace_cap %d)", W, b->trace_cap);
        return LPR_BAD_ARGUMENT;
    }
    if (b->solved) {
        set_error("%s: only before the handle's first lpr_rev_batch_solve", W);
        return LPR_BAD_ARGUMENT;
    }
    std::vector<int64_t> off;
    try {
        off.resize((size_t)b->count);
    } catch (...) {
        return rb_oom("trace offsets", b->count);
    }
    int64_t total = 0;  // 64-bit: a stride is below 2^22 doubles, trace_cap and count below 2^31
    for (int32_t k = 0; k < b->count; ++k) {
        const RevBatchDesc& d = b->h_desc[(size_t)k];
        off[(size_t)k] = total;
        total += (int64_t)trace_cap * rev_trace_stride(d.m, d.n);
    }
    int rc = LPR_OK_OPTIMAL;
    double* slab = nullptr;
    int64_t* d_off = nullptr;
    dev_alloc(&slab, total, "trace: trace_cap x (6 + 7 m + n + m x n + m x m) doubles per LP", &rc,
              rb_oom);
    dev_alloc(&d_off, b->count, "trace offsets", &rc, rb_oom);
    hipStream_t s = b->eng->stream;
    auto upload = [&]() -> int {
        LPR_HIP(hipMemcpyAsync(d_off, off.data(), (size_t)b->count * sizeof(int64_t),
                               hipMemcpyHostToDevice, s));
        // what no record reaches reads as +0.0, the same in every form
        LPR_HIP(hipMemsetAsync(slab, 0, (size_t)total * sizeof(double), s));
        LPR_HIP(hipStreamSynchronize(s));
        return LPR_OK_OPTIMAL;
    };
    if (rc == LPR_OK_OPTIMAL) rc = upload();
    if (rc != LPR_OK_OPTIMAL) {
        hipFree(slab);
        hipFree(d_off);
        return rc;
    }
    b->trace = slab;
    b->trace_off = d_off;
    b->h_trace_off.swap(off);
    b->trace_n = total;
    b->trace_cap = trace_cap;
    return LPR_OK_OPTIMAL;
}

// Per LP: records counted, and where the kept ones are in the trace slab; any may be NULL
int lpr_rev_batch_trace_info(lpr_rev_batch* b, int64_t* snapshots, int64_t* offset,
                             int64_t* stride) {
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!rb_traced("lpr_rev_batch_trace_info", b)) return LPR_BAD_ARGUMENT;
    for (int32_t k = 0; k < b->count; ++k) {
        const RevBatchDesc& d = b->h_desc[(size_t)k];
        if (snapshots) snapshots[k] = rb_snapshots(d);
        if (offset) offset[k] = b->h_trace_off[(size_t)k];
        if (stride) stride[k] = rev_trace_stride(d.m, d.n);
    }
    return LPR_OK_OPTIMAL;
}

// Records [first, first + n) of LP k
int lpr_rev_batch_trace_read(lpr_rev_batch* b, int32_t k, int64_t first, int64_t n, double* out) {
    static const char* W = "lpr_rev_batch_trace_read";
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!rb_traced(W, b) || !rb_item_ok(W, b, k)) return LPR_BAD_ARGUMENT;
    const RevBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t kept = std::min<int64_t>(rb_snapshots(d), b->trace_cap);
    if (first < 0 || n < 0 || first > kept || n > kept - first) {
        set_error("%s: records [%lld, %lld + %lld) of LP %d, which keeps %lld (trace_cap %d)", W,
                  (long long)first, (long long)first, (long long)n, k, (long long)kept,
                  b->trace_cap);
        return LPR_BAD_ARGUMENT;
    }
    if (n == 0) return LPR_OK_OPTIMAL;
    if (!out) {
        set_error("%s: null output", W);
        return LPR_BAD_ARGUMENT;
    }
    const int64_t st = rev_trace_stride(d.m, d.n);
    LPR_HIP(hipMemcpyAsync(out, b->trace + b->h_trace_off[(size_t)k] + first * st,
                           (size_t)(n * st) * sizeof(double), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// The whole trace slab in one copy; cap_doubles is what `out` holds
int lpr_rev_batch_trace_read_all(lpr_rev_batch* b, double* out, int64_t cap_doubles) {
    static const char* W = "lpr_rev_batch_trace_read_all";
    LPR_LIVE_HANDLE(b, "revised batch");
    if (!rb_traced(W, b)) return LPR_BAD_ARGUMENT;
    if (!out || cap_doubles < b->trace_n) {
        set_error("%s: null output, or cap_doubles %lld below the slab's %lld doubles", W,
                  (long long)cap_doubles, (long long)b->trace_n);
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipMemcpyAsync(out, b->trace, (size_t)b->trace_n * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

}  // extern "C"
