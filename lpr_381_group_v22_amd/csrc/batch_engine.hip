// batch_engine.hip -- host side of the batched primal simplex (include/lpr_engine.h, lpr_batch_*;
// DESIGN.md section 12).  Every LP of a batch is solved on the device with the rules of
// PrimalSimplexSolver; the host only picks each LP's form, relaunches the bounded solve kernels
// while LPs are still running (BatchRunLists: one small counter read per launch round) and copies
// results out.  A handle made traced (lpr_batch_trace_*, section 22) launches the traced kernels,
// which also write the tableau after every pivot of every LP.
#include "batch_common.hpp"

#include <algorithm>
#include <climits>

using namespace lpr;

struct lpr_batch {
    lpr_engine* eng = nullptr;
    int32_t count = 0;
    std::vector<BatchDesc> h_desc;  // host mirror, current after every create / solve
    BatchDesc* desc = nullptr;      // device
    double* slab = nullptr;         // every tableau, packed rows x cols row-major
    int32_t* basis = nullptr;       // packed by rows - 1
    int32_t* logs = nullptr;        // packed by log_cap pairs
    BatchRunLists run;              // the running lists and their counters
    double* xz = nullptr;           // extract output: x (x_total) then z (count), lazy
    int64_t slab_n = 0, basis_n = 0, log_n = 0, x_total = 0;
    bool solved = false;               // lpr_batch_solve has run: too late to reserve a trace
    // traced (lpr_batch_trace_reserve): trace_cap records per LP, section 22
    int32_t trace_cap = 0;             // 0: untraced
    double* trace = nullptr;           // device, trace_n doubles
    int64_t* trace_off = nullptr;      // device, per LP
    std::vector<int64_t> h_trace_off;  // LP k's records start at trace + h_trace_off[k]
    int64_t trace_n = 0;
};

namespace {

int batch_oom(const char* what, int64_t n) {
    set_error("lpr_batch: cannot allocate %s (%lld elements)", what, (long long)n);
    return LPR_OUT_OF_MEMORY;
}

void batch_release_device(lpr_batch* b) {
    hipFree(b->desc);
    hipFree(b->slab);
    hipFree(b->basis);
    hipFree(b->logs);
    hipFree(b->xz);
    hipFree(b->trace);
    hipFree(b->trace_off);
    b->trace = nullptr;
    b->trace_off = nullptr;
    b->run.release();
    b->desc = nullptr;
    b->slab = nullptr;
    b->basis = nullptr;
    b->logs = nullptr;
    b->xz = nullptr;
}

// Shapes within form H (rows <= kBatchMaxRowsH, cols <= kBatchMaxColsH) and at least a Z row
// and one column besides the RHS, as lpr_tableau_create requires.
bool batch_shape_ok(const char* where, int32_t k, int64_t rows, int64_t cols) {
    if (rows < 1 || cols < 2) {
        set_error("%s: LP %d has a %lld x %lld tableau; it needs rows >= 1 and cols >= 2", where,
                  k, (long long)rows, (long long)cols);
        return false;
    }
    if (rows > kBatchMaxRowsH || cols > kBatchMaxColsH) {
        set_error("%s: LP %d has a %lld x %lld tableau, beyond the batch limit of %d x %d (form "
                  "H); solve it alone with lpr_primal_solve",
                  where, k, (long long)rows, (long long)cols, kBatchMaxRowsH, kBatchMaxColsH);
        return false;
    }
    return true;
}

// Offsets and device memory for `count` LPs of the given shapes.  On failure nothing is left.
int batch_alloc(lpr_engine* e, int32_t count, const std::vector<int32_t>& R,
                const std::vector<int32_t>& Cc, const std::vector<int32_t>& nv, int32_t log_cap,
                lpr_batch** out) {
    lpr_batch* b = new (std::nothrow) lpr_batch();
    if (!b) return batch_oom("handle", 1);
    b->eng = e;
    b->count = count;
    try {
        b->h_desc.resize((size_t)count);
    } catch (...) {
        delete b;
        return batch_oom("descriptors", count);
    }
    int64_t t = 0, bs = 0, lg = 0, x = 0;
    for (int32_t k = 0; k < count; ++k) {
        BatchDesc& d = b->h_desc[(size_t)k];
        d.rows = R[(size_t)k];
        d.cols = Cc[(size_t)k];
        d.n = nv[(size_t)k];
        d.log_cap = log_cap > 0 ? log_cap
                                : std::min<int32_t>(kBatchLogDefaultMax, 4 * (d.rows + d.cols));
        d.t_off = t;
        d.b_off = bs;
        d.log_off = lg;
        d.x_off = x;
        d.iter = 0;
        d.max_iter = 0;
        d.status = kRunning;
        d.log_fill = 0;
        // no overflow: each term is below 2^22 and count below 2^31
        t += (int64_t)d.rows * d.cols;
        bs += d.rows - 1;
        lg += d.log_cap;
        x += d.n;
    }
    b->slab_n = t;
    b->basis_n = bs;
    b->log_n = lg;
    b->x_total = x;
    int rc = LPR_OK_OPTIMAL;
    // the message gives the entries asked for (n), which a padded or paired allocation exceeds
    auto oom_n = [](int64_t n) {
        return [n](const char* what, int64_t) { return batch_oom(what, n); };
    };
    dev_alloc(&b->desc, count, "descriptors", &rc, batch_oom);
    dev_alloc(&b->slab, std::max<int64_t>(t, 1), "tableau slab", &rc, oom_n(t));
    dev_alloc(&b->basis, std::max<int64_t>(bs, 1), "bases", &rc, oom_n(bs));
    dev_alloc(&b->logs, std::max<int64_t>(lg, 1) * 2, "pivot logs", &rc, oom_n(lg));
    b->run.alloc(count, &rc, batch_oom);
    if (rc == LPR_OK_OPTIMAL &&
        hipMemcpy(b->desc, b->h_desc.data(), (size_t)count * sizeof(BatchDesc),
                  hipMemcpyHostToDevice) != hipSuccess) {
        set_error("lpr_batch: descriptor upload failed");
        rc = LPR_DEVICE_ERROR;
    }
    if (rc != LPR_OK_OPTIMAL) {
        batch_release_device(b);
        delete b;
        return rc;
    }
    *out = b;
    return LPR_OK_OPTIMAL;
}

}  // namespace

namespace lpr {
void batch_orphan(lpr_batch* b) {  // lpr_engine_close
    batch_release_device(b);
    b->eng = nullptr;
}
// What lpr_bb_batch_from_batch reads of a batch: its engine (null once orphaned), the host mirror
// of its descriptors and the tableau slab.
lpr_engine* batch_view(lpr_batch* b, const std::vector<BatchDesc>** desc, const double** slab) {
    if (!b) return nullptr;
    *desc = &b->h_desc;
    *slab = b->slab;
    return b->eng;
}
int32_t batch_trace_view(lpr_batch* b, const double** trace, const std::vector<int64_t>** off) {
    *trace = b->trace;
    *off = &b->h_trace_off;
    return b->trace_cap;
}
}  // namespace lpr

extern "C" {

// new PrimalSimplexSolver(objective, constraints, isMaximization) per LP
// (Simplex/PrimalSimplexSolver.cs:27-87), built on the device
int lpr_batch_from_lps(lpr_engine* e, int32_t count, const int32_t* n, const int32_t* m,
                       const double* objective, const double* A, const int32_t* ncoef,
                       const int8_t* relation, const double* rhs, const int8_t* is_max,
                       int32_t log_cap, lpr_batch** out) {
    static const char* W = "lpr_batch_from_lps";
    if (!e || !out || count < 1 || !n || !m || !is_max || log_cap < 0) {
        set_error("%s: bad arguments (count=%d, log_cap=%d, or a null engine / handle / n / m / "
                  "is_max)", W, count, log_cap);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    std::vector<int32_t> R((size_t)count), Cc((size_t)count), nv((size_t)count);
    std::vector<BatchBuild> bd((size_t)count);
    int64_t so = 0, sa = 0, sr = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (n[k] < 0 || m[k] < 0) {
            set_error("%s: LP %d has n=%d m=%d; both must be >= 0", W, k, n[k], m[k]);
            return LPR_BAD_ARGUMENT;
        }
        const int64_t rows = (int64_t)m[k] + 1, cols = (int64_t)n[k] + m[k] + 1;
        if (!batch_shape_ok(W, k, rows, cols)) return LPR_BAD_ARGUMENT;
        R[(size_t)k] = (int32_t)rows;
        Cc[(size_t)k] = (int32_t)cols;
        nv[(size_t)k] = n[k];
        bd[(size_t)k] = BatchBuild{so, sa, sr};
        so += n[k];
        sa += (int64_t)m[k] * n[k];
        sr += m[k];
    }
    if ((so > 0 && !objective) || (sa > 0 && !A) || (sr > 0 && (!relation || !rhs))) {
        set_error("%s: null objective / A / relation / rhs for a batch that has entries", W);
        return LPR_BAD_ARGUMENT;
    }
    for (int32_t k = 0; k < count; ++k) {
        for (int32_t i = 0; i < m[k]; ++i) {
            const int64_t at = bd[(size_t)k].row_off + i;
            if (ncoef && (ncoef[at] < 0 || ncoef[at] > n[k])) {
                set_error("%s: LP %d row %d has ncoef=%d outside [0, %d]", W, k, i, ncoef[at],
                          n[k]);
                return LPR_BAD_ARGUMENT;
            }
            if (relation[at] != LPR_REL_LE && relation[at] != LPR_REL_GE &&
                relation[at] != LPR_REL_EQ) {
                set_error("%s: LP %d row %d has relation code %d (LPR_REL_LE/GE/EQ are 0/1/2)", W,
                          k, i, (int)relation[at]);
                return LPR_BAD_ARGUMENT;
            }
        }
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_batch* b = nullptr;
    int rc = batch_alloc(e, count, R, Cc, nv, log_cap, &b);
    if (rc != LPR_OK_OPTIMAL) return rc;
    hipStream_t s = e->stream;
    double *d_obj = nullptr, *d_A = nullptr, *d_rhs = nullptr;
    int32_t* d_nc = nullptr;
    int8_t *d_rel = nullptr, *d_max = nullptr;
    BatchBuild* d_bd = nullptr;
    bool oom = false;
    hipError_t err = hipSuccess;
    auto up = [&](auto** dst, const auto* src, int64_t cnt) {
        if (oom || err != hipSuccess || cnt <= 0 || !src) return;
        const size_t bytes = (size_t)cnt * sizeof(*src);
        if (hipMalloc(reinterpret_cast<void**>(dst), bytes) != hipSuccess) {
            oom = true;
            return;
        }
        err = hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, s);
    };
    up(&d_obj, objective, so);
    up(&d_A, A, sa);
    up(&d_nc, ncoef, sr);
    up(&d_rel, relation, sr);
    up(&d_rhs, rhs, sr);
    up(&d_max, is_max, (int64_t)count);
    up(&d_bd, bd.data(), (int64_t)count);
    if (!oom && err == hipSuccess) {
        batch_launch_build(s, b->desc, d_bd, count, b->slab, b->basis, d_obj, d_A, d_nc, d_rel,
                           d_rhs, d_max);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipStreamSynchronize(s);  // inputs are borrowed
    }
    hipFree(d_obj);
    hipFree(d_A);
    hipFree(d_nc);
    hipFree(d_rel);
    hipFree(d_rhs);
    hipFree(d_max);
    hipFree(d_bd);
    if (oom || err != hipSuccess) {
        if (oom)
            rc = batch_oom("build inputs", sa);
        else {
            set_error("%s: %s", W, hipGetErrorString(err));
            rc = LPR_DEVICE_ERROR;
        }
        batch_release_device(b);
        delete b;
        return rc;
    }
    e->live_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

// Ready tableaux, as lpr_tableau_create adopts one (BranchAndBoundAdapter.cs:31-46) per LP
int lpr_batch_create(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                     const double* tableaux, const int32_t* basis, int32_t log_cap,
                     lpr_batch** out) {
    static const char* W = "lpr_batch_create";
    if (!e || !out || count < 1 || !rows || !cols || !tableaux || log_cap < 0) {
        set_error("%s: bad arguments (count=%d, log_cap=%d, or a null engine / handle / rows / "
                  "cols / tableaux)", W, count, log_cap);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    std::vector<int32_t> R((size_t)count), Cc((size_t)count), nv((size_t)count);
    for (int32_t k = 0; k < count; ++k) {
        if (!batch_shape_ok(W, k, rows[k], cols[k])) return LPR_BAD_ARGUMENT;
        R[(size_t)k] = rows[k];
        Cc[(size_t)k] = cols[k];
        nv[(size_t)k] = std::max(0, cols[k] - rows[k]);  // [A | I | b]: n = cols - rows
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_batch* b = nullptr;
    int rc = batch_alloc(e, count, R, Cc, nv, log_cap, &b);
    if (rc != LPR_OK_OPTIMAL) return rc;
    hipStream_t s = e->stream;
    hipError_t err = hipMemcpyAsync(b->slab, tableaux, (size_t)b->slab_n * sizeof(double),
                                    hipMemcpyHostToDevice, s);
    if (err == hipSuccess && b->basis_n > 0) {
        if (basis)
            err = hipMemcpyAsync(b->basis, basis, (size_t)b->basis_n * sizeof(int32_t),
                                 hipMemcpyHostToDevice, s);
        else
            err = hipMemsetAsync(b->basis, 0xff, (size_t)b->basis_n * sizeof(int32_t), s);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) {
        set_error("%s: %s", W, hipGetErrorString(err));
        batch_release_device(b);
        delete b;
        return LPR_DEVICE_ERROR;
    }
    e->live_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

int lpr_batch_destroy(lpr_batch* b) {
    if (!b) return LPR_BAD_ARGUMENT;
    if (b->eng) {
        hipSetDevice(b->eng->device);
        hipStreamSynchronize(b->eng->stream);
        batch_release_device(b);
        unlist(b->eng->live_batch, b);
    }
    delete b;
    return LPR_OK_OPTIMAL;
}

// PrimalSimplexSolver.Solve() (:102-150) for every LP that is not finished
int lpr_batch_solve(lpr_batch* b, const lpr_batch_opts* opts, lpr_batch_result* res) {
    LPR_LIVE_HANDLE(b, "batch");
    if (!res) {
        set_error("lpr_batch_solve: null result");
        return LPR_BAD_ARGUMENT;
    }
    lpr_batch_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (o.variant < 0 || o.variant > 3 || o.chunk < 0) {
        set_error("lpr_batch_solve: variant %d (0 auto, 1 W, 2 G, 3 H) / chunk %d (>= 0)",
                  o.variant, o.chunk);
        return LPR_BAD_ARGUMENT;
    }
    std::memset(res, 0, sizeof *res);
    hipStream_t s = b->eng->stream;
    const int32_t count = b->count;
    // the running lists, one contiguous range per form
    std::vector<int32_t> lists[kNumForms];
    int slot[kNumForms] = {0, 0, 0};
    int max_rows = 0, max_cols = 0;
    int64_t before = 0;
    for (int32_t k = 0; k < count; ++k) {
        BatchDesc& d = b->h_desc[(size_t)k];
        before += d.iter;
        if (d.status != kRunning && d.status != LPR_PIVOT_LIMIT) continue;  // finished stays so
        d.status = kRunning;
        d.max_iter = o.max_pivots > 0 ? d.iter + o.max_pivots : 0;
        // one footprint and one form rule, traced or not: the trace adds nothing to LDS
        const size_t fp = batch_footprint(d.rows, d.cols);
        const int f = batch_pick_form(fp * sizeof(double), o.variant);
        lists[f].push_back(k);
        if (f == kFormH) {
            max_rows = std::max(max_rows, d.rows);
            max_cols = std::max(max_cols, d.cols);
        } else {
            slot[f] = std::max(slot[f], ((int)fp + 1) & ~1);
        }
    }
    int rc = b->run.upload(s, lists);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->desc, b->h_desc.data(), (size_t)count * sizeof(BatchDesc),
                           hipMemcpyHostToDevice, s));
    int launches = 0;
    b->solved = true;
    const BatchTrace tr{b->trace, b->trace_off, b->trace_cap};
    rc = b->run.rounds(s, [&](int f, const int32_t* in, int n_in, int32_t* out, int32_t* n_out) {
        const int chunk = o.chunk > 0 ? o.chunk : kBatchChunk[f];
        if (b->trace_cap > 0)
            return batch_trace_launch_simplex(f, s, b->desc, b->slab, b->basis, b->logs, in, n_in,
                                              out, n_out, chunk, slot[f], max_rows, max_cols, tr);
        return batch_launch_simplex(f, s, b->desc, b->slab, b->basis, b->logs, in, n_in, out,
                                    n_out, chunk, slot[f], max_rows, max_cols);
    }, &launches);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->h_desc.data(), b->desc, (size_t)count * sizeof(BatchDesc),
                           hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    int64_t after = 0;
    for (const BatchDesc& d : b->h_desc) {
        after += d.iter;
        res->optimal += d.status == LPR_OK_OPTIMAL;
        res->unbounded += d.status == LPR_UNBOUNDED;
        res->limit += d.status == LPR_PIVOT_LIMIT;
    }
    res->launches = launches;
    res->pivots = after - before;
    return LPR_OK_OPTIMAL;
}

static int batch_extract(lpr_batch* b, bool want_x) {
    if (!b->xz) {
        const int64_t need = b->x_total + b->count;
        if (hipMalloc(&b->xz, (size_t)need * sizeof(double)) != hipSuccess)
            return batch_oom("solution buffer", need);
    }
    batch_launch_extract(b->eng->stream, b->desc, b->count, b->slab, want_x ? b->xz : nullptr,
                         b->xz + b->x_total);
    LPR_HIP(hipGetLastError());
    return LPR_OK_OPTIMAL;
}

// Status, pivots (C# `iteration`) and FinalZ = T[0, cols-1] (:113) of every LP; any may be NULL
int lpr_batch_status_read(lpr_batch* b, int32_t* status, int64_t* pivots, double* z) {
    LPR_LIVE_HANDLE(b, "batch");
    for (int32_t k = 0; k < b->count; ++k) {
        if (status) status[k] = b->h_desc[(size_t)k].status;
        if (pivots) pivots[k] = b->h_desc[(size_t)k].iter;
    }
    if (!z) return LPR_OK_OPTIMAL;
    const int rc = batch_extract(b, false);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(z, b->xz + b->x_total, (size_t)b->count * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// ExtractSolution() (:213-252) of every optimal LP, packed by n[k]; 0 for the others
int lpr_batch_solution_read(lpr_batch* b, double* x) {
    LPR_LIVE_HANDLE(b, "batch");
    if (!x) {
        set_error("lpr_batch_solution_read: null x");
        return LPR_BAD_ARGUMENT;
    }
    if (b->x_total == 0) return LPR_OK_OPTIMAL;
    const int rc = batch_extract(b, true);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(x, b->xz, (size_t)b->x_total * sizeof(double), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// basicVariables (:18-24, :142) of every LP, packed by rows[k] - 1
int lpr_batch_basis_read(lpr_batch* b, int32_t* basis) {
    LPR_LIVE_HANDLE(b, "batch");
    if (!basis) {
        set_error("lpr_batch_basis_read: null basis");
        return LPR_BAD_ARGUMENT;
    }
    if (b->basis_n == 0) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(basis, b->basis, (size_t)b->basis_n * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// The pivot log of LP k (:138): the first min(pivots, log_cap, cap) (row, col) pairs
int lpr_batch_log_read(lpr_batch* b, int32_t k, int32_t* rows, int32_t* cols, int64_t cap,
                       int64_t* count) {
    LPR_LIVE_HANDLE(b, "batch");
    if (k < 0 || k >= b->count || cap < 0 || !count) {
        set_error("lpr_batch_log_read: LP %d out of range (0..%d), cap %lld or null count", k,
                  b->count - 1, (long long)cap);
        return LPR_BAD_ARGUMENT;
    }
    const BatchDesc& d = b->h_desc[(size_t)k];
    const int64_t n = std::min<int64_t>(d.log_fill, cap);
    *count = n;
    if (n == 0) return LPR_OK_OPTIMAL;
    std::vector<int32_t> tmp((size_t)n * 2);
    LPR_HIP(hipMemcpyAsync(tmp.data(), b->logs + 2 * d.log_off, (size_t)n * 2 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    for (int64_t q = 0; q < n; ++q) {
        if (rows) rows[q] = tmp[(size_t)(2 * q)];
        if (cols) cols[q] = tmp[(size_t)(2 * q + 1)];
    }
    return LPR_OK_OPTIMAL;
}

// The tableau of LP k (FinalTableau, :18-24), rows[k] x cols[k] row-major
int lpr_batch_tableau_read(lpr_batch* b, int32_t k, double* rowmajor) {
    LPR_LIVE_HANDLE(b, "batch");
    if (k < 0 || k >= b->count || !rowmajor) {
        set_error("lpr_batch_tableau_read: LP %d out of range (0..%d) or null output", k,
                  b->count - 1);
        return LPR_BAD_ARGUMENT;
    }
    const BatchDesc& d = b->h_desc[(size_t)k];
    LPR_HIP(hipMemcpyAsync(rowmajor, b->slab + d.t_off,
                           (size_t)d.rows * d.cols * sizeof(double), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// Shape of LP k (rows, cols, n), for callers that size their reads
int lpr_batch_shape(lpr_batch* b, int32_t k, int32_t* rows, int32_t* cols, int32_t* n) {
    LPR_LIVE_HANDLE(b, "batch");
    if (k < 0 || k >= b->count) {
        set_error("lpr_batch_shape: LP %d out of range (0..%d)", k, b->count - 1);
        return LPR_BAD_ARGUMENT;
    }
    const BatchDesc& d = b->h_desc[(size_t)k];
    if (rows) *rows = d.rows;
    if (cols) *cols = d.cols;
    if (n) *n = d.n;
    return LPR_OK_OPTIMAL;
}

// ---------------------------------------------------------------- traced batches, section 22

// Records LP k has: the tableau as built (:86) and one per pivot (:148); exact, may exceed
// trace_cap.  The C#'s list also ends with a block formatted from the final tableau (:118-122,
// :133), which lpr_batch_tableau_read gives.
static int64_t batch_records(const BatchDesc& d) { return 1 + d.iter; }

static bool batch_traced(const char* where, const lpr_batch* b) {
    if (b->trace_cap > 0) return true;
    set_error("%s: the batch is not traced (call lpr_batch_trace_reserve before the first solve)",
              where);
    return false;
}

// IterationSnapshots of PrimalSimplexSolver (:86, :148) as numbers: makes the handle traced,
// trace_cap records of batch_trace_stride(rows, cols) doubles per LP, record 0 written here
int lpr_batch_trace_reserve(lpr_batch* b, int32_t trace_cap) {
    static const char* W = "lpr_batch_trace_reserve";
    LPR_LIVE_HANDLE(b, "batch");
    if (trace_cap < 1) {
        set_error("%s: trace_cap %d < 1", W, trace_cap);
        return LPR_BAD_ARGUMENT;
    }
    if (b->trace_cap > 0) {
        set_error("%s: the batch is already traced (trace_cap %d)", W, b->trace_cap);
        return LPR_BAD_ARGUMENT;
    }
    if (b->solved) {
        set_error("%s: only before the handle's first lpr_batch_solve", W);
        return LPR_BAD_ARGUMENT;
    }
    static const char* kSlab = "trace slab: trace_cap records of a header and rows x cols doubles "
                               "per LP";
    std::vector<int64_t> off;
    try {
        off.resize((size_t)b->count);
    } catch (...) {
        return batch_oom("trace offsets", b->count);
    }
    // a stride is below 2^22 doubles, trace_cap and count below 2^31: the sum can pass 2^63
    int64_t total = 0;
    for (int32_t k = 0; k < b->count; ++k) {
        const BatchDesc& d = b->h_desc[(size_t)k];
        const int64_t mine = (int64_t)trace_cap * batch_trace_stride(d.rows, d.cols);  // < 2^53
        off[(size_t)k] = total;
        if (total > INT64_MAX / (int64_t)sizeof(double) - mine) {
            set_error("lpr_batch: cannot allocate %s (trace_cap %d: more than 2^63 bytes at LP %d "
                      "of %d)", kSlab, trace_cap, k, b->count);
            return LPR_OUT_OF_MEMORY;
        }
        total += mine;
    }
    int rc = LPR_OK_OPTIMAL;
    double* slab = nullptr;
    int64_t* d_off = nullptr;
    dev_alloc(&slab, total, kSlab, &rc, batch_oom);
    dev_alloc(&d_off, b->count, "trace offsets", &rc, batch_oom);
    hipStream_t s = b->eng->stream;
    auto fill = [&]() -> int {
        LPR_HIP(hipMemcpyAsync(d_off, off.data(), (size_t)b->count * sizeof(int64_t),
                               hipMemcpyHostToDevice, s));
        // what no record reaches reads as +0.0, the same in every form
        LPR_HIP(hipMemsetAsync(slab, 0, (size_t)total * sizeof(double), s));
        batch_trace_launch_first(s, b->desc, b->count, b->slab, BatchTrace{slab, d_off, trace_cap});
        LPR_HIP(hipGetLastError());
        LPR_HIP(hipStreamSynchronize(s));
        return LPR_OK_OPTIMAL;
    };
    if (rc == LPR_OK_OPTIMAL) rc = fill();
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

// Per LP: records counted (1 + `iteration`, :137), and where the kept ones are in the trace slab;
// any may be NULL
int lpr_batch_trace_info(lpr_batch* b, int64_t* records, int64_t* offset, int64_t* stride) {
    LPR_LIVE_HANDLE(b, "batch");
    if (!batch_traced("lpr_batch_trace_info", b)) return LPR_BAD_ARGUMENT;
    for (int32_t k = 0; k < b->count; ++k) {
        const BatchDesc& d = b->h_desc[(size_t)k];
        if (records) records[k] = batch_records(d);
        if (offset) offset[k] = b->h_trace_off[(size_t)k];
        if (stride) stride[k] = batch_trace_stride(d.rows, d.cols);
    }
    return LPR_OK_OPTIMAL;
}

// Records [first, first + n) of LP k: the tableaux of :86 and :148 with their pivots (:138)
int lpr_batch_trace_read(lpr_batch* b, int32_t k, int64_t first, int64_t n, double* out) {
    static const char* W = "lpr_batch_trace_read";
    LPR_LIVE_HANDLE(b, "batch");
    if (!batch_traced(W, b)) return LPR_BAD_ARGUMENT;
    if (k < 0 || k >= b->count) {
        set_error("%s: LP %d out of range (0..%d)", W, k, b->count - 1);
        return LPR_BAD_ARGUMENT;
    }
    const BatchDesc& d = b->h_desc[(size_t)k];
    const int64_t kept = std::min<int64_t>(batch_records(d), b->trace_cap);
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
    const int64_t st = batch_trace_stride(d.rows, d.cols);
    LPR_HIP(hipMemcpyAsync(out, b->trace + b->h_trace_off[(size_t)k] + first * st,
                           (size_t)(n * st) * sizeof(double), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// The whole trace slab in one copy (every LP's :86 and :148 tableaux); cap_doubles is what `out`
// holds
int lpr_batch_trace_read_all(lpr_batch* b, double* out, int64_t cap_doubles) {
    static const char* W = "lpr_batch_trace_read_all";
    LPR_LIVE_HANDLE(b, "batch");
    if (!batch_traced(W, b)) return LPR_BAD_ARGUMENT;
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
