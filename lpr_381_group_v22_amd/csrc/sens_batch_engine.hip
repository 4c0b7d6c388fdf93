// sens_batch_engine.hip -- host side of the sensitivity scenario batch (include/lpr_engine.h,
// lpr_sens_batch_*).  Every scenario runs its whole script on the device
// with the rules of SensitivityAnalyzer; the host copies the base state in, relaunches the
// bounded script kernel while scenarios are still running (BatchRunLists of batch_common.hpp,
// with one form per call) and copies results out.  lpr_sens_batch_from_batch (section 20) starts
// every scenario from an LP of a solved LP batch instead: the analyzer's constructor runs per
// scenario on the device.
#include "sens_batch_common.hpp"

#include <algorithm>
#include <cstdio>
#include <new>
#include <string>

using namespace lpr;

struct lpr_sens_batch {
    lpr_engine* eng = nullptr;
    int32_t count = 0;
    int64_t total_edits = 0;
    int form = 0;  // the form of the last run (0: none yet)
    bool grow = false;         // from lpr_sens_batch_create_grow: scripts may hold the add edits
    int32_t base_R = 0, base_C = 0;  // the base's shape (vw.R x vw.C is the maximal one); from an
                                     // LP batch: the largest base shape over the chosen LPs
    int32_t min_R = 0;         // the least row count of a base (base_R unless from an LP batch)
    double ctor_ms = -1.0;     // lpr_sens_batch_from_batch: the constructor kernel, from events
    SensBatchView vw{};
    std::vector<SensScenario> h_desc;  // host mirror, current after create and every run
    lpr_sens_edit* d_edits = nullptr;
    double* d_payload = nullptr;
    BatchRunLists run;  // the running lists and their counters; one form per call
    // lpr_sens_batch_ranging: the output block (device) and its pinned mirror, allocated at the
    // first call (the batch's maximal shape never changes), and the events around the kernel
    char* rng_out = nullptr;
    char* rng_pin = nullptr;
    hipEvent_t rng_ev[2] = {nullptr, nullptr};
    bool rng_timed = false;
};

namespace {

int sb_oom(const char* what, int64_t n) {
    set_error("lpr_sens_batch: cannot allocate %s (%lld elements)", what, (long long)n);
    return LPR_OUT_OF_MEMORY;
}

void sb_release_device(lpr_sens_batch* b) {
    SensBatchView& v = b->vw;
    hipFree(v.desc); hipFree(v.cur); hipFree(v.alt); hipFree(v.basic); hipFree(v.bcount);
    hipFree(v.snap); hipFree(v.sol); hipFree(v.log); hipFree(v.outcome); hipFree(v.edit_piv);
    hipFree(b->d_edits); hipFree(b->d_payload);
    b->run.release();
    hipFree(b->rng_out);
    if (b->rng_pin) hipHostFree(b->rng_pin);
    b->rng_out = b->rng_pin = nullptr;
    for (hipEvent_t& ev : b->rng_ev) {
        if (ev) hipEventDestroy(ev);
        ev = nullptr;
    }
    b->rng_timed = false;
    v.desc = nullptr;
    v.cur = v.alt = v.sol = nullptr;
    v.basic = v.bcount = v.snap = v.log = v.outcome = nullptr;
    v.edit_piv = nullptr;
    v.edits = nullptr;
    v.payload = nullptr;
    b->d_edits = nullptr;
    b->d_payload = nullptr;
}

int sb_fail(lpr_sens_batch* b, int rc) {
    sb_release_device(b);
    delete b;
    return rc;
}

// lpr_sens_batch_from_batch: what the scenarios are constructed on instead of a base analyzer
struct SbModels {
    lpr_engine* eng;                    // the LP batch's engine
    const std::vector<BatchDesc>* bd;   // its descriptors (host mirror) and tableau slab
    const double* slab;
    const int32_t* item;                // the LP of scenario k; null: LP k
};

// The LP of every scenario checked and listed; *R x *C is the largest base shape, *min_R the
// least row count and *nsol the longest solutionVector.
int sb_models(const char* W, const SbModels& md, int32_t count, std::vector<SensModelSrc>* srcs,
              int* R, int* C, int* min_R, int* nsol) {
    const int32_t have = (int32_t)md.bd->size();
    if (!md.item && count != have) {
        set_error("%s: count=%d without an item list; the LP batch holds %d LPs", W, count, have);
        return LPR_BAD_ARGUMENT;
    }
    try {
        srcs->resize((size_t)count);
    } catch (...) {
        return sb_oom("item list (host)", count);
    }
    *R = *C = *nsol = 0;
    *min_R = INT32_MAX;
    for (int32_t k = 0; k < count; ++k) {
        const int32_t it = md.item ? md.item[k] : k;
        if (it < 0 || it >= have) {
            set_error("%s: scenario %d names item %d, outside the LP batch's 0..%d", W, k, it,
                      have - 1);
            return LPR_BAD_ARGUMENT;
        }
        const BatchDesc& d = (*md.bd)[(size_t)it];
        if (d.status != LPR_OK_OPTIMAL) {
            set_error("%s: scenario %d names item %d, which has no optimal final tableau (status "
                      "%d: %s); the analyzer takes the SolutionVector of an optimal solve", W, k, it,
                      d.status,
                      d.status == kRunning ? "not solved"
                      : d.status == LPR_PIVOT_LIMIT ? "stopped at its pivot limit"
                      : d.status == LPR_UNBOUNDED ? "unbounded" : "not optimal");
            return LPR_BAD_ARGUMENT;
        }
        if (d.cols < d.rows || d.n < 0 || d.n > d.cols - 1) {
            set_error("%s: scenario %d names item %d, a %d x %d tableau with n=%d; an analyzer "
                      "needs cols >= rows (lpr_sens_create) and 0 <= n < cols", W, k, it, d.rows,
                      d.cols, d.n);
            return LPR_BAD_ARGUMENT;
        }
        SensModelSrc& s = (*srcs)[(size_t)k];
        s.t_off = d.t_off;
        s.rows = d.rows;
        s.cols = d.cols;
        s.n = d.n;
        s.item = it;
        *R = std::max(*R, (int)d.rows);
        *C = std::max(*C, (int)d.cols);
        *min_R = std::min(*min_R, (int)d.rows);
        *nsol = std::max(*nsol, (int)d.n);
    }
    return LPR_OK_OPTIMAL;
}

// count scenarios, one script each: private copies of the state of `base`
// (SensitivityAnalyzer.cs:14-18), or with `md` (base null) a fresh analyzer per scenario on an LP of
// a solved LP batch.  W names the call in messages; grow: the scripts may hold the two add edits,
// whose columns and rows lie in `payload`.
int sb_create(const char* W, bool grow, lpr_sens* base, const SbModels* md, int32_t count,
              const int32_t* nedits, const lpr_sens_edit* edits, const double* payload,
              int64_t npayload, int32_t log_cap, lpr_sens_batch** out) {
    int R = 0, C = 0, ld = 0;  // the base's shape; with md the largest one
    const double* baseT = nullptr;
    const int32_t *base_basic = nullptr, *base_bcount = nullptr;
    const std::vector<double>* base_sol = nullptr;
    double z = 0.0;
    lpr_engine* e = md ? md->eng : sens_view(base, &R, &C, &ld, &baseT, &base_basic, &base_bcount,
                                             &base_sol, &z);
    if (!e) {
        set_error("%s: the base handle is null or orphaned: its engine has been closed", W);
        return LPR_BAD_ARGUMENT;
    }
    if (!out || count < 1 || !nedits || log_cap < 0) {
        set_error("%s: bad arguments (count=%d, log_cap=%d, or a null handle / nedits)", W, count,
                  log_cap);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    std::vector<SensModelSrc> srcs;  // md: the LP of every scenario
    int min_R = 0, nsol = 0;
    if (md) {
        const int rc = sb_models(W, *md, count, &srcs, &R, &C, &min_R, &nsol);
        if (rc != LPR_OK_OPTIMAL) return rc;
    } else {
        min_R = R;
        nsol = (int)base_sol->size();
    }
    // "scenario k", with the LP it names where there is one
    auto who = [&](int32_t k) {
        char buf[64];
        if (md)
            std::snprintf(buf, sizeof buf, "scenario %d (item %d)", k, srcs[(size_t)k].item);
        else
            std::snprintf(buf, sizeof buf, "scenario %d", k);
        return std::string(buf);
    };
    if (R > kBatchMaxRowsH || C > kBatchMaxColsH) {
        set_error("%s: the base is a %d x %d tableau, beyond the batch limit of %d x %d (form H); "
                  "edit it alone with lpr_sens_*", W, R, C, kBatchMaxRowsH, kBatchMaxColsH);
        return LPR_BAD_ARGUMENT;
    }
    if (grow && (npayload < 0 || npayload > INT32_MAX || (npayload > 0 && !payload))) {
        set_error("%s: npayload=%lld must lie in 0..2^31-1, with a payload where it is not 0", W,
                  (long long)npayload);
        return LPR_BAD_ARGUMENT;
    }
    int64_t total = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (nedits[k] < 0) {
            set_error("%s: scenario %d has nedits=%d; it must be >= 0", W, k, nedits[k]);
            return LPR_BAD_ARGUMENT;
        }
        total += nedits[k];
    }
    if (total > 0 && !edits) {
        set_error("%s: null edits for scripts that have entries", W);
        return LPR_BAD_ARGUMENT;
    }
    int maxR = R, maxC = C;  // the largest shape any script can reach
    if (!grow) {
        for (int64_t q = 0; q < total; ++q) {
            const int op = edits[q].op;
            if (op < LPR_SENS_EDIT_RESOLVE_ALL || op > LPR_SENS_EDIT_NONBASIC_COLUMN) {
                set_error("%s: edit %lld has op %d; a batch takes the ops 0..4 that keep the "
                          "tableau's shape -- AddNewActivity / AddNewConstraint go through "
                          "lpr_sens_add_activity / lpr_sens_add_constraint on a single handle, or "
                          "lpr_sens_batch_create_grow", W, (long long)q, op);
                return LPR_BAD_ARGUMENT;
            }
        }
    } else {
        int64_t q = 0;
        for (int32_t k = 0; k < count; ++k) {
            const int R0 = md ? srcs[(size_t)k].rows : R, C0 = md ? srcs[(size_t)k].cols : C;
            int rows = R0, cols = C0;
            for (int32_t i = 0; i < nedits[k]; ++i, ++q) {
                const lpr_sens_edit& ed = edits[q];
                if (ed.op < LPR_SENS_EDIT_RESOLVE_ALL || ed.op > LPR_SENS_EDIT_ADD_CONSTRAINT) {
                    set_error("%s: %s edit %d has op %d; the ops are 0..6", W, who(k).c_str(), i,
                              ed.op);
                    return LPR_BAD_ARGUMENT;
                }
                if (ed.op < LPR_SENS_EDIT_ADD_ACTIVITY) continue;
                if (ed.b < 0 || ed.a < 0 || (int64_t)ed.a + ed.b > npayload) {
                    set_error("%s: %s edit %d (op %d) takes payload [%d, %d + %d), "
                              "outside [0, %lld)", W, who(k).c_str(), i, ed.op, ed.a, ed.a, ed.b,
                              (long long)npayload);
                    return LPR_BAD_ARGUMENT;
                }
                rows += ed.op == LPR_SENS_EDIT_ADD_CONSTRAINT;
                cols += 1;
                if (rows > kBatchMaxRowsH || cols > kBatchMaxColsH) {
                    set_error("%s: %s edit %d can grow the %d x %d base to %d x %d, "
                              "beyond the batch limit of %d x %d (form H)", W, who(k).c_str(), i,
                              R0, C0, rows, cols, kBatchMaxRowsH, kBatchMaxColsH);
                    return LPR_BAD_ARGUMENT;
                }
            }
            maxR = std::max(maxR, rows);
            maxC = std::max(maxC, cols);
        }
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_sens_batch* b = new (std::nothrow) lpr_sens_batch();
    if (!b) return sb_oom("handle", 1);
    b->eng = e;
    b->count = count;
    b->total_edits = total;
    b->grow = grow;
    b->base_R = R;
    b->base_C = C;
    b->min_R = min_R;
    SensBatchView& v = b->vw;
    v.R = maxR;
    v.C = maxC;
    v.sol_cap = std::max(std::max(nsol, maxC - 1), 1);
    v.log_cap = log_cap > 0 ? log_cap : std::min<int32_t>(kBatchLogDefaultMax, 4 * (R + C));
    try {
        b->h_desc.resize((size_t)count);
    } catch (...) {
        delete b;
        return sb_oom("descriptors", count);
    }
    int64_t at = 0;
    for (int32_t k = 0; k < count; ++k) {
        SensScenario& d = b->h_desc[(size_t)k];
        std::memset(&d, 0, sizeof d);
        d.z = z;
        d.old_z = z;
        d.edit_off = at;
        d.nedits = nedits[k];
        d.phase = kPhaseApply;
        d.nsol = md ? srcs[(size_t)k].n : nsol;  // md: z and old_z come from the device
        d.status = kRunning;
        d.R = md ? srcs[(size_t)k].rows : R;
        d.C = md ? srcs[(size_t)k].cols : C;
        at += nedits[k];
    }
    const int64_t n = count, RC = (int64_t)maxR * maxC;
    const int m = maxR - 1;
    const int64_t te = std::max<int64_t>(total, 1);
    int rc = LPR_OK_OPTIMAL;
    auto get = [&](auto** p, int64_t elems, const char* what) {
        dev_alloc(p, elems, what, &rc, sb_oom);
    };
    get(&v.desc, n, "descriptors");
    get(&v.cur, n * RC, "tableau slab");
    get(&v.alt, n * RC, "second tableau slab");
    get(&v.basic, n * std::max(m, 1), "basicVars");
    get(&v.bcount, n * maxC, "membership counts");
    get(&v.snap, n * (m + maxC), "ChangeRHS snapshots");
    get(&v.sol, n * v.sol_cap, "solution vectors");
    get(&v.log, n * 3 * v.log_cap, "pivot logs");
    get(&v.outcome, te, "outcomes");
    get(&v.edit_piv, te, "pivot counts");
    get(&b->d_edits, te, "edits");
    if (npayload > 0) get(&b->d_payload, npayload, "payload");
    b->run.alloc(count, &rc, sb_oom);
    if (rc != LPR_OK_OPTIMAL) return sb_fail(b, rc);
    v.edits = b->d_edits;
    v.payload = b->d_payload;
    hipStream_t s = e->stream;
    double* d_sol = nullptr;  // the base's solutionVector is a host mirror
    SensModelSrc* d_src = nullptr;  // md: the LP of every scenario
    hipEvent_t ev[2] = {nullptr, nullptr};  // md: around the constructor kernel
    auto drop = [&]() {
        hipFree(d_sol);
        hipFree(d_src);
        for (hipEvent_t& x : ev)
            if (x) hipEventDestroy(x);
    };
    hipError_t err = hipSuccess;
    if (md) {
        if (hipMalloc(&d_src, (size_t)count * sizeof(SensModelSrc)) != hipSuccess) {
            (void)hipGetLastError();
            return sb_fail(b, sb_oom("item list", count));
        }
        err = hipMemcpyAsync(d_src, srcs.data(), (size_t)count * sizeof(SensModelSrc),
                             hipMemcpyHostToDevice, s);
        for (hipEvent_t& x : ev)
            if (err == hipSuccess) err = hipEventCreate(&x);
    } else if (nsol > 0) {
        if (hipMalloc(&d_sol, (size_t)nsol * sizeof(double)) != hipSuccess)
            return sb_fail(b, sb_oom("base solution", nsol));
        err = hipMemcpyAsync(d_sol, base_sol->data(), (size_t)nsol * sizeof(double),
                             hipMemcpyHostToDevice, s);
    }
    if (err == hipSuccess)
        err = hipMemcpyAsync(v.desc, b->h_desc.data(), (size_t)count * sizeof(SensScenario),
                             hipMemcpyHostToDevice, s);
    if (err == hipSuccess && total > 0)
        err = hipMemcpyAsync(b->d_edits, edits, (size_t)total * sizeof(lpr_sens_edit),
                             hipMemcpyHostToDevice, s);
    if (err == hipSuccess && npayload > 0)
        err = hipMemcpyAsync(b->d_payload, payload, (size_t)npayload * sizeof(double),
                             hipMemcpyHostToDevice, s);
    std::vector<int32_t> not_run;  // every outcome starts as kSensEditNotRun
    try {
        not_run.assign((size_t)te, kSensEditNotRun);
    } catch (...) {
        drop();
        return sb_fail(b, sb_oom("outcomes (host)", te));
    }
    if (err == hipSuccess)
        err = hipMemcpyAsync(v.outcome, not_run.data(), (size_t)te * sizeof(int32_t),
                             hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipMemsetAsync(v.edit_piv, 0, (size_t)te * sizeof(int64_t), s);
    if (err == hipSuccess) err = hipMemsetAsync(v.sol, 0, (size_t)(n * v.sol_cap) * sizeof(double), s);
    rc = LPR_OK_OPTIMAL;
    if (err == hipSuccess && md) {
        // :22-39 per scenario on the device; the descriptors come back with z and old_z
        err = hipEventRecord(ev[0], s);
        if (err == hipSuccess) rc = sens_batch_launch_from_models(s, v, count, d_src, md->slab);
        if (err == hipSuccess && rc == LPR_OK_OPTIMAL) err = hipEventRecord(ev[1], s);
        if (err == hipSuccess && rc == LPR_OK_OPTIMAL)
            err = hipMemcpyAsync(b->h_desc.data(), v.desc, (size_t)count * sizeof(SensScenario),
                                 hipMemcpyDeviceToHost, s);
    } else if (err == hipSuccess) {
        rc = sens_batch_launch_init(s, v, count, R, C, baseT, ld, base_basic, base_bcount, d_sol,
                                    nsol);
    }
    if (err == hipSuccess && rc == LPR_OK_OPTIMAL)
        err = hipStreamSynchronize(s);  // edits are borrowed, and the base may go after this call
    if (err == hipSuccess && rc == LPR_OK_OPTIMAL && md) {
        float ms = 0.f;
        err = hipEventElapsedTime(&ms, ev[0], ev[1]);
        b->ctor_ms = ms;
    }
    drop();
    if (err != hipSuccess) {
        set_error("%s: %s", W, hipGetErrorString(err));
        rc = LPR_DEVICE_ERROR;
    }
    if (rc != LPR_OK_OPTIMAL) return sb_fail(b, rc);
    e->live_sens_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

}  // namespace

namespace lpr {
void sens_batch_orphan(lpr_sens_batch* b) {  // lpr_engine_close
    sb_release_device(b);
    b->eng = nullptr;
}
}  // namespace lpr

extern "C" {

int lpr_sens_batch_create(lpr_sens* base, int32_t count, const int32_t* nedits,
                          const lpr_sens_edit* edits, int32_t log_cap, lpr_sens_batch** out) {
    return sb_create("lpr_sens_batch_create", false, base, nullptr, count, nedits, edits, nullptr,
                     0, log_cap, out);
}

// ... whose scripts may also hold AddNewActivity (:534-584) and AddNewConstraint (:609-659)
int lpr_sens_batch_create_grow(lpr_sens* base, int32_t count, const int32_t* nedits,
                               const lpr_sens_edit* edits, const double* payload,
                               int64_t npayload, int32_t log_cap, lpr_sens_batch** out) {
    return sb_create("lpr_sens_batch_create_grow", true, base, nullptr, count, nedits, edits,
                     payload, npayload, log_cap, out);
}

// new SensitivityAnalyzer(GetFinalTableau(), SolutionVector, FinalZ, BasicVariables)
// (Program.cs:147-151, SensitivityAnalyzer.cs:22-39) per scenario, on LP item[k] of a solved LP
// batch, device to device; the scripts are those of a grow batch
int lpr_sens_batch_from_batch(lpr_batch* lps, int32_t count, const int32_t* item,
                              const int32_t* nedits, const lpr_sens_edit* edits,
                              const double* payload, int64_t npayload, int32_t log_cap,
                              lpr_sens_batch** out) {
    static const char* W = "lpr_sens_batch_from_batch";
    if (out) *out = nullptr;
    SbModels md;
    md.bd = nullptr;
    md.slab = nullptr;
    md.item = item;
    md.eng = batch_view(lps, &md.bd, &md.slab);
    if (!md.eng) {
        set_error("%s: the LP batch is null or orphaned: its engine has been closed", W);
        return LPR_BAD_ARGUMENT;
    }
    return sb_create(W, true, nullptr, &md, count, nedits, edits, payload, npayload, log_cap, out);
}

int lpr_sens_batch_from_batch_time(lpr_sens_batch* b, double* kernel_ms) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    if (b->ctor_ms < 0.0) {
        set_error("lpr_sens_batch_from_batch_time: the batch was not made by "
                  "lpr_sens_batch_from_batch");
        return LPR_BAD_ARGUMENT;
    }
    if (kernel_ms) *kernel_ms = b->ctor_ms;
    return LPR_OK_OPTIMAL;
}

int lpr_sens_batch_destroy(lpr_sens_batch* b) {
    if (!b) return LPR_BAD_ARGUMENT;
    if (b->eng) {
        hipSetDevice(b->eng->device);
        hipStreamSynchronize(b->eng->stream);
        sb_release_device(b);
        unlist(b->eng->live_sens_batch, b);
    }
    delete b;
    return LPR_OK_OPTIMAL;
}

// Every script that has not ended, edit after edit (:203-208, :300-321, :362-393, :427-470,
// :502-531, and in a grow batch :534-584, :609-659)
int lpr_sens_batch_run(lpr_sens_batch* b, const lpr_sens_batch_opts* opts,
                       lpr_sens_batch_result* res) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    if (!res) {
        set_error("lpr_sens_batch_run: null result");
        return LPR_BAD_ARGUMENT;
    }
    lpr_sens_batch_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if ((o.variant != 0 && o.variant != 2 && o.variant != 3) || o.chunk < 0) {
        set_error("lpr_sens_batch_run: variant %d (0 auto, 2 G, 3 H) / chunk %d (>= 0)", o.variant,
                  o.chunk);
        return LPR_BAD_ARGUMENT;
    }
    std::memset(res, 0, sizeof *res);
    hipStream_t s = b->eng->stream;
    const int32_t count = b->count;
    const SensBatchView& v = b->vw;
    std::vector<int32_t> lists[kNumForms];  // one form per call: one list is filled
    std::vector<int32_t> list;
    int64_t before = 0;
    bool inside = false;  // a scenario is stopped inside an edit: its slices belong to one form
    for (int32_t k = 0; k < count; ++k) {
        SensScenario& d = b->h_desc[(size_t)k];
        before += d.pivots;
        if (d.status != kRunning && d.status != LPR_PIVOT_LIMIT) continue;  // finished stays so
        inside = inside || d.phase != kPhaseApply;
        d.status = kRunning;
        d.pivot_stop = o.max_pivots > 0 ? d.pivots + o.max_pivots : 0;
        list.push_back(k);
    }
    int form = batch_pick_form(sens_batch_footprint_g(v.R, v.C), o.variant, false);
    if (inside && b->form != 0) form = b->form;
    b->form = form;
    res->form = form;
    lists[form].swap(list);
    int rc = b->run.upload(s, lists);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(v.desc, b->h_desc.data(), (size_t)count * sizeof(SensScenario),
                           hipMemcpyHostToDevice, s));
    const int chunk = o.chunk > 0 ? o.chunk : kSensBatchChunk[form];
    int launches = 0;
    rc = b->run.rounds(s, [&](int f, const int32_t* in, int n_in, int32_t* out, int32_t* n_out) {
        return sens_batch_launch(f, b->grow, s, v, in, n_in, out, n_out, chunk);
    }, &launches);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->h_desc.data(), v.desc, (size_t)count * sizeof(SensScenario),
                           hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    int64_t after = 0;
    for (const SensScenario& d : b->h_desc) {
        after += d.pivots;
        res->finished += d.status == LPR_OK_OPTIMAL;
        res->running += d.status == LPR_PIVOT_LIMIT;
    }
    res->launches = launches;
    res->pivots = after - before;
    return LPR_OK_OPTIMAL;
}

int lpr_sens_batch_info(lpr_sens_batch* b, int32_t* count, int32_t* rows, int32_t* cols,
                        int64_t* total_edits, int32_t* log_cap, int32_t* form) {
    if (!b) {
        set_error("lpr_sens_batch_info: null handle");
        return LPR_BAD_ARGUMENT;
    }
    if (count) *count = b->count;
    if (rows) *rows = b->base_R;
    if (cols) *cols = b->base_C;
    if (total_edits) *total_edits = b->total_edits;
    if (log_cap) *log_cap = b->vw.log_cap;
    if (form) *form = b->form;
    return LPR_OK_OPTIMAL;
}

// The outcome of every edit and its pivots, packed as the scripts are
int lpr_sens_batch_outcomes_read(lpr_sens_batch* b, int32_t* outcome, int64_t* pivots) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    if (b->total_edits == 0) return LPR_OK_OPTIMAL;
    hipStream_t s = b->eng->stream;
    if (outcome)
        LPR_HIP(hipMemcpyAsync(outcome, b->vw.outcome, (size_t)b->total_edits * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
    if (pivots)
        LPR_HIP(hipMemcpyAsync(pivots, b->vw.edit_piv, (size_t)b->total_edits * sizeof(int64_t),
                               hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    return LPR_OK_OPTIMAL;
}

// CurrentZ :728, solutionVector.Count and basicVars of every scenario
int lpr_sens_batch_state_read(lpr_sens_batch* b, double* z, int32_t* nsol, int32_t* basic) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    for (int32_t k = 0; k < b->count; ++k) {
        if (z) z[k] = b->h_desc[(size_t)k].z;
        if (nsol) nsol[k] = b->h_desc[(size_t)k].nsol;
    }
    const int64_t sm = b->vw.R - 1, nb = (int64_t)b->count * sm;
    if (basic && nb > 0) {
        LPR_HIP(hipMemcpyAsync(basic, b->vw.basic, (size_t)nb * sizeof(int32_t),
                               hipMemcpyDeviceToHost, b->eng->stream));
        LPR_HIP(hipStreamSynchronize(b->eng->stream));
        for (int32_t k = 0; k < b->count; ++k)  // past a scenario's own rows: no entry
            for (int64_t i = b->h_desc[(size_t)k].R - 1; i < sm; ++i) basic[k * sm + i] = INT32_MIN;
    }
    return LPR_OK_OPTIMAL;
}

// The shape of every scenario as of now, and the batch-wide maxima the strides are sized by
int lpr_sens_batch_shape_read(lpr_sens_batch* b, int32_t* rows, int32_t* cols, int32_t* max_rows,
                              int32_t* max_cols) {
    if (!b) {
        set_error("lpr_sens_batch_shape_read: null handle");
        return LPR_BAD_ARGUMENT;
    }
    for (int32_t k = 0; k < b->count; ++k) {
        if (rows) rows[k] = b->h_desc[(size_t)k].R;
        if (cols) cols[k] = b->h_desc[(size_t)k].C;
    }
    if (max_rows) *max_rows = b->vw.R;
    if (max_cols) *max_cols = b->vw.C;
    return LPR_OK_OPTIMAL;
}

// CurrentSolutionVector :729 of scenario k
int lpr_sens_batch_solution_read(lpr_sens_batch* b, int32_t k, double* x, int32_t cap,
                                 int32_t* count) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    if (k < 0 || k >= b->count || cap < 0 || !count) {
        set_error("lpr_sens_batch_solution_read: scenario %d out of range (0..%d), cap %d or null "
                  "count", k, b->count - 1, cap);
        return LPR_BAD_ARGUMENT;
    }
    const int32_t ns = b->h_desc[(size_t)k].nsol;
    *count = ns;
    const int32_t n = std::min(ns, cap);
    if (n == 0 || !x) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(x, b->vw.sol + (size_t)k * b->vw.sol_cap, (size_t)n * sizeof(double),
                           hipMemcpyDeviceToHost, b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// CurrentTableau :727 of scenario k
int lpr_sens_batch_tableau_read(lpr_sens_batch* b, int32_t k, double* rowmajor) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    if (k < 0 || k >= b->count || !rowmajor) {
        set_error("lpr_sens_batch_tableau_read: scenario %d out of range (0..%d) or null output",
                  k, b->count - 1);
        return LPR_BAD_ARGUMENT;
    }
    const SensScenario& d = b->h_desc[(size_t)k];
    const size_t RC = (size_t)d.R * d.C;  // compact at the scenario's own shape
    const double* src = (d.in_alt ? b->vw.alt : b->vw.cur) + (size_t)k * b->vw.R * b->vw.C;
    LPR_HIP(hipMemcpyAsync(rowmajor, src, RC * sizeof(double), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// The pivot log of scenario k, as lpr_sens_log_read
int lpr_sens_batch_log_read(lpr_sens_batch* b, int32_t k, int32_t* triples, int64_t cap,
                            int64_t* count) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    if (k < 0 || k >= b->count || cap < 0 || !count) {
        set_error("lpr_sens_batch_log_read: scenario %d out of range (0..%d), cap %lld or null "
                  "count", k, b->count - 1, (long long)cap);
        return LPR_BAD_ARGUMENT;
    }
    const int64_t total = b->h_desc[(size_t)k].log_n;
    *count = total;
    const int64_t n = std::min(std::min<int64_t>(total, b->vw.log_cap), cap);
    if (n == 0 || !triples) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpyAsync(triples, b->vw.log + (size_t)k * 3 * b->vw.log_cap,
                           (size_t)n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost,
                           b->eng->stream));
    LPR_HIP(hipStreamSynchronize(b->eng->stream));
    return LPR_OK_OPTIMAL;
}

// DisplayRangeNonBasic :276-297, DisplayRangeBasic :324-359, DisplayRangeRHS :396-424,
// ShadowPrices :212-222, GetBasicRow :69-84 of every scenario on the state the batch holds now
int lpr_sens_batch_ranging(lpr_sens_batch* b, int32_t* kind, int32_t* var_row,
                           double* reduced_cost, double* cost_lo, double* cost_hi, double* shadow,
                           double* rhs_lo, double* rhs_hi, double* rhs_now) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    SensBatchRangingPlan pl;
    if (b->min_R < 2 ||
        !sens_batch_ranging_plan(b->count, b->base_R, b->base_C, b->vw.R, b->vw.C, &pl)) {
        set_error("lpr_sens_batch_ranging: a %d x %d base has no slack block (n < 0), or a base "
                  "has no constraint row (least rows %d)", b->base_R, b->base_C, b->min_R);
        return LPR_BAD_ARGUMENT;
    }
    hipStream_t s = b->eng->stream;
    if (!b->rng_out && hipMalloc(&b->rng_out, pl.total) != hipSuccess) {
        b->rng_out = nullptr;
        (void)hipGetLastError();
        set_error("lpr_sens_batch_ranging: output block allocation (%zu bytes) failed", pl.total);
        return LPR_OUT_OF_MEMORY;
    }
    if (!b->rng_pin && hipHostMalloc(&b->rng_pin, pl.total) != hipSuccess) {
        b->rng_pin = nullptr;
        (void)hipGetLastError();
        set_error("lpr_sens_batch_ranging: pinned buffer allocation (%zu bytes) failed", pl.total);
        return LPR_OUT_OF_MEMORY;
    }
    for (hipEvent_t& ev : b->rng_ev)
        if (!ev) LPR_HIP(hipEventCreate(&ev));
    b->rng_timed = false;
    // the kernel takes shapes and in_alt from the device descriptors, which are current after
    // create and after every run (a run uploads h_desc before its first launch)
    LPR_HIP(hipEventRecord(b->rng_ev[0], s));
    const int rc = sens_batch_ranging_launch(s, b->vw, b->rng_out, pl);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipEventRecord(b->rng_ev[1], s));
    // one copy of the whole output block, then plain host copies to whatever the caller asked for
    LPR_HIP(hipMemcpyAsync(b->rng_pin, b->rng_out, pl.total, hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    b->rng_timed = true;
    sens_report_copy(pl.out, b->rng_pin, kind, var_row, reduced_cost, cost_lo, cost_hi, shadow,
                     rhs_lo, rhs_hi, rhs_now);
    return LPR_OK_OPTIMAL;
}

int lpr_sens_batch_ranging_time(lpr_sens_batch* b, double* kernel_ms) {
    LPR_LIVE_HANDLE(b, "scenario batch");
    if (!b->rng_timed) {
        set_error("lpr_sens_batch_ranging_time: no lpr_sens_batch_ranging call has completed on "
                  "this handle");
        return LPR_BAD_ARGUMENT;
    }
    float ms = 0.f;
    LPR_HIP(hipEventElapsedTime(&ms, b->rng_ev[0], b->rng_ev[1]));
    if (kernel_ms) *kernel_ms = ms;
    return LPR_OK_OPTIMAL;
}

}  // extern "C"
