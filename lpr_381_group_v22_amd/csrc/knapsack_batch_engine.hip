// knapsack_batch_engine.hip -- host side of the knapsack batch (include/lpr_engine.h,
// lpr_knap_batch_*).  Every instance runs the whole level-synchronous search
// of section 11 on the device; the host validates and ranks the items once (the single engine's
// rules, knapsack_common.hpp), relaunches the bounded kernel while instances are still running
// (BatchRunLists of batch_common.hpp, forms mixed per call) and rebuilds the selected items from
// the incumbents' bitmaps at the end.
#include "knapsack_batch_common.hpp"

#include <algorithm>
#include <new>

using namespace lpr;

struct lpr_knap_batch {
    lpr_engine* eng = nullptr;
    int32_t count = 0;
    int64_t bit_words = 0;  // incumbent bitmaps of all instances
    std::vector<KnapBatchDesc> h_desc;  // host mirror, current after create and every solve
    std::vector<int32_t> rank;          // packed by n: rank position -> original index
    std::vector<int32_t> selected;      // packed by n; sel_count entries per instance are valid
    std::vector<int32_t> sel_count;
    KnapBatchBufs B{};
    uint32_t *rw = nullptr, *rv = nullptr, *ow = nullptr, *ov = nullptr;
    BatchRunLists run;
    bool solved = false;
};

namespace {

int kb_oom(const char* what, int64_t n) {
    set_error("lpr_knap_batch: cannot allocate %s (%lld elements)", what, (long long)n);
    return LPR_OUT_OF_MEMORY;
}

void kb_release_device(lpr_knap_batch* b) {
    hipFree(b->B.desc);
    hipFree(b->B.slab);
    hipFree(b->B.inc_bits);
    hipFree(b->B.log.par);
    hipFree(b->B.log.br);
    hipFree(b->B.log.st);
    hipFree(b->B.log.kp);
    hipFree(b->B.log.bd);
    hipFree(b->B.log.V);
    hipFree(b->rw);
    hipFree(b->rv);
    hipFree(b->ow);
    hipFree(b->ov);
    b->run.release();
    b->B = KnapBatchBufs{};
    b->rw = b->rv = b->ow = b->ov = nullptr;
}

int kb_fail(lpr_knap_batch* b, int rc) {
    kb_release_device(b);
    delete b;
    return rc;
}

bool kb_item_ok(const char* where, const lpr_knap_batch* b, int32_t k) {
    if (k >= 0 && k < b->count) return true;
    set_error("%s: instance %d out of range (0..%d)", where, k, b->count - 1);
    return false;
}

template <class T>
int kb_upload(T* dst, const std::vector<T>& src) {
    if (src.empty()) return LPR_OK_OPTIMAL;
    LPR_HIP(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return LPR_OK_OPTIMAL;
}

size_t round8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace

namespace lpr {
void knap_batch_orphan(lpr_knap_batch* b) {  // lpr_engine_close
    kb_release_device(b);
    b->eng = nullptr;
}
}  // namespace lpr

extern "C" {

int lpr_knap_batch_create(lpr_engine* e, int32_t count, const int64_t* capacity, const int32_t* n,
                          const double* weights, const double* values, const int64_t* node_cap,
                          int32_t narrate, lpr_knap_batch** out) {
    static const char* W = "lpr_knap_batch_create";
    if (!e || !out || count < 1 || !capacity || !n || !weights || !values || narrate < 0) {
        set_error("%s: bad arguments (count=%d, narrate=%d, or a null engine / handle / capacity "
                  "/ n / weights / values)", W, count, narrate);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    char where[96];
    int64_t items = 0;
    for (int32_t k = 0; k < count; ++k) {
        std::snprintf(where, sizeof where, "%s: instance %d", W, k);
        if (n[k] < 1 || n[k] > kKnapMaxItems) {
            set_error("%s: n = %d is outside 1..%d", where, n[k], kKnapMaxItems);
            return LPR_BAD_ARGUMENT;
        }
        if (capacity[k] < 0) {
            set_error("%s: capacity %lld < 0", where, (long long)capacity[k]);
            return LPR_BAD_ARGUMENT;
        }
        if (node_cap && node_cap[k] > kKnapBatchMaxCap) {
            set_error("%s: node_cap %lld is over 2^22 (%lld); solve it alone with "
                      "lpr_knap_bb_solve", where, (long long)node_cap[k],
                      (long long)kKnapBatchMaxCap);
            return LPR_BAD_ARGUMENT;
        }
        if (!knap_items_ok(where, weights + items, values + items, n[k])) return LPR_BAD_ARGUMENT;
        items += n[k];
    }
    LPR_HIP(hipSetDevice(e->device));
    lpr_knap_batch* b = new (std::nothrow) lpr_knap_batch();
    if (!b) return kb_oom("handle", 1);
    b->eng = e;
    b->count = count;
    std::vector<uint32_t> h_rw, h_rv, h_ow, h_ov;
    int64_t slab = 0, words = 0, recs = 0;
    try {
        b->h_desc.resize((size_t)count);
        b->rank.resize((size_t)items);
        b->selected.assign((size_t)items, 0);
        b->sel_count.assign((size_t)count, 0);
        h_rw.resize((size_t)items);
        h_rv.resize((size_t)items);
        h_ow.resize((size_t)items);
        h_ov.resize((size_t)items);
        std::vector<uint64_t> iw((size_t)kKnapMaxItems), iv((size_t)kKnapMaxItems);
        int64_t at = 0;
        for (int32_t k = 0; k < count; ++k) {
            KnapBatchDesc& d = b->h_desc[(size_t)k];
            std::memset(&d, 0, sizeof d);
            d.n = n[k];
            d.nw = knap_words(n[k]);
            d.C = capacity[k];
            d.cap = node_cap && node_cap[k] > 0 ? node_cap[k] : kKnapBatchDefaultCap;
            d.narrate = (int32_t)std::min<int64_t>(narrate, d.cap);
            d.item_off = at;
            d.s_off = slab;
            d.bits_off = words;
            d.log_off = recs;
            d.status = LPR_OK_OPTIMAL;  // not solved yet
            int32_t* rank = b->rank.data() + at;
            knap_rank_items(weights + at, values + at, d.n, iw.data(), iv.data(), rank);
            for (int p = 0; p < d.n; ++p) {
                h_ow[(size_t)(at + p)] = (uint32_t)iw[(size_t)p];
                h_ov[(size_t)(at + p)] = (uint32_t)iv[(size_t)p];
                h_rw[(size_t)(at + p)] = (uint32_t)iw[(size_t)rank[p]];
                h_rv[(size_t)(at + p)] = (uint32_t)iv[(size_t)rank[p]];
            }
            at += d.n;
            slab += (int64_t)((size_t)d.cap * knap_batch_node_bytes(d.n));  // a multiple of 8
            words += 2 * d.nw;
            recs += d.narrate;
        }
    } catch (...) {
        delete b;
        return kb_oom("host arrays", items);
    }
    b->bit_words = words;
    int rc = LPR_OK_OPTIMAL;
    dev_alloc(&b->B.desc, count, "descriptors", &rc, kb_oom);
    dev_alloc(&b->B.slab, slab,
              "node storage: node_cap x (32 x ceil(n / 64) + 32) bytes per instance", &rc, kb_oom);
    dev_alloc(&b->B.inc_bits, words, "incumbent bitmaps", &rc, kb_oom);
    const int64_t lr = std::max<int64_t>(recs, 1);
    dev_alloc(&b->B.log.par, lr, "node records", &rc, kb_oom);
    dev_alloc(&b->B.log.br, lr, "node records", &rc, kb_oom);
    dev_alloc(&b->B.log.st, lr, "node records", &rc, kb_oom);
    dev_alloc(&b->B.log.kp, lr, "node records", &rc, kb_oom);
    dev_alloc(&b->B.log.bd, lr, "node records", &rc, kb_oom);
    dev_alloc(&b->B.log.V, lr, "node records", &rc, kb_oom);
    dev_alloc(&b->rw, items, "items", &rc, kb_oom);
    dev_alloc(&b->rv, items, "items", &rc, kb_oom);
    dev_alloc(&b->ow, items, "items", &rc, kb_oom);
    dev_alloc(&b->ov, items, "items", &rc, kb_oom);
    b->run.alloc(count, &rc, kb_oom);
    if (rc != LPR_OK_OPTIMAL) return kb_fail(b, rc);
    b->B.rw = b->rw;
    b->B.rv = b->rv;
    b->B.ow = b->ow;
    b->B.ov = b->ov;
    rc = kb_upload(b->rw, h_rw);
    if (rc == LPR_OK_OPTIMAL) rc = kb_upload(b->rv, h_rv);
    if (rc == LPR_OK_OPTIMAL) rc = kb_upload(b->ow, h_ow);
    if (rc == LPR_OK_OPTIMAL) rc = kb_upload(b->ov, h_ov);
    if (rc == LPR_OK_OPTIMAL) rc = kb_upload(b->B.desc, b->h_desc);
    if (rc != LPR_OK_OPTIMAL) return kb_fail(b, rc);
    e->live_knap_batch.push_back(b);
    *out = b;
    return LPR_OK_OPTIMAL;
}

int lpr_knap_batch_destroy(lpr_knap_batch* b) {
    if (!b) return LPR_BAD_ARGUMENT;
    if (b->eng) {
        hipSetDevice(b->eng->device);
        hipStreamSynchronize(b->eng->stream);
        kb_release_device(b);
        unlist(b->eng->live_knap_batch, b);
    }
    delete b;
    return LPR_OK_OPTIMAL;
}

int lpr_knap_batch_solve(lpr_knap_batch* b, const lpr_knap_batch_opts* opts,
                         lpr_knap_batch_result* res) {
    static const char* W = "lpr_knap_batch_solve";
    LPR_LIVE_HANDLE(b, "knapsack batch");
    if (!res) {
        set_error("%s: null result", W);
        return LPR_BAD_ARGUMENT;
    }
    lpr_knap_batch_opts o;
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
    b->solved = false;
    std::vector<int32_t> lists[kNumForms];
    size_t slot[kNumForms] = {0, 0, 0};
    for (int32_t k = 0; k < count; ++k) {  // every call starts from the roots
        KnapBatchDesc& d = b->h_desc[(size_t)k];
        d.evaluated = 0;
        d.width = 1;
        d.widest = 0;
        d.inc_z = 0;
        d.inc_gid = -1;
        d.levels = 0;
        d.cur = 0;
        d.status = kRunning;
        d.inc_found = 0;
        d.inc_stop = d.n;
        const size_t fp = knap_batch_footprint(d.n, d.cap);
        const int form = batch_pick_form(fp, o.variant);
        slot[form] = std::max(slot[form],
                              round8(form == kFormH ? knap_batch_items_bytes(d.n) : fp));
        lists[form].push_back(k);
    }
    int rc = b->run.upload(s, lists);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(b->B.desc, b->h_desc.data(), (size_t)count * sizeof(KnapBatchDesc),
                           hipMemcpyHostToDevice, s));
    LPR_HIP(hipMemsetAsync(b->B.inc_bits, 0, (size_t)b->bit_words * sizeof(uint64_t), s));
    int launches = 0;
    rc = b->run.rounds(s, [&](int f, const int32_t* in, int n_in, int32_t* out, int32_t* n_out) {
        return knap_batch_launch(f, s, b->B, slot[f], in, n_in, out, n_out,
                                 o.chunk > 0 ? o.chunk : kKnapBatchChunk[f]);
    }, &launches);
    if (rc != LPR_OK_OPTIMAL) return rc;
    std::vector<uint64_t> bits((size_t)b->bit_words);
    LPR_HIP(hipMemcpyAsync(b->h_desc.data(), b->B.desc, (size_t)count * sizeof(KnapBatchDesc),
                           hipMemcpyDeviceToHost, s));
    LPR_HIP(hipMemcpyAsync(bits.data(), b->B.inc_bits, bits.size() * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    for (int32_t k = 0; k < count; ++k) {
        const KnapBatchDesc& d = b->h_desc[(size_t)k];
        if (d.status != LPR_OK_OPTIMAL && d.status != LPR_BB_NODE_CAP) {
            set_error("%s: instance %d ended with status %d", W, k, d.status);
            return LPR_DEVICE_ERROR;
        }
        // the incumbent's items: F1 plus the free items its greedy walk took
        const uint64_t* f1 = bits.data() + d.bits_off;
        const uint64_t* f0 = f1 + d.nw;
        const int32_t* rank = b->rank.data() + d.item_off;
        int32_t* sel = b->selected.data() + d.item_off;
        int32_t m = 0;
        if (d.inc_found)
            for (int p = 0; p < d.n; ++p) {
                const bool in1 = (f1[p / kWave] >> (p % kWave)) & 1ull;
                const bool in0 = (f0[p / kWave] >> (p % kWave)) & 1ull;
                if (in1 || (p < d.inc_stop && !in0)) sel[m++] = rank[p];
            }
        std::sort(sel, sel + m);
        b->sel_count[(size_t)k] = m;
        if (d.status == LPR_OK_OPTIMAL) res->finished += 1;
        else res->capped += 1;
        res->nodes += d.evaluated;
    }
    res->launches = launches;
    res->items_w = (int32_t)lists[kFormW].size();
    res->items_g = (int32_t)lists[kFormG].size();
    res->items_h = (int32_t)lists[kFormH].size();
    b->solved = true;
    return LPR_OK_OPTIMAL;
}

int lpr_knap_batch_result_read(lpr_knap_batch* b, int32_t* status, int32_t* found, double* z,
                               int64_t* evaluated, int64_t* widest, int32_t* levels) {
    LPR_LIVE_HANDLE(b, "knapsack batch");
    for (int32_t k = 0; k < b->count; ++k) {
        const KnapBatchDesc& d = b->h_desc[(size_t)k];
        if (status) status[k] = d.status;
        if (found) found[k] = d.inc_found;
        if (z) z[k] = d.inc_found ? (double)d.inc_z : 0.0;
        if (evaluated) evaluated[k] = d.evaluated;
        if (widest) widest[k] = d.widest;
        if (levels) levels[k] = d.levels;
    }
    return LPR_OK_OPTIMAL;
}

int lpr_knap_batch_rank_read(lpr_knap_batch* b, int32_t* rank) {
    LPR_LIVE_HANDLE(b, "knapsack batch");
    if (!rank) {
        set_error("lpr_knap_batch_rank_read: null output");
        return LPR_BAD_ARGUMENT;
    }
    std::copy(b->rank.begin(), b->rank.end(), rank);
    return LPR_OK_OPTIMAL;
}

int lpr_knap_batch_selected_read(lpr_knap_batch* b, int32_t* ids, int32_t* counts) {
    LPR_LIVE_HANDLE(b, "knapsack batch");
    if (!ids || !counts) {
        set_error("lpr_knap_batch_selected_read: null output");
        return LPR_BAD_ARGUMENT;
    }
    for (int32_t k = 0; k < b->count; ++k) {
        const KnapBatchDesc& d = b->h_desc[(size_t)k];
        const int32_t m = b->sel_count[(size_t)k];
        std::copy(b->selected.begin() + d.item_off, b->selected.begin() + d.item_off + m,
                  ids + d.item_off);
        std::fill(ids + d.item_off + m, ids + d.item_off + d.n, -1);
        counts[k] = m;
    }
    return LPR_OK_OPTIMAL;
}

int lpr_knap_batch_nodes_read(lpr_knap_batch* b, int32_t k, int32_t* parent, int32_t* branch,
                              int32_t* status, double* bound, int32_t* kitem, int64_t* value,
                              int64_t cap, int64_t* count) {
    static const char* W = "lpr_knap_batch_nodes_read";
    LPR_LIVE_HANDLE(b, "knapsack batch");
    if (!kb_item_ok(W, b, k)) return LPR_BAD_ARGUMENT;
    if (!count || cap < 0) {
        set_error("%s: null count or cap < 0", W);
        return LPR_BAD_ARGUMENT;
    }
    const KnapBatchDesc& d = b->h_desc[(size_t)k];
    const int64_t kept = b->solved ? std::min<int64_t>(d.evaluated, d.narrate) : 0;
    *count = kept;
    const int64_t m = std::min(cap, kept);
    if (m == 0) return LPR_OK_OPTIMAL;
    hipStream_t s = b->eng->stream;
    const KnapLog& L = b->B.log;
    const size_t m4 = (size_t)m * sizeof(int32_t), m8 = (size_t)m * sizeof(int64_t);
    if (parent) LPR_HIP(hipMemcpyAsync(parent, L.par + d.log_off, m4, hipMemcpyDeviceToHost, s));
    if (branch) LPR_HIP(hipMemcpyAsync(branch, L.br + d.log_off, m4, hipMemcpyDeviceToHost, s));
    if (status) LPR_HIP(hipMemcpyAsync(status, L.st + d.log_off, m4, hipMemcpyDeviceToHost, s));
    if (bound) LPR_HIP(hipMemcpyAsync(bound, L.bd + d.log_off, m8, hipMemcpyDeviceToHost, s));
    if (kitem) LPR_HIP(hipMemcpyAsync(kitem, L.kp + d.log_off, m4, hipMemcpyDeviceToHost, s));
    if (value) LPR_HIP(hipMemcpyAsync(value, L.V + d.log_off, m8, hipMemcpyDeviceToHost, s));
    LPR_HIP(hipStreamSynchronize(s));
    if (kitem) {  // rank positions -> original indices
        const int32_t* rank = b->rank.data() + d.item_off;
        for (int64_t r = 0; r < m; ++r)
            if (kitem[r] >= 0 && kitem[r] < d.n) kitem[r] = rank[kitem[r]];
    }
    return LPR_OK_OPTIMAL;
}

int lpr_knap_batch_dp(lpr_knap_batch* b, const uint8_t* which, int64_t* best) {
    static const char* W = "lpr_knap_batch_dp";
    LPR_LIVE_HANDLE(b, "knapsack batch");
    if (!best) {
        set_error("%s: null output", W);
        return LPR_BAD_ARGUMENT;
    }
    hipStream_t s = b->eng->stream;
    const int32_t count = b->count;
    std::vector<int32_t> lists[kNumForms];
    size_t slot[kNumForms] = {0, 0, 0};
    int64_t row_cells = 0;
    int h_launches = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (which && !which[k]) continue;
        KnapBatchDesc& d = b->h_desc[(size_t)k];
        const int64_t cells = d.C + 1;
        if (cells > kKnapBatchDpMaxCells) {
            set_error("%s: instance %d needs %lld cells (capacity + 1), over the batch limit of "
                      "%lld; solve it alone with lpr_knap_dp", W, k, (long long)cells,
                      (long long)kKnapBatchDpMaxCells);
            return LPR_BAD_ARGUMENT;
        }
        const size_t bytes = (size_t)cells * sizeof(int64_t);
        const int form = batch_pick_form(bytes, 0);
        slot[form] = std::max(slot[form], bytes);
        lists[form].push_back(k);
        d.dp_item = 0;
        d.dp_cur = 0;
        d.dp_row = 0;
        if (form == kFormH) {
            d.dp_row = row_cells;
            row_cells += 2 * cells;
            // the launches k_knap_batch_dp needs: whole items, kKnapBatchDpWork updates each
            const int64_t per = std::max<int64_t>(1, kKnapBatchDpWork / cells);
            h_launches = std::max(h_launches, (int)((d.n + per - 1) / per));
        }
    }
    int64_t* d_best = nullptr;
    int64_t* d_rows = nullptr;
    int32_t* d_idx = nullptr;
    int rc = LPR_OK_OPTIMAL;
    dev_alloc(&d_best, count, "DP results", &rc, kb_oom);
    dev_alloc(&d_idx, count, "DP lists", &rc, kb_oom);
    if (row_cells > 0) dev_alloc(&d_rows, row_cells, "DP rows: 2 x (capacity + 1) cells", &rc, kb_oom);
    std::vector<int64_t> h_best((size_t)count, -1);
    auto run = [&]() -> int {
        LPR_HIP(hipMemcpyAsync(b->B.desc, b->h_desc.data(), (size_t)count * sizeof(KnapBatchDesc),
                               hipMemcpyHostToDevice, s));
        LPR_HIP(hipMemcpyAsync(d_best, h_best.data(), (size_t)count * sizeof(int64_t),
                               hipMemcpyHostToDevice, s));
        int at = 0;
        for (int f = 0; f < kNumForms; ++f) {
            const int m = (int)lists[f].size();
            if (m == 0) continue;
            LPR_HIP(hipMemcpyAsync(d_idx + at, lists[f].data(), (size_t)m * sizeof(int32_t),
                                   hipMemcpyHostToDevice, s));
            for (int r = 0; r < (f == kFormH ? h_launches : 1); ++r) {
                const int lrc = knap_batch_launch_dp(f, s, b->B, slot[f], d_idx + at, m, d_rows,
                                                     d_best);
                if (lrc != LPR_OK_OPTIMAL) return lrc;
            }
            at += m;
        }
        LPR_HIP(hipMemcpyAsync(h_best.data(), d_best, (size_t)count * sizeof(int64_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipStreamSynchronize(s));
        return LPR_OK_OPTIMAL;
    };
    if (rc == LPR_OK_OPTIMAL) rc = run();
    hipStreamSynchronize(s);
    hipFree(d_best);
    hipFree(d_rows);
    hipFree(d_idx);
    if (rc != LPR_OK_OPTIMAL) return rc;
    std::copy(h_best.begin(), h_best.end(), best);
    return LPR_OK_OPTIMAL;
}

}  // extern "C"
