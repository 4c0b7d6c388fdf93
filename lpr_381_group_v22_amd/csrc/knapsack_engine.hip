// knapsack_engine.hip -- C ABI of menu option 5 (Program.cs:430-470): lpr_knap_dp
// (KnapsackBranchBoundSolver.Solve) and the lpr_knap_bb_* handle (KnapsackBranchBoundSimplex).
// The host ranks the items once, then only launches kernels and reads one KnapLevel per level;
// nothing on the host grows with the frontier.  Rules: DESIGN.md section 11.
#include "knapsack_common.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <new>

#pragma clang fp contract(off)

using namespace lpr;

struct lpr_knap {
    lpr_engine* eng = nullptr;
    int n = 0, nw = 0;  // items, 64-bit words per bitmap
    int64_t C = 0;
    std::vector<int32_t> rank;      // rank position -> original index
    std::vector<int64_t> hw, hv;    // weights / values in rank order
    int64_t *d_w = nullptr, *d_v = nullptr;
    // double-buffered frontier: 2 * nw words per node, parent record and branch bit per node
    uint64_t* nodes[2] = {nullptr, nullptr};
    int32_t* par[2] = {nullptr, nullptr};
    int32_t* br[2] = {nullptr, nullptr};
    int64_t fcap[2] = {0, 0};
    // evaluation records of the level being processed
    int32_t *st = nullptr, *kp = nullptr, *stop = nullptr, *pos = nullptr;
    int64_t* V = nullptr;
    double* bd = nullptr;
    int64_t rcap = 0;
    KnapInc* inc = nullptr;
    uint64_t* inc_bits = nullptr;
    KnapLevel* lvl = nullptr;
    KnapLevel* h_lvl = nullptr;  // pinned
    KnapLog log{};
    // results of the last solve
    bool solved = false;
    int32_t levels = 0;
    int64_t evaluated = 0, widest = 0;
    std::vector<int32_t> selected;
    std::vector<int32_t> r_par, r_br, r_st, r_kp;
    std::vector<double> r_bd;
    std::vector<int64_t> r_V;
};

namespace {

template <class T>
void knap_free(T*& p) {
    if (p) hipFree(p);
    p = nullptr;
}

void knap_free_log(lpr_knap* k) {
    knap_free(k->log.par);
    knap_free(k->log.br);
    knap_free(k->log.st);
    knap_free(k->log.kp);
    knap_free(k->log.bd);
    knap_free(k->log.V);
    k->log.cap = 0;
}

void knap_release_device(lpr_knap* k) {
    knap_free(k->d_w);
    knap_free(k->d_v);
    for (int b = 0; b < 2; ++b) {
        knap_free(k->nodes[b]);
        knap_free(k->par[b]);
        knap_free(k->br[b]);
        k->fcap[b] = 0;
    }
    knap_free(k->st);
    knap_free(k->kp);
    knap_free(k->stop);
    knap_free(k->pos);
    knap_free(k->V);
    knap_free(k->bd);
    k->rcap = 0;
    knap_free(k->inc);
    knap_free(k->inc_bits);
    knap_free(k->lvl);
    if (k->h_lvl) hipHostFree(k->h_lvl);
    k->h_lvl = nullptr;
    knap_free_log(k);
}

int knap_oom(const char* what, int64_t count) {
    set_error("knapsack: device allocation of %s (%lld entries) failed", what, (long long)count);
    return LPR_OUT_OF_MEMORY;
}

// frontier buffer b holds at least `need` nodes (its contents are not kept: it is about to be
// written by k_knap_children)
int knap_ensure_frontier(lpr_knap* k, int b, int64_t need) {
    if (need <= k->fcap[b]) return LPR_OK_OPTIMAL;
    const int64_t cap = std::max(need, 2 * k->fcap[b]);
    knap_free(k->nodes[b]);
    knap_free(k->par[b]);
    knap_free(k->br[b]);
    k->fcap[b] = 0;
    if (hipMalloc(&k->nodes[b], (size_t)cap * 2 * k->nw * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&k->par[b], (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->br[b], (size_t)cap * sizeof(int32_t)) != hipSuccess)
        return knap_oom("frontier", cap);
    k->fcap[b] = cap;
    return LPR_OK_OPTIMAL;
}

int knap_ensure_records(lpr_knap* k, int64_t need) {
    if (need <= k->rcap) return LPR_OK_OPTIMAL;
    const int64_t cap = std::max(need, 2 * k->rcap);
    knap_free(k->st);
    knap_free(k->kp);
    knap_free(k->stop);
    knap_free(k->pos);
    knap_free(k->V);
    knap_free(k->bd);
    k->rcap = 0;
    if (hipMalloc(&k->st, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->kp, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->stop, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->pos, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->V, (size_t)cap * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&k->bd, (size_t)cap * sizeof(double)) != hipSuccess)
        return knap_oom("level records", cap);
    k->rcap = cap;
    return LPR_OK_OPTIMAL;
}

int knap_ensure_log(lpr_knap* k, int64_t cap) {
    if (cap == k->log.cap) return LPR_OK_OPTIMAL;
    knap_free_log(k);
    if (cap == 0) return LPR_OK_OPTIMAL;
    if (hipMalloc(&k->log.par, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->log.br, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->log.st, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->log.kp, (size_t)cap * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&k->log.bd, (size_t)cap * sizeof(double)) != hipSuccess ||
        hipMalloc(&k->log.V, (size_t)cap * sizeof(int64_t)) != hipSuccess) {
        knap_free_log(k);
        return knap_oom("node log", cap);
    }
    k->log.cap = cap;
    return LPR_OK_OPTIMAL;
}

}  // namespace

namespace lpr {
void knap_orphan(lpr_knap* k) {  // lpr_engine_close
    knap_release_device(k);
    k->eng = nullptr;
}
}  // namespace lpr

#define LPR_LIVE_K(k)                                                                       \
    do {                                                                                    \
        if (!(k) || !(k)->eng) {                                                            \
            set_error("knapsack handle is null or its engine has been closed");             \
            return LPR_BAD_ARGUMENT;                                                        \
        }                                                                                   \
        LPR_HIP(hipSetDevice((k)->eng->device));                                            \
    } while (0)

extern "C" {

int lpr_knap_dp(lpr_engine* e, int64_t capacity, const int32_t* weights, const int32_t* values,
                int32_t n, const lpr_knap_dp_opts* opts, int64_t* best) {
    if (!e || !best || n < 0 || (n > 0 && (!weights || !values))) {
        set_error("lpr_knap_dp: null engine / output / item arrays or n < 0");
        return LPR_BAD_ARGUMENT;
    }
    if (capacity < 0) {
        set_error("lpr_knap_dp: capacity %lld < 0", (long long)capacity);
        return LPR_BAD_ARGUMENT;
    }
    for (int32_t i = 0; i < n; ++i)
        if (weights[i] < 0) {
            set_error("lpr_knap_dp: weights[%d] = %d < 0", i, weights[i]);
            return LPR_BAD_ARGUMENT;
        }
    if (capacity > (int64_t)1 << 36) {
        set_error("lpr_knap_dp: capacity %lld is over 2^36 cells", (long long)capacity);
        return LPR_BAD_ARGUMENT;
    }
    const int variant = opts ? opts->variant : 0;
    if (variant != 0 && variant != 1) {
        set_error("lpr_knap_dp: unknown variant %d", variant);
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipSetDevice(e->device));
    // items heavier than the capacity change nothing
    std::vector<int32_t> w, v;
    for (int32_t i = 0; i < n; ++i)
        if (weights[i] <= capacity) {
            w.push_back(weights[i]);
            v.push_back(values[i]);
        }
    const int64_t cells = capacity + 1;
    const int m = (int)w.size();
    hipStream_t s = e->stream;
    int64_t* row[2] = {nullptr, nullptr};
    int32_t *d_w = nullptr, *d_v = nullptr;
    int rc = LPR_OK_OPTIMAL;
    auto done = [&](int code) {
        hipStreamSynchronize(s);
        knap_free(row[0]);
        knap_free(row[1]);
        knap_free(d_w);
        knap_free(d_v);
        return code;
    };
    if (hipMalloc(&row[0], (size_t)cells * sizeof(int64_t)) != hipSuccess ||
        (m > 0 && hipMalloc(&row[1], (size_t)cells * sizeof(int64_t)) != hipSuccess) ||
        (m > 0 && hipMalloc(&d_w, (size_t)m * sizeof(int32_t)) != hipSuccess) ||
        (m > 0 && hipMalloc(&d_v, (size_t)m * sizeof(int32_t)) != hipSuccess)) {
        knap_oom("DP row", cells);
        return done(LPR_OUT_OF_MEMORY);
    }
    if (hipMemsetAsync(row[0], 0, (size_t)cells * sizeof(int64_t), s) != hipSuccess ||
        (m > 0 && (hipMemcpyAsync(d_w, w.data(), (size_t)m * sizeof(int32_t),
                                  hipMemcpyHostToDevice, s) != hipSuccess ||
                   hipMemcpyAsync(d_v, v.data(), (size_t)m * sizeof(int32_t),
                                  hipMemcpyHostToDevice, s) != hipSuccess))) {
        set_error("lpr_knap_dp: upload failed");
        return done(LPR_DEVICE_ERROR);
    }
    int cur = 0;
    int j0 = 0, S = 0;  // open block [j0, j) with weight sum S
    auto flush = [&](int j1) {
        if (j1 > j0) {
            knap_launch_dp_block(s, row[cur], row[cur ^ 1], cells, d_w, d_v, j0, j1, S);
            cur ^= 1;
        }
        j0 = j1;
        S = 0;
    };
    for (int j = 0; j < m; ++j) {
        if (variant == 1 || w[j] > kKnapHalo) {  // single-item streaming pass
            flush(j);
            knap_launch_dp_stream(s, row[cur], row[cur ^ 1], cells, w[j], v[j], e->num_cus);
            cur ^= 1;
            j0 = j + 1;
            continue;
        }
        if (S + w[j] > kKnapHalo) flush(j);
        S += w[j];
    }
    flush(m);
    if (hipGetLastError() != hipSuccess) {
        set_error("lpr_knap_dp: kernel launch failed");
        return done(LPR_DEVICE_ERROR);
    }
    int64_t out = 0;
    if (hipMemcpyAsync(&out, row[cur] + capacity, sizeof(int64_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("lpr_knap_dp: device error while running the DP");
        return done(LPR_DEVICE_ERROR);
    }
    *best = out;
    return done(rc);
}

int lpr_knap_bb_create(lpr_engine* e, int64_t capacity, const double* weights,
                       const double* values, int32_t n, lpr_knap** out) {
    if (!e || !out || (n > 0 && (!weights || !values))) {
        set_error("lpr_knap_bb_create: null engine / output / item arrays");
        return LPR_BAD_ARGUMENT;
    }
    if (n < 1 || n > kKnapMaxItems) {
        set_error("lpr_knap_bb_create: n = %d is outside 1..%d", n, kKnapMaxItems);
        return LPR_BAD_ARGUMENT;
    }
    if (capacity < 0) {
        set_error("lpr_knap_bb_create: capacity %lld < 0", (long long)capacity);
        return LPR_BAD_ARGUMENT;
    }
    if (!knap_items_ok("lpr_knap_bb_create", weights, values, n)) return LPR_BAD_ARGUMENT;
    LPR_HIP(hipSetDevice(e->device));
    lpr_knap* k = new (std::nothrow) lpr_knap();
    if (!k) return LPR_OUT_OF_MEMORY;
    k->eng = e;
    k->n = n;
    k->nw = (n + kWave - 1) / kWave;
    k->C = capacity;
    std::vector<uint64_t> ow(n), ov(n);
    k->rank.resize(n);
    knap_rank_items(weights, values, n, ow.data(), ov.data(), k->rank.data());
    k->hw.resize(n);
    k->hv.resize(n);
    for (int p = 0; p < n; ++p) {
        k->hw[p] = (int64_t)ow[k->rank[p]];
        k->hv[p] = (int64_t)ov[k->rank[p]];
    }
    int rc = LPR_OK_OPTIMAL;
    if (hipMalloc(&k->d_w, (size_t)n * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&k->d_v, (size_t)n * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&k->inc, sizeof(KnapInc)) != hipSuccess ||
        hipMalloc(&k->inc_bits, (size_t)2 * k->nw * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&k->lvl, sizeof(KnapLevel)) != hipSuccess ||
        hipHostMalloc(&k->h_lvl, sizeof(KnapLevel)) != hipSuccess) {
        rc = knap_oom("item arrays", n);
    } else if (hipMemcpy(k->d_w, k->hw.data(), (size_t)n * sizeof(int64_t),
                         hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(k->d_v, k->hv.data(), (size_t)n * sizeof(int64_t),
                         hipMemcpyHostToDevice) != hipSuccess) {
        set_error("lpr_knap_bb_create: upload failed");
        rc = LPR_DEVICE_ERROR;
    }
    if (rc != LPR_OK_OPTIMAL) {
        knap_release_device(k);
        delete k;
        return rc;
    }
    e->live_knap.push_back(k);
    *out = k;
    return LPR_OK_OPTIMAL;
}

int lpr_knap_bb_destroy(lpr_knap* k) {
    if (!k) return LPR_BAD_ARGUMENT;
    if (k->eng) {
        hipSetDevice(k->eng->device);
        hipStreamSynchronize(k->eng->stream);
        knap_release_device(k);
        auto& lv = k->eng->live_knap;
        for (size_t q = 0; q < lv.size(); ++q)
            if (lv[q] == k) {
                lv.erase(lv.begin() + q);
                break;
            }
    }
    delete k;
    return LPR_OK_OPTIMAL;
}

int lpr_knap_bb_solve(lpr_knap* k, const lpr_knap_bb_opts* opts, lpr_knap_bb_result* res) {
    LPR_LIVE_K(k);
    int64_t cap = opts && opts->node_cap > 0 ? opts->node_cap : (int64_t)1 << 22;
    if (cap > INT32_MAX) cap = INT32_MAX;  // record indices are int32
    const int32_t narrate = opts ? opts->narrate : -1;
    int64_t log_cap = narrate > 0 ? narrate : (narrate < 0 && k->n <= 64 ? 4096 : 0);
    if (log_cap > cap) log_cap = cap;
    k->solved = false;
    k->selected.clear();
    int rc = knap_ensure_log(k, log_cap);
    if (rc == LPR_OK_OPTIMAL) rc = knap_ensure_frontier(k, 0, 1);
    if (rc != LPR_OK_OPTIMAL) return rc;
    hipStream_t s = k->eng->stream;
    const int nw = k->nw;
    KnapInc inc0{0, 0, k->n, -1};
    const int32_t root_par = -1, root_br = 0;
    LPR_HIP(hipMemsetAsync(k->nodes[0], 0, (size_t)2 * nw * sizeof(uint64_t), s));
    LPR_HIP(hipMemcpyAsync(k->par[0], &root_par, sizeof(int32_t), hipMemcpyHostToDevice, s));
    LPR_HIP(hipMemcpyAsync(k->br[0], &root_br, sizeof(int32_t), hipMemcpyHostToDevice, s));
    LPR_HIP(hipMemcpyAsync(k->inc, &inc0, sizeof inc0, hipMemcpyHostToDevice, s));
    LPR_HIP(hipMemsetAsync(k->inc_bits, 0, (size_t)2 * nw * sizeof(uint64_t), s));
    LPR_HIP(hipStreamSynchronize(s));  // the sources above live on this stack frame
    int cur = 0;
    int64_t W = 1, evaluated = 0, widest = 0;
    int32_t levels = 0;
    int status = LPR_OK_OPTIMAL;
    while (W > 0) {
        if (evaluated + W > cap) {
            status = LPR_BB_NODE_CAP;
            break;
        }
        rc = knap_ensure_records(k, W);
        if (rc != LPR_OK_OPTIMAL) return rc;
        knap_launch_eval(s, k->nodes[cur], nw, k->n, k->C, k->d_w, k->d_v, W, k->st, k->kp,
                         k->stop, k->V, k->bd);
        knap_launch_level(s, W, evaluated, k->nodes[cur], nw, k->par[cur], k->br[cur], k->st,
                          k->kp, k->stop, k->V, k->bd, k->pos, k->inc, k->inc_bits, k->lvl, k->log);
        LPR_HIP(hipGetLastError());
        LPR_HIP(hipMemcpyAsync(k->h_lvl, k->lvl, sizeof(KnapLevel), hipMemcpyDeviceToHost, s));
        LPR_HIP(hipStreamSynchronize(s));
        evaluated += W;
        levels += 1;
        widest = std::max(widest, W);
        const int64_t next = k->h_lvl->next_width;
        if (next < 0 || next > 2 * W) {
            set_error("lpr_knap_bb_solve: level %d reported %lld children of %lld nodes", levels,
                      (long long)next, (long long)W);
            return LPR_DEVICE_ERROR;
        }
        if (next == 0) break;
        if (evaluated + next > cap) {  // the children would not be evaluated: do not make them
            status = LPR_BB_NODE_CAP;
            break;
        }
        rc = knap_ensure_frontier(k, cur ^ 1, next);
        if (rc != LPR_OK_OPTIMAL) return rc;
        knap_launch_children(s, W, evaluated - W, k->nodes[cur], nw, k->pos, k->kp,
                             k->nodes[cur ^ 1], k->par[cur ^ 1], k->br[cur ^ 1]);
        LPR_HIP(hipGetLastError());
        cur ^= 1;
        W = next;
    }
    // the incumbent's items: F1 plus the free items its greedy walk took
    KnapInc inc{};
    std::vector<uint64_t> bits((size_t)2 * nw);
    LPR_HIP(hipMemcpyAsync(&inc, k->inc, sizeof inc, hipMemcpyDeviceToHost, s));
    LPR_HIP(hipMemcpyAsync(bits.data(), k->inc_bits, bits.size() * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, s));
    const int64_t kept = std::min(evaluated, k->log.cap);
    k->r_par.resize(kept);
    k->r_br.resize(kept);
    k->r_st.resize(kept);
    k->r_kp.resize(kept);
    k->r_bd.resize(kept);
    k->r_V.resize(kept);
    if (kept > 0) {
        LPR_HIP(hipMemcpyAsync(k->r_par.data(), k->log.par, kept * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(k->r_br.data(), k->log.br, kept * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(k->r_st.data(), k->log.st, kept * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(k->r_kp.data(), k->log.kp, kept * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(k->r_bd.data(), k->log.bd, kept * sizeof(double),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(k->r_V.data(), k->log.V, kept * sizeof(int64_t),
                               hipMemcpyDeviceToHost, s));
    }
    LPR_HIP(hipStreamSynchronize(s));
    for (int64_t r = 0; r < kept; ++r)  // rank positions -> original indices
        if (k->r_kp[r] >= 0 && k->r_kp[r] < k->n) k->r_kp[r] = k->rank[k->r_kp[r]];
    if (inc.found) {
        for (int p = 0; p < k->n; ++p) {
            const bool f1 = (bits[p / kWave] >> (p % kWave)) & 1ull;
            const bool f0 = (bits[nw + p / kWave] >> (p % kWave)) & 1ull;
            if (f1 || (p < inc.stop && !f0)) k->selected.push_back(k->rank[p]);
        }
        std::sort(k->selected.begin(), k->selected.end());
    }
    k->levels = levels;
    k->evaluated = evaluated;
    k->widest = widest;
    k->solved = true;
    if (res) {
        res->status = status;
        res->found = inc.found;
        res->z = inc.found ? (double)inc.z : 0.0;
        res->evaluated = evaluated;
        res->widest = widest;
        res->levels = levels;
        res->reserved = 0;
    }
    return status;
}

int lpr_knap_bb_rank_read(lpr_knap* k, int32_t* rank) {
    if (!k || !rank) {
        set_error("lpr_knap_bb_rank_read: null handle / output");
        return LPR_BAD_ARGUMENT;
    }
    std::copy(k->rank.begin(), k->rank.end(), rank);
    return LPR_OK_OPTIMAL;
}

int lpr_knap_bb_selected_read(lpr_knap* k, int32_t* ids, int32_t* count) {
    if (!k || !count || (!ids && !k->selected.empty())) {
        set_error("lpr_knap_bb_selected_read: null handle / output");
        return LPR_BAD_ARGUMENT;
    }
    std::copy(k->selected.begin(), k->selected.end(), ids);
    *count = (int32_t)k->selected.size();
    return LPR_OK_OPTIMAL;
}

int lpr_knap_bb_stats(lpr_knap* k, int32_t* levels, int64_t* evaluated, int64_t* widest) {
    if (!k) {
        set_error("lpr_knap_bb_stats: null handle");
        return LPR_BAD_ARGUMENT;
    }
    if (levels) *levels = k->levels;
    if (evaluated) *evaluated = k->evaluated;
    if (widest) *widest = k->widest;
    return LPR_OK_OPTIMAL;
}

int lpr_knap_bb_nodes_read(lpr_knap* k, int32_t* parent, int32_t* branch, int32_t* status,
                           double* bound, int32_t* kitem, int64_t* value, int64_t cap,
                           int64_t* count) {
    if (!k || !count || cap < 0) {
        set_error("lpr_knap_bb_nodes_read: null handle / count or cap < 0");
        return LPR_BAD_ARGUMENT;
    }
    const int64_t m = std::min<int64_t>(cap, (int64_t)k->r_st.size());
    for (int64_t r = 0; r < m; ++r) {
        if (parent) parent[r] = k->r_par[r];
        if (branch) branch[r] = k->r_br[r];
        if (status) status[r] = k->r_st[r];
        if (bound) bound[r] = k->r_bd[r];
        if (kitem) kitem[r] = k->r_kp[r];
        if (value) value[r] = k->r_V[r];
    }
    *count = (int64_t)k->r_st.size();
    return LPR_OK_OPTIMAL;
}

}  // extern "C"
