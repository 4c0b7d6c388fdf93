// knapsack_batch_kernels.hip -- device side of the knapsack batch: the
// whole level-synchronous search of section 11 for many instances per launch, and the 0/1 DP of
// every instance.  The rules and the node evaluation are the single engine's (knapsack_common.hpp);
// all sums are int64 and the bound's three roundings go through knap_bound.
#include "knapsack_batch_common.hpp"

#include "batch_device.hpp"

#pragma clang fp contract(off)

namespace lpr {

namespace {

constexpr int kScratchWords = (int)(kBatchWgScratch / sizeof(uint64_t));

// One lane evaluates one node of an instance with n <= 64 (one word per bitmap): the greedy walk
// over the free items in rank order, on registers.  Same results as knap_eval_wave.
__device__ __forceinline__ KnapEval knap_eval_lane(uint64_t F1, uint64_t F0, int n, int64_t C,
                                                   const uint32_t* w, const uint32_t* v) {
    int64_t R = C, V = 0;
    for (uint64_t m = F1; m; m &= m - 1) {
        const int p = __builtin_ctzll(m);
        R -= (int64_t)w[p];
        V += (int64_t)v[p];
    }
    if (R < 0) return KnapEval{kKnapInfeasible, -1, n, 0, 0.0};
    uint64_t fr = ~(F1 | F0) & (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
    int k = -1;
    for (; fr; fr &= fr - 1) {
        const int p = __builtin_ctzll(fr);
        const int64_t wp = (int64_t)w[p];
        if (wp > R) {
            k = p;
            break;
        }
        R -= wp;
        V += (int64_t)v[p];
    }
    return knap_eval_close(n, k, R, V, k < 0 ? 1 : (int64_t)w[k], k < 0 ? 0 : (int64_t)v[k]);
}

}  // namespace

// One instance per NT lanes; 256 / NT instances per workgroup (form W: four waves that never wait
// for each other).  kLds: the node storage is in LDS (W, G) and the frontier is parked in the
// instance's slab slice between launches; otherwise it lives there (H).  The items are in LDS in
// every form.  idx_in lists the instances still running; one that is still running when its chunk
// is used up appends itself to idx_out (n_out counts them: the one word the host reads).
template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_knap_batch(KnapBatchBufs B,
                                                    const int32_t* __restrict__ idx_in, int n_in,
                                                    int32_t* __restrict__ idx_out,
                                                    int32_t* __restrict__ n_out, int chunk,
                                                    int slot_words) {
    extern __shared__ uint64_t smem[];
    constexpr int kPerWg = 256 / NT;
    constexpr int kWaves = NT / kWave;
    constexpr FenceScope kScope = kLds ? kFenceWave : kFenceWorkgroup;
    const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / NT);
    const int lane = (int)threadIdx.x % NT;
    const int wl = lane & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(lane / kWave);
    const int at = (int)blockIdx.x * kPerWg + sub;
    if (at >= n_in) return;  // whole waves (W), the whole workgroup (G, H)
    const int k = idx_in[at];
    KnapBatchDesc* const d = B.desc + k;
    int64_t* const scratch = reinterpret_cast<int64_t*>(smem);  // s_v, s_i, s_cnt: kWaves each
    uint64_t* const region = smem + kScratchWords + (size_t)sub * slot_words;

    const int n = d->n, nw = d->nw;
    const int64_t C = d->C, cap = d->cap;
    const int32_t narrate = d->narrate;
    uint32_t* const w = reinterpret_cast<uint32_t*>(region);
    uint32_t* const v = w + n;
    const KnapStore G = knap_store_at(B.slab + d->s_off, nw, cap);
    const KnapStore S = kLds ? knap_store_at(region + n, nw, cap) : G;

    int64_t evaluated = d->evaluated, widest = d->widest, inc_z = d->inc_z, inc_gid = d->inc_gid;
    int W = (int)d->width;
    int32_t levels = d->levels, cur = d->cur, found = d->inc_found, inc_stop = d->inc_stop;
    int32_t status = kRunning;

    for (int p = lane; p < n; p += NT) {
        w[p] = B.rw[d->item_off + p];
        v[p] = B.rv[d->item_off + p];
    }
    if (levels == 0) {  // the root: nothing fixed, no parent
        for (int t = lane; t < 2 * nw; t += NT) S.bits[0][t] = 0ull;
        if (lane == 0) S.par[0][0] = -1;
    } else if (kLds) {  // the frontier the last launch parked
        uint64_t* const sb = cur ? S.bits[1] : S.bits[0];
        const uint64_t* const gb = cur ? G.bits[1] : G.bits[0];
        int32_t* const sp = cur ? S.par[1] : S.par[0];
        const int32_t* const gp = cur ? G.par[1] : G.par[0];
        for (int64_t t = lane; t < (int64_t)W * 2 * nw; t += NT) sb[t] = gb[t];
        for (int t = lane; t < W; t += NT) sp[t] = gp[t];
    }
    group_sync<NT, kScope>();

    int done = 0;
    for (;;) {
        if (evaluated + W > cap) {  // section 11: a level is evaluated whole or not at all
            status = LPR_BB_NODE_CAP;
            break;
        }
        if (done >= chunk) break;  // still running: the next launch resumes here
        const uint64_t* const bits = cur ? S.bits[1] : S.bits[0];
        const int32_t* const par = cur ? S.par[1] : S.par[0];
        // ---- evaluation: a lane per node when a bitmap is one word, a wave per node otherwise
        if (nw == 1) {
            for (int i = lane; i < W; i += NT) {
                const KnapEval e = knap_eval_lane(bits[2 * i], bits[2 * i + 1], n, C, w, v);
                S.st[i] = e.st;
                S.stop[i] = e.stop;
                S.V[i] = e.V;
                S.bd[i] = e.bd;
            }
        } else {
            for (int i = wave; i < W; i += kWaves) {
                const uint64_t* F1 = bits + (size_t)i * 2 * nw;
                const KnapEval e = knap_eval_wave(F1, F1 + nw, nw, n, C, w, v, wl);
                if (wl == 0) {
                    S.st[i] = e.st;
                    S.stop[i] = e.stop;
                    S.V[i] = e.V;
                    S.bd[i] = e.bd;
                }
            }
        }
        group_sync<NT, kScope>();
        // ---- incumbent: (largest V, lowest index) over the feasible nodes.  A lane's strided
        // walk keeps its first maximum and every fold prefers the lower index.
        int64_t bv = -1;
        int bi = INT32_MAX;
        for (int i = lane; i < W; i += NT)
            if (S.st[i] != kKnapInfeasible && S.V[i] > bv) {
                bv = S.V[i];
                bi = i;
            }
#pragma unroll
        for (int m = kWave / 2; m > 0; m >>= 1) {
            const int64_t ov = shfl_xor64(bv, m);
            const int oi = __shfl_xor(bi, m, kWave);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if constexpr (kWaves > 1) {
            if (wl == 0) {
                scratch[wave] = bv;
                scratch[kWaves + wave] = bi;
            }
            __syncthreads();
            bv = scratch[0];
            bi = (int)scratch[kWaves];
#pragma unroll
            for (int q = 1; q < kWaves; ++q) {
                const int64_t ov = scratch[q];
                const int oi = (int)scratch[kWaves + q];
                if (ov > bv || (ov == bv && oi < bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
        }
        if (bv >= 0 && (!found || bv > inc_z)) {  // only a strictly larger candidate replaces
            inc_z = bv;
            found = 1;
            inc_stop = S.stop[bi];
            inc_gid = evaluated + bi;
            for (int t = lane; t < 2 * nw; t += NT)
                B.inc_bits[d->bits_off + t] = bits[(size_t)bi * 2 * nw + t];
        }
        // ---- pruning against the Z* just scored, the records, and the stable compaction of the
        // parents to branch: the r-th of them is the parent of children 2r and 2r + 1, which get
        // its record index now (the copy of the bitmaps waits for the count)
        const double zd = (double)inc_z;  // Z* <= 2^44: exact
        int32_t* const npar = cur ? S.par[0] : S.par[1];
        int run = 0;
        for (int b0 = 0; b0 < W; b0 += NT) {
            const int i = b0 + lane;
            bool f = false;
            if (i < W) {
                int32_t s = S.st[i];
                if (s == kKnapFractional) {
                    f = !found || S.bd[i] > zd;
                    if (!f) {
                        s = kKnapPruned;
                        S.st[i] = s;
                    }
                }
                const int64_t g = evaluated + i;
                if (g < narrate) {
                    const int64_t r = d->log_off + g;
                    B.log.par[r] = par[i];
                    B.log.br[r] = levels == 0 ? 0 : (i & 1);
                    B.log.st[r] = s;
                    B.log.kp[r] = s == kKnapFractional || s == kKnapPruned ? S.stop[i] : -1;
                    B.log.bd[r] = S.bd[i];
                    B.log.V[r] = S.V[i];
                }
            }
            const uint64_t mask = __ballot(f);
            const int below = __popcll(mask & ((1ull << wl) - 1ull));
            int off = 0, total = __popcll(mask);
            if constexpr (kWaves > 1) {
                __syncthreads();  // the slots of the previous step (or the arg-max) have been read
                if (wl == 0) scratch[2 * kWaves + wave] = total;
                __syncthreads();
                total = 0;
#pragma unroll
                for (int q = 0; q < kWaves; ++q) {
                    const int c = (int)scratch[2 * kWaves + q];
                    if (q < wave) off += c;
                    total += c;
                }
            }
            if (f) {
                const int64_t r = run + off + below;
                if (2 * r + 1 < cap) {  // past that the count below ends the instance
                    npar[2 * r] = (int32_t)(evaluated + i);
                    npar[2 * r + 1] = (int32_t)(evaluated + i);
                }
            }
            run += total;
        }
        const int64_t level_base = evaluated;
        evaluated += W;
        levels += 1;
        widest = widest > W ? widest : (int64_t)W;
        done += W;
        const int64_t children = 2 * (int64_t)run;
        if (children == 0) {
            status = LPR_OK_OPTIMAL;
            break;
        }
        // The restatement builds the children and finds evaluated + width > node_cap at the top of
        // its next loop; nothing happens in between, so its records, evaluated, levels, widest and
        // incumbent are final here already and the outcome is the same.  Counting before writing
        // is what lets a buffer of node_cap nodes do: children that are written are evaluated,
        // so children <= node_cap - evaluated.
        if (evaluated + children > cap) {
            status = LPR_BB_NODE_CAP;
            break;
        }
        group_sync<NT, kScope>();  // npar is complete
        // ---- children .1 (x_k = 0: k joins F0) then .2 (x_k = 1: k joins F1), in parent order
        uint64_t* const nbits = cur ? S.bits[0] : S.bits[1];
        if (nw == 1) {
            for (int c = lane; c < (int)children; c += NT) {
                const int i = (int)(npar[c] - level_base);
                const uint64_t kb = 1ull << S.stop[i];
                nbits[2 * c] = bits[2 * i] | ((c & 1) ? kb : 0ull);
                nbits[2 * c + 1] = bits[2 * i + 1] | ((c & 1) ? 0ull : kb);
            }
        } else {
            for (int c = wave; c < (int)children; c += kWaves) {
                const int i = (int)(npar[c] - level_base);
                const int kk = S.stop[i];
                const int kw = (c & 1) ? kk / kWave : nw + kk / kWave;
                const uint64_t kb = 1ull << (kk % kWave);
                const uint64_t* src = bits + (size_t)i * 2 * nw;
                uint64_t* dst = nbits + (size_t)c * 2 * nw;
                for (int t = wl; t < 2 * nw; t += kWave) dst[t] = t == kw ? (src[t] | kb) : src[t];
            }
        }
        group_sync<NT, kScope>();
        cur ^= 1;
        W = (int)children;
    }

    if (kLds && status == kRunning) {  // park the frontier
        const uint64_t* const sb = cur ? S.bits[1] : S.bits[0];
        uint64_t* const gb = cur ? G.bits[1] : G.bits[0];
        const int32_t* const sp = cur ? S.par[1] : S.par[0];
        int32_t* const gp = cur ? G.par[1] : G.par[0];
        for (int64_t t = lane; t < (int64_t)W * 2 * nw; t += NT) gb[t] = sb[t];
        for (int t = lane; t < W; t += NT) gp[t] = sp[t];
    }
    if (lane == 0) {
        d->evaluated = evaluated;
        d->width = W;
        d->widest = widest;
        d->inc_z = inc_z;
        d->inc_gid = inc_gid;
        d->levels = levels;
        d->cur = cur;
        d->inc_found = found;
        d->inc_stop = inc_stop;
        d->status = status;
        if (status == kRunning) idx_out[atomicAdd(n_out, 1)] = k;
    }
}

// The 0/1 DP of one instance per NT lanes: dp'[c] = max(dp[c], dp[c - w] + v) over an int64 row
// initialised to 0, items in input order, items heavier than the capacity skipped.  kLds: the
// row is in LDS and an item walks it downwards in chunks of NT * kKnapBatchDpCells cells; every
// lane reads its cells of a chunk before any lane writes (a chunk reads only itself and lower
// cells, and those are written after a later barrier).  Otherwise (H) two global rows ping-pong,
// one barrier per item, and a launch stops after kKnapBatchDpWork cell updates.
template <int NT, bool kLds>
__global__ __launch_bounds__(256) void k_knap_batch_dp(KnapBatchBufs B,
                                                       const int32_t* __restrict__ idx, int n_in,
                                                       int64_t* __restrict__ rows,
                                                       int64_t* __restrict__ best,
                                                       int slot_words) {
    extern __shared__ uint64_t smem[];
    constexpr int kPerWg = 256 / NT;
    const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / NT);
    const int lane = (int)threadIdx.x % NT;
    const int at = (int)blockIdx.x * kPerWg + sub;
    if (at >= n_in) return;
    const int k = idx[at];
    KnapBatchDesc* const d = B.desc + k;
    const int n = d->n;
    const int64_t C = d->C, cells = C + 1;
    const uint32_t* const ow = B.ow + d->item_off;
    const uint32_t* const ov = B.ov + d->item_off;
    if constexpr (kLds) {
        int64_t* const L = reinterpret_cast<int64_t*>(smem + kScratchWords + (size_t)sub * slot_words);
        const int ncell = (int)cells;
        for (int c = lane; c < ncell; c += NT) L[c] = 0;
        group_sync<NT, kFenceWave>();
        for (int j = 0; j < n; ++j) {
            const int64_t wj64 = ow[j];
            if (wj64 > C) continue;
            const int wj = (int)wj64;
            const int64_t vj = ov[j];
            for (int hi = ncell; hi > wj; hi -= NT * kKnapBatchDpCells) {
                int64_t nv[kKnapBatchDpCells];
#pragma unroll
                for (int r = 0; r < kKnapBatchDpCells; ++r) {
                    const int x = hi - 1 - lane - r * NT;
                    if (x >= wj) {
                        const int64_t keep = L[x];
                        const int64_t take = L[x - wj] + vj;
                        nv[r] = take > keep ? take : keep;
                    }
                }
                group_sync<NT, kFenceWave>();
#pragma unroll
                for (int r = 0; r < kKnapBatchDpCells; ++r) {
                    const int x = hi - 1 - lane - r * NT;
                    if (x >= wj) L[x] = nv[r];
                }
            }
            group_sync<NT, kFenceWave>();
        }
        if (lane == 0) best[k] = L[C];
    } else {
        int64_t* const row0 = rows + d->dp_row;
        int64_t* const row1 = row0 + cells;
        int j = d->dp_item, cur = d->dp_cur;
        if (j == 0) {
            for (int64_t c = lane; c < cells; c += NT) row0[c] = 0;
            cur = 0;
        }
        __syncthreads();
        int64_t work = 0;
        for (; j < n; ++j) {
            const int64_t wj = ow[j];
            if (wj > C) continue;
            if (work > 0 && work + cells > kKnapBatchDpWork) break;
            const int64_t vj = ov[j];
            const int64_t* const in = cur ? row1 : row0;
            int64_t* const out = cur ? row0 : row1;
            for (int64_t c = lane; c < cells; c += NT) {
                int64_t a = in[c];
                if (c >= wj) {
                    const int64_t b = in[c - wj] + vj;
                    a = b > a ? b : a;
                }
                out[c] = a;
            }
            __syncthreads();
            cur ^= 1;
            work += cells;
        }
        if (lane == 0) {
            d->dp_item = j;
            d->dp_cur = cur;
            if (j >= n) best[k] = (cur ? row1 : row0)[C];
        }
    }
}

// The launchers name their ABI call and pass no noun: batch_launch's message then gives the LDS
// bytes.  The workgroup's scratch is dynamic LDS here, so the attribute covers it too.
constexpr size_t kKnapBatchAttr = kBatchMaxLdsG + kBatchWgScratch;

// slot_bytes: the LDS of one instance of this form in this call (a multiple of 8): the largest
// footprint (W, G) or the largest items block (H).
int knap_batch_launch(int form, hipStream_t s, const KnapBatchBufs& B, size_t slot_bytes,
                      const int32_t* idx_in, int n_in, int32_t* idx_out, int32_t* n_out,
                      int chunk) {
    const char* const name = "lpr_knap_batch_solve";
    const int slot_words = (int)(slot_bytes / sizeof(uint64_t));
    const size_t lds = kBatchWgScratch + slot_bytes;
    if (form == kFormW)
        return batch_launch<&k_knap_batch<kWave, true>>(
            name, nullptr, form, s, n_in, kBatchWgScratch + 4 * slot_bytes, kKnapBatchAttr, B,
            idx_in, n_in, idx_out, n_out, chunk, slot_words);
    if (form == kFormG)
        return batch_launch<&k_knap_batch<256, true>>(name, nullptr, form, s, n_in, lds,
                                                      kKnapBatchAttr, B, idx_in, n_in, idx_out,
                                                      n_out, chunk, slot_words);
    return batch_launch<&k_knap_batch<256, false>>(name, nullptr, form, s, n_in, lds,
                                                   kKnapBatchAttr, B, idx_in, n_in, idx_out, n_out,
                                                   chunk, slot_words);
}

// slot_bytes: the largest row of this form in this call (W, G); unused in form H.
int knap_batch_launch_dp(int form, hipStream_t s, const KnapBatchBufs& B, size_t slot_bytes,
                         const int32_t* idx, int n_in, int64_t* rows, int64_t* best) {
    const char* const name = "lpr_knap_batch_dp";
    const int slot_words = (int)(slot_bytes / sizeof(uint64_t));
    if (form == kFormW)
        return batch_launch<&k_knap_batch_dp<kWave, true>>(
            name, nullptr, form, s, n_in, kBatchWgScratch + 4 * slot_bytes, kKnapBatchAttr, B, idx,
            n_in, rows, best, slot_words);
    if (form == kFormG)
        return batch_launch<&k_knap_batch_dp<256, true>>(
            name, nullptr, form, s, n_in, kBatchWgScratch + slot_bytes, kKnapBatchAttr, B, idx,
            n_in, rows, best, slot_words);
    return batch_launch<&k_knap_batch_dp<256, false>>(name, nullptr, form, s, n_in,
                                                      kBatchWgScratch, kKnapBatchAttr, B, idx,
                                                      n_in, rows, best, 0);
}

}  // namespace lpr
