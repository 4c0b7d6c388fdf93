// knapsack_kernels.hip -- device side of menu option 5 (Program.cs:430-470): the 0/1 DP of
// KnapsackBranchBoundSolver.Solve and the level-synchronous branch-and-bound of
// KnapsackBranchBoundSimplex.  Rules: DESIGN.md section 11.  All sums are int64, so only the three
// floating-point operations of the bound need care (ieee_div, one product, one sum).
#include "knapsack_common.hpp"

#pragma clang fp contract(off)

namespace lpr {

// ================================================================ 0/1 DP
// dp'[c] = max(dp[c], dp[c - w] + v) for c >= w, dp'[c] = dp[c] below.  Rows ping-pong in HBM.

// One item, one pass over the row (items whose weight exceeds the LDS halo, and variant 1).
__global__ __launch_bounds__(256) void k_knap_dp_stream(const int64_t* __restrict__ in,
                                                        int64_t* __restrict__ out, int64_t cells,
                                                        int64_t w, int64_t v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
        int64_t a = in[c];
        if (c >= w) {
            const int64_t b = in[c - w] + v;
            a = b > a ? b : a;
        }
        out[c] = a;
    }
}

// Items [j0, j1) with weight sum S <= kKnapHalo, applied in order inside LDS.  The workgroup owns
// output cells [a, a + kKnapTile) and loads dp[a - S, a + kKnapTile) once (local x = global - a + S).
// After item j (prefix weight W_j) the cells x >= W_j hold the exact row after item j: cell x
// reads x - w_j >= W_{j-1}.  Cells below that are not computed.  Within an item the cells are
// walked downwards in chunks of kKnapDpChunk (kKnapDpCells per thread, all read before any is
// written); a chunk reads only itself and lower cells, and every lower chunk is written after a
// later barrier, so one barrier per chunk separates reads from writes.
__global__ __launch_bounds__(kKnapDpThreads) void k_knap_dp_block(
    const int64_t* __restrict__ in, int64_t* __restrict__ out, int64_t cells,
    const int32_t* __restrict__ w, const int32_t* __restrict__ v, int j0, int j1, int S) {
    __shared__ int64_t L[kKnapHalo + kKnapTile];
    const int tid = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * kKnapTile;
    const int cnt = (int)((cells - a) < kKnapTile ? (cells - a) : kKnapTile);
    const int span = S + cnt;
    const int lo0 = a >= S ? 0 : (int)(S - a);  // first local cell with a global index >= 0
    for (int x = lo0 + tid; x < span; x += kKnapDpThreads) L[x] = in[a - S + x];
    __syncthreads();
    int W = 0;
    for (int j = j0; j < j1; ++j) {
        const int wj = w[j];
        const int64_t vj = v[j];
        W += wj;
        // x >= W: valid after item j; x >= lo0 + wj: the item fits (global index >= w_j)
        const int lo = W > lo0 + wj ? W : lo0 + wj;
        for (int hi = span; hi > lo; hi -= kKnapDpChunk) {
            int64_t nv[kKnapDpCells];
#pragma unroll
            for (int r = 0; r < kKnapDpCells; ++r) {
                const int x = hi - 1 - tid - r * kKnapDpThreads;
                if (x >= lo) {
                    const int64_t keep = L[x];
                    const int64_t take = L[x - wj] + vj;
                    nv[r] = take > keep ? take : keep;
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kKnapDpCells; ++r) {
                const int x = hi - 1 - tid - r * kKnapDpThreads;
                if (x >= lo) L[x] = nv[r];
            }
        }
        __syncthreads();
    }
    for (int x = S + tid; x < span; x += kKnapDpThreads) out[a - S + x] = L[x];
}

void knap_launch_dp_block(hipStream_t s, const int64_t* in, int64_t* out, int64_t cells,
                          const int32_t* w, const int32_t* v, int j0, int j1, int S) {
    const int64_t tiles = (cells + kKnapTile - 1) / kKnapTile;
    hipLaunchKernelGGL(k_knap_dp_block, dim3((unsigned)tiles), dim3(kKnapDpThreads), 0, s, in, out,
                       cells, w, v, j0, j1, S);
}

void knap_launch_dp_stream(hipStream_t s, const int64_t* in, int64_t* out, int64_t cells,
                           int64_t w, int64_t v, int num_cus) {
    int64_t blocks = (cells + 255) / 256;
    const int64_t most = (int64_t)(num_cus > 0 ? num_cus : 256) * 16;
    if (blocks > most) blocks = most;
    hipLaunchKernelGGL(k_knap_dp_stream, dim3((unsigned)blocks), dim3(256), 0, s, in, out, cells,
                       w, v);
}

// ================================================================ branch-and-bound
// One wave per node.  Node i's bitmaps are nodes[i * 2nw, +nw) = F1 and the next nw words = F0,
// over rank positions.  w, v are in rank order.
__global__ __launch_bounds__(kKnapEvalWaves * kWave) void k_knap_eval(
    const uint64_t* __restrict__ nodes, int nw, int n, int64_t C, const int64_t* __restrict__ w,
    const int64_t* __restrict__ v, int64_t W, int32_t* __restrict__ st, int32_t* __restrict__ kp,
    int32_t* __restrict__ stop, int64_t* __restrict__ Vout, double* __restrict__ bd) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t node = (int64_t)blockIdx.x * kKnapEvalWaves + (threadIdx.x / kWave);
    if (node >= W) return;  // whole waves
    const uint64_t* F1 = nodes + (size_t)node * 2 * nw;
    const uint64_t* F0 = F1 + nw;
    const KnapEval e = knap_eval_wave(F1, F0, nw, n, C, w, v, lane);
    if (lane != 0) return;
    st[node] = e.st;
    kp[node] = e.kp;
    stop[node] = e.stop;
    Vout[node] = e.V;
    bd[node] = e.bd;
}

void knap_launch_eval(hipStream_t s, const uint64_t* nodes, int nw, int n, int64_t C,
                      const int64_t* w, const int64_t* v, int64_t W, int32_t* st, int32_t* kp,
                      int32_t* stop, int64_t* V, double* bd) {
    const int64_t blocks = (W + kKnapEvalWaves - 1) / kKnapEvalWaves;
    hipLaunchKernelGGL(k_knap_eval, dim3((unsigned)blocks), dim3(kKnapEvalWaves * kWave), 0, s,
                       nodes, nw, n, C, w, v, W, st, kp, stop, V, bd);
}

// The level step, one workgroup: incumbent arg-max (largest V, first index), a copy of the new
// incumbent's bitmaps, the pruned marks, the node log, and the stable compaction of the parents
// to branch (pos[i] = their rank among them, -1 otherwise).
constexpr int kKnapLevelThreads = 1024;
__global__ __launch_bounds__(kKnapLevelThreads) void k_knap_level(
    int64_t W, int64_t base, const uint64_t* __restrict__ nodes, int nw,
    const int32_t* __restrict__ par, const int32_t* __restrict__ br, int32_t* __restrict__ st,
    const int32_t* __restrict__ kp, const int32_t* __restrict__ stop,
    const int64_t* __restrict__ V, const double* __restrict__ bd, int32_t* __restrict__ pos,
    KnapInc* inc, uint64_t* __restrict__ inc_bits, KnapLevel* lvl, KnapLog log) {
    constexpr int kWaves = kKnapLevelThreads / kWave;
    __shared__ int64_t s_v[kWaves], s_i[kWaves];
    __shared__ int64_t s_cnt[kWaves];
    __shared__ int64_t s_copy, s_z;
    __shared__ int32_t s_found;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    // arg-max: a thread's strided walk keeps its first maximum, the folds prefer the lower index
    int64_t bv = -1, bi = INT64_MAX;
    for (int64_t i = tid; i < W; i += kKnapLevelThreads)
        if (st[i] != kKnapInfeasible && V[i] > bv) {
            bv = V[i];
            bi = i;
        }
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const int64_t ov = shfl_xor64(bv, m), oi = shfl_xor64(bi, m);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < kWaves; ++q)
            if (s_v[q] > bv || (s_v[q] == bv && s_i[q] < bi)) {
                bv = s_v[q];
                bi = s_i[q];
            }
        int32_t found = inc->found;
        int64_t z = inc->z;
        s_copy = -1;
        if (bv >= 0 && (!found || bv > z)) {  // strictly larger replaces
            z = bv;
            found = 1;
            inc->z = z;
            inc->found = 1;
            inc->stop = stop[bi];
            inc->gid = base + bi;
            s_copy = bi;
        }
        s_z = z;
        s_found = found;
    }
    __syncthreads();
    if (s_copy >= 0)
        for (int t = tid; t < 2 * nw; t += kKnapLevelThreads)
            inc_bits[t] = nodes[(size_t)s_copy * 2 * nw + t];
    const double zd = (double)s_z;  // Z* <= 2^44: exact
    const bool found = s_found != 0;
    int64_t run = 0;
    for (int64_t b0 = 0; b0 < W; b0 += kKnapLevelThreads) {
        const int64_t i = b0 + tid;
        bool f = false;
        if (i < W) {
            int32_t s = st[i];
            if (s == kKnapFractional) {
                f = !found || bd[i] > zd;
                if (!f) {
                    s = kKnapPruned;
                    st[i] = s;
                }
            }
            const int64_t g = base + i;
            if (g < log.cap) {
                log.par[g] = par[i];
                log.br[g] = br[i];
                log.st[g] = s;
                log.kp[g] = kp[i];
                log.bd[g] = bd[i];
                log.V[g] = V[i];
            }
        }
        const uint64_t mask = __ballot(f);
        const int64_t below = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();  // s_cnt of the previous chunk has been read by everyone
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();
        int64_t off = run, total = 0;
        for (int q = 0; q < kWaves; ++q) {
            if (q < wave) off += s_cnt[q];
            total += s_cnt[q];
        }
        if (i < W) pos[i] = f ? (int32_t)(off + below) : -1;
        run += total;
    }
    if (tid == 0) {
        lvl->next_width = 2 * run;
        lvl->z = s_z;
        lvl->found = s_found;
        lvl->pad = 0;
    }
}

void knap_launch_level(hipStream_t s, int64_t W, int64_t base, const uint64_t* nodes, int nw,
                       const int32_t* par, const int32_t* br, int32_t* st, const int32_t* kp,
                       const int32_t* stop, const int64_t* V, const double* bd, int32_t* pos,
                       KnapInc* inc, uint64_t* inc_bits, KnapLevel* lvl, KnapLog log) {
    hipLaunchKernelGGL(k_knap_level, dim3(1), dim3(kKnapLevelThreads), 0, s, W, base, nodes, nw,
                       par, br, st, kp, stop, V, bd, pos, inc, inc_bits, lvl, log);
}

// One wave per parent: a branched parent p (pos[p] = r) writes child 2r (".1", x_k = 0: k joins
// F0) and child 2r + 1 (".2", x_k = 1: k joins F1).
__global__ __launch_bounds__(kKnapEvalWaves * kWave) void k_knap_children(
    int64_t W, int64_t base, const uint64_t* __restrict__ nodes, int nw,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ kp, uint64_t* __restrict__ next,
    int32_t* __restrict__ next_par, int32_t* __restrict__ next_br) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * kKnapEvalWaves + (threadIdx.x / kWave);
    if (i >= W) return;
    const int32_t r = pos[i];
    if (r < 0) return;
    const int k = kp[i];
    const int kw = k / kWave;
    const uint64_t kb = 1ull << (k % kWave);
    const uint64_t* src = nodes + (size_t)i * 2 * nw;
    uint64_t* c0 = next + (size_t)(2 * (int64_t)r) * 2 * nw;
    uint64_t* c1 = c0 + 2 * nw;
    for (int t = lane; t < 2 * nw; t += kWave) {
        const uint64_t x = src[t];
        c0[t] = t == nw + kw ? (x | kb) : x;
        c1[t] = t == kw ? (x | kb) : x;
    }
    if (lane == 0) {
        next_par[2 * (int64_t)r] = (int32_t)(base + i);
        next_par[2 * (int64_t)r + 1] = (int32_t)(base + i);
        next_br[2 * (int64_t)r] = 0;
        next_br[2 * (int64_t)r + 1] = 1;
    }
}

void knap_launch_children(hipStream_t s, int64_t W, int64_t base, const uint64_t* nodes, int nw,
                          const int32_t* pos, const int32_t* kp, uint64_t* next,
                          int32_t* next_par, int32_t* next_br) {
    const int64_t blocks = (W + kKnapEvalWaves - 1) / kKnapEvalWaves;
    hipLaunchKernelGGL(k_knap_children, dim3((unsigned)blocks), dim3(kKnapEvalWaves * kWave), 0, s,
                       W, base, nodes, nw, pos, kp, next, next_par, next_br);
}

}  // namespace lpr
