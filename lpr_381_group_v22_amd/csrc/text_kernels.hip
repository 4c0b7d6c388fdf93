// text_kernels.hip -- the device text formatter (lpr_text_*): the bytes of
// TableIterationFormater.Format (Utilities/TableIterationFormater.cs:22-48) without its title
// line, for every block of a call.  Two passes over the cells with the number core of
// text_common.hpp -- measure (row lengths) and write (every byte to its final place) -- around an
// exclusive scan of the row lengths; cells of 1e15 or more are listed by the write pass and
// finished by a kernel of their own, so the two passes carry none of its arrays.  No kernel waits
// for another workgroup: the order is the stream's.
#include "bb_device_round.hpp"
#include "engine_common.hpp"
#include "text_common.hpp"

#include <algorithm>

namespace lpr {
namespace {

constexpr int kTextWg = 256;                  // four waves
constexpr int kTextWavesPerWg = kTextWg / kWave;
constexpr int64_t kTextMaxGrid = 1 << 16;     // workgroups of a pass; waves stride over the tasks

// The block of wave task t: the last one whose wave0 is <= t (wave0 is non-decreasing and
// blk[0].wave0 == 0; every block has at least one task).  Uniform over the wave.
__device__ __forceinline__ int64_t text_block_of(const TextBlock* blk, int64_t n_blk, int64_t t) {
    int64_t lo = 0, hi = n_blk - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (blk[mid].wave0 <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The bits of a cell as it is formatted.  kRound: after B.round4 applications of Math.Round(v, 4)
// (DisplayTableau, BranchBoundSimplexSolver.cs:623-640) -- dn_round4, the
// second one evaluated as dn_round4_twice evaluates it, only where the first result is 1e11 or
// more.  Both passes load their cells through this, so they see the same value.
template <bool kRound>
__device__ __forceinline__ uint64_t text_cell_bits(const double* p, int n) {
    double v = *p;
    if constexpr (kRound) {
        if (n >= 1) {
            v = dn_round4(v);
            if (n >= 2 && !(fabs(v) < 1e11)) v = dn_round4(v);
        }
    }
    return (uint64_t)__double_as_longlong(v);
}

// Measure: row_len[r] = the bytes of row r, label and line end included; *big_count += the cells
// of 1e15 or more.
template <bool kRound>
__global__ __launch_bounds__(kTextWg) void k_text_measure(const TextBlock* __restrict__ blk,
                                                          int64_t n_blk, int64_t n_tasks,
                                                          int64_t* __restrict__ row_len,
                                                          uint32_t* __restrict__ big_count) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_waves = (int64_t)gridDim.x * kTextWavesPerWg;
    for (int64_t t = (int64_t)blockIdx.x * kTextWavesPerWg + threadIdx.x / kWave; t < n_tasks;
         t += n_waves) {
        const TextBlock B = blk[text_block_of(blk, n_blk, t)];
        const int L = B.lanes, g = lane & (L - 1);
        const int64_t row = (t - B.wave0) * (kWave / L) + lane / L;
        const bool valid = row < B.rows;
        int32_t sum = 0;
        uint32_t big = 0;
        if (valid) {
            const double* src = B.src + row * B.cols;
            for (int32_t j = g; j < B.cols; j += L) {
                const TextCell c = text_cell_measure(text_cell_bits<kRound>(src + j, B.round4));
                sum += c.len;
                big += c.cls == kTextBig;
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, kWave);
        if (valid && g == 0) row_len[B.row0 + row] = sum + text_row_frame_len((int32_t)row, B.cols);
        if (big) atomicAdd(big_count, big);
    }
}

// Exclusive scan of 256 values, one per lane of the workgroup; *total gets their sum.
__device__ __forceinline__ int64_t text_wg_exclusive(int64_t v, int64_t* lds4, int64_t* total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int64_t incl = v;
    for (int o = 1; o < kWave; o <<= 1) {
        const int64_t up = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += up;
    }
    __syncthreads();  // lds4 may still be read from the call before
    if (lane == kWave - 1) lds4[wave] = incl;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int q = 0; q < kTextWavesPerWg; ++q) {
        if (q < wave) before += lds4[q];
        all += lds4[q];
    }
    *total = all;
    return before + incl - v;
}

constexpr int kTextPerLane = kTextScanTile / kTextWg;

__global__ __launch_bounds__(kTextWg) void k_text_scan_reduce(const int64_t* __restrict__ v,
                                                              int64_t n,
                                                              int64_t* __restrict__ partials) {
    __shared__ int64_t lds4[kTextWavesPerWg];
    const int64_t at = (int64_t)blockIdx.x * kTextScanTile + (int64_t)threadIdx.x * kTextPerLane;
    int64_t mine = 0;
    for (int q = 0; q < kTextPerLane; ++q)
        if (at + q < n) mine += v[at + q];
    int64_t total;
    (void)text_wg_exclusive(mine, lds4, &total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// One workgroup: the partials become their exclusive prefix, 256 at a time behind a carry.
__global__ __launch_bounds__(kTextWg) void k_text_scan_top(int64_t* __restrict__ partials,
                                                           int64_t n) {
    __shared__ int64_t lds4[kTextWavesPerWg];
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += kTextWg) {
        const int64_t i = base + threadIdx.x;
        const int64_t mine = i < n ? partials[i] : 0;
        int64_t total;
        const int64_t ex = text_wg_exclusive(mine, lds4, &total);
        if (i < n) partials[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kTextWg) void k_text_scan_apply(int64_t* __restrict__ v, int64_t n,
                                                             const int64_t* __restrict__ partials) {
    __shared__ int64_t lds4[kTextWavesPerWg];
    const int64_t at = (int64_t)blockIdx.x * kTextScanTile + (int64_t)threadIdx.x * kTextPerLane;
    int64_t x[kTextPerLane], mine = 0;
    for (int q = 0; q < kTextPerLane; ++q) {
        x[q] = at + q < n ? v[at + q] : 0;
        mine += x[q];
    }
    int64_t total;
    int64_t run = partials[blockIdx.x] + text_wg_exclusive(mine, lds4, &total);
    for (int q = 0; q < kTextPerLane; ++q) {
        if (at + q < n) v[at + q] = run;
        run += x[q];
    }
}

// offsets[b]: where block b starts in the text; offsets[n_blk]: the bytes of the whole text.
__global__ void k_text_offsets(const TextBlock* __restrict__ blk, int64_t n_blk, int64_t n_rows,
                               const int64_t* __restrict__ row_at, int64_t* __restrict__ offsets) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blk) return;
    const TextBlock B = blk[b];
    offsets[b] = row_at[B.row0] + B.hdr_end - text_header_len(B.cols, B.nvars);
    if (b == n_blk - 1) offsets[n_blk] = row_at[n_rows] + B.hdr_end;
}

// "x1\t" .. "x{n}\t" (or t) at dst, by the 64 lanes of a wave
__device__ __forceinline__ void text_put_labels(uint8_t* dst, char letter, int64_t n, int lane) {
    for (int64_t j = 1 + lane; j <= n; j += kWave) {
        uint8_t* p = dst + 2 * (j - 1) + text_sum_ndigits(j - 1);
        const int nd = text_ndigits32((uint32_t)j);
        p[0] = (uint8_t)letter;
        text_put_uint32(p + 1, (uint32_t)j, nd);
        p[1 + nd] = '\t';
    }
}

// Write: every byte of every block but the bytes of the big cells, which are listed.
template <bool kRound>
__global__ __launch_bounds__(kTextWg) void k_text_write(const TextBlock* __restrict__ blk,
                                                        int64_t n_blk, int64_t n_tasks,
                                                        const int64_t* __restrict__ row_at,
                                                        uint8_t* __restrict__ text,
                                                        TextBigCell* __restrict__ big,
                                                        uint32_t big_cap,
                                                        uint32_t* __restrict__ big_fill) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_waves = (int64_t)gridDim.x * kTextWavesPerWg;
    for (int64_t t = (int64_t)blockIdx.x * kTextWavesPerWg + threadIdx.x / kWave; t < n_tasks;
         t += n_waves) {
        const TextBlock B = blk[text_block_of(blk, n_blk, t)];
        if (t == B.wave0) {  // the block's first wave also writes the rule and the "Table" line
            const int64_t xs = text_labels_len(B.nvars), tc = text_tcount(B.cols, B.nvars);
            uint8_t* h = text + row_at[B.row0] + B.hdr_end - text_header_len(B.cols, B.nvars);
            for (int i = lane; i < kTextDashes; i += kWave) h[i] = '-';
            if (lane == 0) {
                h[kTextDashes] = '\r';
                h[kTextDashes + 1] = '\n';
                text_put_literal(h + kTextRuleLen, "Table\t", (int)kTextTableLen);
                text_put_literal(h + kTextRuleLen + kTextTableLen + xs + text_labels_len(tc),
                                 "RHS\r\n", 5);
            }
            text_put_labels(h + kTextRuleLen + kTextTableLen, 'x', B.nvars, lane);
            text_put_labels(h + kTextRuleLen + kTextTableLen + xs, 't', tc, lane);
        }
        const int L = B.lanes, g = lane & (L - 1);
        const int64_t row = (t - B.wave0) * (kWave / L) + lane / L;
        const bool valid = row < B.rows;
        const double* src = B.src + (valid ? row : 0) * B.cols;
        int64_t pos = 0;
        if (valid) {
            pos = row_at[B.row0 + row] + B.hdr_end;
            const int nl = text_row_label_len((int32_t)row);
            if (g == 0) {
                if (row == 0)
                    text[pos] = 'Z';
                else
                    text_put_uint32(text + pos, (uint32_t)row, nl);
                text[pos + nl] = '\t';
            }
            pos += nl + 1;
        }
        for (int32_t j0 = 0; j0 < B.cols; j0 += L) {  // the same trips for every lane of the wave
            const bool has = valid && j0 + g < B.cols;
            TextCell c;
            c.len = 0;
            uint64_t bits = 0;
            if (has) {
                bits = text_cell_bits<kRound>(src + j0 + g, B.round4);
                c = text_cell_measure(bits);
            }
            const int32_t len1 = has ? c.len + 1 : 0;  // the cell and its tab
            int32_t incl = len1;
            for (int o = 1; o < L; o <<= 1) {
                const int32_t up = __shfl_up(incl, o, L);
                if (g >= o) incl += up;
            }
            const int32_t total = __shfl(incl, L - 1, L);
            if (has) {
                const int64_t at = pos + incl - len1;
                if (c.cls == kTextBig) {
                    const uint32_t q = atomicAdd(big_fill, 1u);
                    if (q < big_cap) big[q] = TextBigCell{bits, at};
                } else {
                    text_cell_put(c, text + at);
                }
                text[at + c.len] = '\t';
            }
            pos += total;
        }
        if (valid && g == 0) {
            text[pos] = '\r';
            text[pos + 1] = '\n';
        }
    }
}

// The slow path: one lane per listed cell, its 33 + 35 words in scratch.
__global__ __launch_bounds__(kTextWg) void k_text_big(const TextBigCell* __restrict__ big,
                                                      uint32_t n, uint8_t* __restrict__ text) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) (void)text_big_put(big[i].bits, text + big[i].at);
}

int text_grid(int64_t n_tasks) {
    return (int)std::min<int64_t>((n_tasks + kTextWavesPerWg - 1) / kTextWavesPerWg, kTextMaxGrid);
}

}  // namespace

void text_launch_measure(hipStream_t s, bool rounded, const TextBlock* blk, int64_t n_blk,
                         int64_t n_tasks, int64_t* rows_scan, uint32_t* big_count) {
    auto* k = rounded ? k_text_measure<true> : k_text_measure<false>;
    hipLaunchKernelGGL(k, dim3(text_grid(n_tasks)), dim3(kTextWg), 0, s, blk, n_blk, n_tasks,
                       rows_scan, big_count);
}

void text_launch_scan(hipStream_t s, int64_t* rows_scan, int64_t n, int64_t* partials) {
    const int64_t tiles = (n + kTextScanTile - 1) / kTextScanTile;
    hipLaunchKernelGGL(k_text_scan_reduce, dim3((unsigned)tiles), dim3(kTextWg), 0, s, rows_scan, n,
                       partials);
    hipLaunchKernelGGL(k_text_scan_top, dim3(1), dim3(kTextWg), 0, s, partials, tiles);
    hipLaunchKernelGGL(k_text_scan_apply, dim3((unsigned)tiles), dim3(kTextWg), 0, s, rows_scan, n,
                       partials);
}

void text_launch_offsets(hipStream_t s, const TextBlock* blk, int64_t n_blk, int64_t n_rows,
                         const int64_t* rows_scan, int64_t* offsets) {
    hipLaunchKernelGGL(k_text_offsets, dim3((unsigned)((n_blk + kTextWg - 1) / kTextWg)),
                       dim3(kTextWg), 0, s, blk, n_blk, n_rows, rows_scan, offsets);
}

void text_launch_write(hipStream_t s, bool rounded, const TextBlock* blk, int64_t n_blk,
                       int64_t n_tasks, const int64_t* rows_scan, uint8_t* text, TextBigCell* big,
                       uint32_t big_cap, uint32_t* big_fill) {
    auto* k = rounded ? k_text_write<true> : k_text_write<false>;
    hipLaunchKernelGGL(k, dim3(text_grid(n_tasks)), dim3(kTextWg), 0, s, blk, n_blk, n_tasks,
                       rows_scan, text, big, big_cap, big_fill);
}

void text_launch_big(hipStream_t s, const TextBigCell* big, uint32_t n, uint8_t* text) {
    hipLaunchKernelGGL(k_text_big, dim3((n + kTextWg - 1) / kTextWg), dim3(kTextWg), 0, s, big, n,
                       text);
}

}  // namespace lpr
