// text_engine.hip -- host side of the device text formatter (include/lpr_engine.h, lpr_text_* and
// lpr_batch_trace_text): the bytes of TableIterationFormater.Format
// (Utilities/TableIterationFormater.cs:22-48) for a ragged list of tableaux or for every kept
// record of a traced primal batch.  The host lays the blocks out (one descriptor each), the
// kernels of text_kernels.hip measure, scan and write; one small read between the two passes
// sizes the text.  An lpr_text owns the text and its offsets, nothing of its source.
#include "batch_common.hpp"
#include "text_common.hpp"

#include <algorithm>
#include <new>

using namespace lpr;

struct lpr_text {
    lpr_engine* eng = nullptr;
    int64_t blocks = 0, bytes = 0;
    uint8_t* text = nullptr;     // device, bytes
    int64_t* offsets = nullptr;  // device, blocks + 1
    double kernel_ms = 0.0;
};

namespace {

int text_oom(const char* what, int64_t n) {
    set_error("lpr_text: cannot allocate %s (%lld elements)", what, (long long)n);
    return LPR_OUT_OF_MEMORY;
}

void text_release_device(lpr_text* t) {
    hipFree(t->text);
    hipFree(t->offsets);
    t->text = nullptr;
    t->offsets = nullptr;
}

// What a call needs besides the text: freed when it returns, whatever it returns.
struct TextWork {
    TextBlock* blk = nullptr;
    int64_t* rows_scan = nullptr;
    int64_t* partials = nullptr;
    uint32_t* counters = nullptr;  // [0] big cells counted by measure  [1] listed by write
    TextBigCell* big = nullptr;
    double* upload = nullptr;      // lpr_text_format_tableaux: the tableaux
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~TextWork() {
        hipFree(blk);
        hipFree(rows_scan);
        hipFree(partials);
        hipFree(counters);
        hipFree(big);
        hipFree(upload);
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
};

// The layout fields of the descriptors (src, rows, cols, nvars, round4 are set): lanes, row0,
// wave0, hdr_end.  Returns the rows and wave tasks of the call, and whether any block is rounded.
bool text_lay_out(std::vector<TextBlock>& blk, int64_t* n_rows, int64_t* n_tasks) {
    int64_t r = 0, w = 0, h = 0;
    bool rounded = false;
    for (TextBlock& b : blk) {
        rounded = rounded || b.round4 != 0;
        b.lanes = (int16_t)text_lanes(b.cols);
        b.row0 = r;
        b.wave0 = w;
        h += text_header_len(b.cols, b.nvars);
        b.hdr_end = h;
        const int per_wave = kWave / b.lanes;
        r += b.rows;
        w += ((int64_t)b.rows + per_wave - 1) / per_wave;
    }
    *n_rows = r;
    *n_tasks = w;
    return rounded;
}

// Blocks laid out on the host -> an lpr_text on e.  wk.upload, when set, already holds what the
// descriptors point to (copied on e's stream).
int text_format(const char* W, lpr_engine* e, std::vector<TextBlock>& blk, TextWork& wk,
                lpr_text** out) {
    const int64_t n_blk = (int64_t)blk.size();
    int64_t n_rows = 0, n_tasks = 0;
    const bool rounded = text_lay_out(blk, &n_rows, &n_tasks);
    const int64_t n_scan = n_rows + 1;
    const int64_t tiles = (n_scan + kTextScanTile - 1) / kTextScanTile;
    if (tiles > INT32_MAX) {
        set_error("%s: %lld rows in one call are more than the scan takes", W, (long long)n_rows);
        return LPR_BAD_ARGUMENT;
    }
    lpr_text* t = new (std::nothrow) lpr_text();
    if (!t) return text_oom("handle", 1);
    int rc = LPR_OK_OPTIMAL;
    dev_alloc(&wk.blk, n_blk, "block descriptors", &rc, text_oom);
    dev_alloc(&wk.rows_scan, n_scan, "row offsets", &rc, text_oom);
    dev_alloc(&wk.partials, tiles, "scan partials", &rc, text_oom);
    dev_alloc(&wk.counters, 2, "counters", &rc, text_oom);
    dev_alloc(&t->offsets, n_blk + 1, "block offsets", &rc, text_oom);
    hipStream_t s = e->stream;
    struct {
        int64_t bytes;
        uint32_t big;
    } sized = {0, 0};
    auto first = [&]() -> int {
        for (hipEvent_t& ev : wk.ev) LPR_HIP(hipEventCreate(&ev));
        LPR_HIP(hipMemcpyAsync(wk.blk, blk.data(), (size_t)n_blk * sizeof(TextBlock),
                               hipMemcpyHostToDevice, s));
        LPR_HIP(hipMemsetAsync(wk.rows_scan, 0, (size_t)n_scan * sizeof(int64_t), s));
        LPR_HIP(hipMemsetAsync(wk.counters, 0, 2 * sizeof(uint32_t), s));
        LPR_HIP(hipEventRecord(wk.ev[0], s));
        text_launch_measure(s, rounded, wk.blk, n_blk, n_tasks, wk.rows_scan, wk.counters);
        text_launch_scan(s, wk.rows_scan, n_scan, wk.partials);
        text_launch_offsets(s, wk.blk, n_blk, n_rows, wk.rows_scan, t->offsets);
        LPR_HIP(hipGetLastError());
        LPR_HIP(hipEventRecord(wk.ev[1], s));
        LPR_HIP(hipMemcpyAsync(&sized.bytes, t->offsets + n_blk, sizeof(int64_t),
                               hipMemcpyDeviceToHost, s));
        LPR_HIP(hipMemcpyAsync(&sized.big, wk.counters, sizeof(uint32_t), hipMemcpyDeviceToHost,
                               s));
        LPR_HIP(hipStreamSynchronize(s));
        return LPR_OK_OPTIMAL;
    };
    if (rc == LPR_OK_OPTIMAL) rc = first();
    if (rc == LPR_OK_OPTIMAL) {
        dev_alloc(&t->text, std::max<int64_t>(sized.bytes, 1), "text", &rc, text_oom);
        if (sized.big > 0) dev_alloc(&wk.big, sized.big, "big-cell list", &rc, text_oom);
    }
    auto second = [&]() -> int {
        LPR_HIP(hipEventRecord(wk.ev[2], s));
        text_launch_write(s, rounded, wk.blk, n_blk, n_tasks, wk.rows_scan, t->text, wk.big, sized.big,
                          wk.counters + 1);
        if (sized.big > 0) text_launch_big(s, wk.big, sized.big, t->text);
        LPR_HIP(hipGetLastError());
        LPR_HIP(hipEventRecord(wk.ev[3], s));
        LPR_HIP(hipStreamSynchronize(s));
        float a = 0.f, b = 0.f;
        LPR_HIP(hipEventElapsedTime(&a, wk.ev[0], wk.ev[1]));
        LPR_HIP(hipEventElapsedTime(&b, wk.ev[2], wk.ev[3]));
        t->kernel_ms = (double)a + (double)b;
        return LPR_OK_OPTIMAL;
    };
    if (rc == LPR_OK_OPTIMAL) rc = second();
    if (rc != LPR_OK_OPTIMAL) {
        text_release_device(t);
        delete t;
        return rc;
    }
    t->eng = e;
    t->blocks = n_blk;
    t->bytes = sized.bytes;
    e->live_text.push_back(t);
    *out = t;
    return LPR_OK_OPTIMAL;
}

}  // namespace

namespace lpr {
void text_orphan(lpr_text* t) {  // lpr_engine_close
    text_release_device(t);
    t->eng = nullptr;
}
int text_format_blocks(const char* W, lpr_engine* e, std::vector<TextBlock>& blk, lpr_text** out) {
    TextWork wk;
    return text_format(W, e, blk, wk, out);
}
}  // namespace lpr

namespace {

// lpr_text_format_tableaux (round4 null: no block is rounded) and lpr_text_format_tableaux_rounded
int text_format_tableaux(const char* W, lpr_engine* e, int32_t count, const int32_t* rows,
                         const int32_t* cols, const int32_t* nvars, const int32_t* round4,
                         const double* tableaux, lpr_text** out) {
    if (!e || !out || count < 1 || !rows || !cols || !nvars || !tableaux) {
        set_error("%s: bad arguments (count=%d, or a null engine / out / rows / cols / nvars / "
                  "tableaux)", W, count);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    int64_t total = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (rows[k] < 1 || cols[k] < 1 || nvars[k] < 0) {
            set_error("%s: block %d is %d x %d with nvars %d; it needs rows >= 1, cols >= 1 and "
                      "nvars >= 0", W, k, rows[k], cols[k], nvars[k]);
            return LPR_BAD_ARGUMENT;
        }
        if (round4 && (round4[k] < 0 || round4[k] > kTextMaxRound4)) {
            set_error("%s: round4[%d] = %d; a block is rounded 0, 1 or 2 times", W, k, round4[k]);
            return LPR_BAD_ARGUMENT;
        }
        total += (int64_t)rows[k] * cols[k];  // a term is below 2^62 and total was at most 2^59
        if (total > INT64_MAX / 16) {
            set_error("%s: more than 2^59 cells at block %d", W, k);
            return LPR_BAD_ARGUMENT;
        }
    }
    LPR_HIP(hipSetDevice(e->device));
    TextWork wk;
    int rc = LPR_OK_OPTIMAL;
    dev_alloc(&wk.upload, total, "tableaux", &rc, text_oom);
    if (rc != LPR_OK_OPTIMAL) return rc;
    LPR_HIP(hipMemcpyAsync(wk.upload, tableaux, (size_t)total * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    std::vector<TextBlock> blk;
    try {
        blk.resize((size_t)count);
    } catch (...) {
        hipStreamSynchronize(e->stream);  // the upload reads the caller's memory
        return text_oom("block descriptors (host)", count);
    }
    int64_t at = 0;
    for (int32_t k = 0; k < count; ++k) {
        TextBlock& b = blk[(size_t)k];
        b.src = wk.upload + at;
        b.rows = rows[k];
        b.cols = cols[k];
        b.nvars = nvars[k];
        b.round4 = (int16_t)(round4 ? round4[k] : 0);
        at += (int64_t)rows[k] * cols[k];
    }
    rc = text_format(W, e, blk, wk, out);
    if (rc != LPR_OK_OPTIMAL) hipStreamSynchronize(e->stream);
    return rc;
}

}  // namespace

extern "C" {

// TableIterationFormater.Format (:22-48) without its title line, per tableau of a ragged list
int lpr_text_format_tableaux(lpr_engine* e, int32_t count, const int32_t* rows, const int32_t* cols,
                             const int32_t* nvars, const double* tableaux, lpr_text** out) {
    return text_format_tableaux("lpr_text_format_tableaux", e, count, rows, cols, nvars, nullptr,
                                tableaux, out);
}

// DisplayTableau (BranchBoundSimplexSolver.cs:623-640) per tableau of a ragged list: Format of the
// tableau after round4[k] applications of Math.Round(v, 4)
int lpr_text_format_tableaux_rounded(lpr_engine* e, int32_t count, const int32_t* rows,
                                     const int32_t* cols, const int32_t* nvars,
                                     const int32_t* round4, const double* tableaux,
                                     lpr_text** out) {
    static const char* W = "lpr_text_format_tableaux_rounded";
    if (!round4) {
        set_error("%s: null round4", W);
        return LPR_BAD_ARGUMENT;
    }
    return text_format_tableaux(W, e, count, rows, cols, nvars, round4, tableaux, out);
}

// Format (:22-48) of every kept record of a traced batch and of the final tableau of every LP
// that ended (PrimalSimplexSolver.cs:118-122, :133), read where the batch keeps them
int lpr_batch_trace_text(lpr_batch* b, int64_t* first_block, lpr_text** out) {
    static const char* W = "lpr_batch_trace_text";
    const std::vector<BatchDesc>* desc = nullptr;
    const double* slab = nullptr;
    lpr_engine* e = batch_view(b, &desc, &slab);
    if (!b || !e) {
        set_error("%s: batch handle is null or orphaned: its engine has been closed", W);
        return LPR_BAD_ARGUMENT;
    }
    if (!out) {
        set_error("%s: null out", W);
        return LPR_BAD_ARGUMENT;
    }
    *out = nullptr;
    const double* trace = nullptr;
    const std::vector<int64_t>* off = nullptr;
    const int32_t cap = batch_trace_view(b, &trace, &off);
    if (cap < 1) {
        set_error("%s: the batch is not traced (call lpr_batch_trace_reserve before the first "
                  "solve)", W);
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipSetDevice(e->device));
    std::vector<TextBlock> blk;
    try {
        for (size_t k = 0; k < desc->size(); ++k) {
            const BatchDesc& d = (*desc)[k];
            if (first_block) first_block[k] = (int64_t)blk.size();
            const int64_t kept = std::min<int64_t>(1 + d.iter, cap);
            const int64_t stride = batch_trace_stride(d.rows, d.cols);
            TextBlock tb{};
            tb.rows = d.rows;
            tb.cols = d.cols;
            tb.nvars = d.n;
            for (int64_t i = 0; i < kept; ++i) {
                tb.src = trace + (*off)[k] + i * stride + batch_trace_tab();
                blk.push_back(tb);
            }
            if (d.status == LPR_OK_OPTIMAL || d.status == LPR_UNBOUNDED) {
                tb.src = slab + d.t_off;
                blk.push_back(tb);
            }
        }
    } catch (...) {
        return text_oom("block descriptors (host)", (int64_t)blk.size());
    }
    if (first_block) first_block[desc->size()] = (int64_t)blk.size();
    TextWork wk;
    return text_format(W, e, blk, wk, out);
}

int lpr_text_info(lpr_text* t, int64_t* blocks, int64_t* bytes, double* kernel_ms) {
    LPR_LIVE_HANDLE(t, "text");
    if (blocks) *blocks = t->blocks;
    if (bytes) *bytes = t->bytes;
    if (kernel_ms) *kernel_ms = t->kernel_ms;
    return LPR_OK_OPTIMAL;
}

int lpr_text_offsets_read(lpr_text* t, int64_t* offsets) {
    LPR_LIVE_HANDLE(t, "text");
    if (!offsets) {
        set_error("lpr_text_offsets_read: null offsets");
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipMemcpyAsync(offsets, t->offsets, (size_t)(t->blocks + 1) * sizeof(int64_t),
                           hipMemcpyDeviceToHost, t->eng->stream));
    LPR_HIP(hipStreamSynchronize(t->eng->stream));
    return LPR_OK_OPTIMAL;
}

int lpr_text_read(lpr_text* t, int64_t first_byte, int64_t n, uint8_t* out) {
    LPR_LIVE_HANDLE(t, "text");
    if (first_byte < 0 || n < 0 || first_byte > t->bytes || n > t->bytes - first_byte) {
        set_error("lpr_text_read: bytes [%lld, %lld + %lld) of a text of %lld bytes",
                  (long long)first_byte, (long long)first_byte, (long long)n, (long long)t->bytes);
        return LPR_BAD_ARGUMENT;
    }
    if (n == 0) return LPR_OK_OPTIMAL;
    if (!out) {
        set_error("lpr_text_read: null output");
        return LPR_BAD_ARGUMENT;
    }
    LPR_HIP(hipMemcpyAsync(out, t->text + first_byte, (size_t)n, hipMemcpyDeviceToHost,
                           t->eng->stream));
    LPR_HIP(hipStreamSynchronize(t->eng->stream));
    return LPR_OK_OPTIMAL;
}

int lpr_text_destroy(lpr_text* t) {
    if (!t) return LPR_BAD_ARGUMENT;
    if (t->eng) {
        hipSetDevice(t->eng->device);
        hipStreamSynchronize(t->eng->stream);
        text_release_device(t);
        unlist(t->eng->live_text, t);
    }
    delete t;
    return LPR_OK_OPTIMAL;
}

}  // extern "C"
