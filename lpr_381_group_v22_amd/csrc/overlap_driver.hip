// overlap_driver.hip -- host driver of the K-pivot primal path (kernels and launchers:
// overlap_kernels.hip; which calls come here: primal_plan.hpp).  No device code in this file.
#include "overlap.hpp"

#include <cmath>
#include <cstdlib>

namespace lpr {

// Device work queued behind a mid-call snapshot of the K-pivot driver, in microseconds.  At the
// headline size (a step is 161 us by the driver's estimate) ONE step behind the snapshot already
// leaves no idle stretch at a batch boundary in a kernel trace (profiles/r07_poll_gaps_lead1.json);
// the value kept is twice that.
static constexpr double kOvLeadUs = 320.0;

// Tableaux above kFusedBytes that do not fit the cache-resident path: K pivots per sweep --
// overlap_kernels.hip.  Two streams (PrimalPath::TwoStream): the next block's loop heads run on a stream of their own
// beside the current block's out-of-place sweep; otherwise (InPlace) the heads of a block, then its
// sweep in place, both on the engine stream.
//
// A "step" is one launch pair.  Two streams: step j sweeps block j (K pivots) while its heads decide
// block j + 1, so a call that applies N blocks takes N + 1 steps (the first only decides, the last
// only sweeps).  In place: step j decides block j and sweeps it.  The host learns the outcome from
// the control block the last step wrote: `status`, or -- when the heads found the end (`pending`)
// and left nothing staged (`kdone == 0`) -- `pending` itself, so no further launch is needed to
// publish it.
// opts.time_kernels: HIP events on the sweep's own stream bracket EVERY sweep launch (start =
// both kernels of the previous step done); sweep time = stop - start, step time = start of the
// next step - start of this one.  Only steps that swept a full block are counted.
//
// Polling ahead.  The host does not wait for the queue to run dry before it learns the state: in a
// batch of nb steps a SNAPSHOT of the control block (ov2_launch_step / ov_snapshot: one copy into a
// pinned slot and an event) is queued `lead` steps before the end, the host waits for that event
// alone and, while the device works through the last `lead` steps, queues the next batch behind
// them -- no join, no stream synchronisation, no idle device.  A snapshot is `lead` steps stale when
// the next batch is sized, so the driver assumes that every step queued so far applied a full
// block: exact unless a step met the end of the solve, and then the steps queued for nothing return
// at once, as idle steps always have (at most `lead` of them when the snapshot itself shows the end,
// one more batch when the end falls in the `lead` steps behind a snapshot).  With a pivot limit the
// bound is exact, so a call queues ceil(max_pivots / K) + 1 steps whatever the batch length.  Once a
// snapshot shows anything but a running solve -- the end found, an error -- and whenever the log has
// to grow, the driver DRAINS (join, synchronous ov_poll) and carries on from the exact state the
// way it always did, one step at a time while an end is pending.  What a call returns (z, the live
// buffer, the sweep direction for the next call) comes from that final poll only.
struct OvTimedBatch {  // a queued batch whose timing events have not been read yet
    bool live = false;
    bool own_close = false;  // its last window closes at its own event 2 * nb (else: at the first
                             // start event of the batch queued behind it, in the other event set)
    int nb = 0;
    int64_t g0 = 0;          // index of its first step in the call
};

static int solve_overlapped(lpr_tableau* t, const lpr_solve_opts& o, const PrimalPlan& plan,
                            lpr_solve_result* res) {
    lpr_engine* e = t->eng;
    hipStream_t s = e->stream;
    const int K = plan.K, tr = plan.tile;
    const bool two_streams = plan.path == PrimalPath::TwoStream;
    int rc = ov_ensure(t, two_streams);
    if (rc != LPR_OK_OPTIMAL) return rc;
    const bool timed = o.time_kernels != 0;
    // opts.time_kernels = n > 1: events around every n-th step only (two event records per step
    // cost the two-stream pipeline ~3 % -- they sit on the sweep's stream, on the critical cycle)
    const int tstride = o.time_kernels > 1 ? (o.time_kernels < 16 ? o.time_kernels : 16) : 1;
    // steps between snapshots: about 5 ms of device work (a step = one sweep at ~5 TB/s, or K loop
    // heads at ~8 us, whichever is longer)
    const double sweep_us = 16.0 * t->rows * (double)t->ld / 5.0e6;
    const double step_us = sweep_us > 8.0 * K ? sweep_us : 8.0 * K;
    int nlaunch;
    if (o.batch > 0) {
        nlaunch = (o.batch + K - 1) / K;
    } else {
        nlaunch = (int)(5000.0 / step_us);
        if (nlaunch > 64) nlaunch = 64;
    }
    if (nlaunch < 2) nlaunch = 2;
    // steps queued behind a snapshot: kOvLeadUs of device work by the same estimate (DESIGN 4b
    // "Control": where the figure comes from), at least 1, at most half the batch
    const int lead_steps = t->poll_lead > 0 ? t->poll_lead : (int)std::ceil(kOvLeadUs / step_us);
    const bool ahead = plan.poll_ahead;
    const bool poll_flags = plan.form.sweep_on_device;
    const int64_t start_iter = t->total_pivots;
    const int64_t max_iter = o.max_pivots > 0 ? start_iter + o.max_pivots : 0;
    rc = ov_begin(t, start_iter, max_iter);
    if (rc != LPR_OK_OPTIMAL) return rc;
    if (two_streams) {
        rc = ov2_begin(t);
        if (rc != LPR_OK_OPTIMAL) return rc;
    }

    OvPoll pl;
    pl.status = kRunning;
    pl.pending = kRunning;
    pl.applied = start_iter;
    int32_t status = kRunning;
    int64_t applied = start_iter;  // pivots applied at the latest poll or snapshot
    int64_t step = 0;              // launches (pairs) queued by this call; parity = control block
    int idle_batches = 0;
    bool exact = true;   // `pl` is a synchronous poll and nothing has been queued since
    int64_t nbatch = 0;  // batches queued; parity = event set and snapshot slot
    OvTimedBatch tb[2];  // by event set
    int last_set = -1;   // event set of the batch queued last
    const int first_full = two_streams ? 1 : 0;  // the first step of a two-stream call sweeps nothing
    const int evset = 2 * nlaunch + 1;           // events per set: (start, stop) per step + closing

    // Reads the events of batch `b`.  Steps sweep full blocks in order: first (two streams) the step
    // that sweeps nothing, then full blocks, then at most one partial block and idle steps -- so the
    // sampled steps that count are those with a call-wide index in [first_full, full_end).
    auto read_events = [&](int b, int64_t full_end) -> int {
        OvTimedBatch& B = tb[b];
        hipEvent_t* ev = t->ev.data() + (size_t)b * evset;
        hipEvent_t close = B.own_close ? ev[2 * B.nb] : t->ev[(size_t)(b ^ 1) * evset];
        for (int k = 0; k < B.nb && B.g0 + k < full_end; k += tstride) {
            if (B.g0 + k < first_full) continue;  // (the sampled steps are the multiples of tstride)
            float ms = 0.f;
            LPR_HIP(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
            t->timed_total_ms += ms;
            t->timed_launches += 1;
            // start of this step to the start of the next SAMPLED one (or the closing event):
            // that many steps, all of them full as long as they lie before full_end
            const int kn = (k + tstride < B.nb) ? k + tstride : B.nb;
            if (B.g0 + kn <= full_end) {
                float st = 0.f;
                LPR_HIP(hipEventElapsedTime(&st, ev[2 * k], kn < B.nb ? ev[2 * kn] : close));
                t->timed_step_ms += st;
                t->timed_steps += kn - k;
            }
        }
        B.live = false;
        return LPR_OK_OPTIMAL;
    };

    // The synchronous poll: both streams joined, the control block and z read back, the events of
    // every batch still pending read against the exact count of full blocks.
    auto drain = [&]() -> int {
        if (two_streams) {
            int jr = ov2_join(t);
            if (jr != LPR_OK_OPTIMAL) return jr;
        }
        if (timed && last_set >= 0 && tb[last_set].live && !tb[last_set].own_close) {
            // closes the last step's window
            LPR_HIP(hipEventRecord(t->ev[(size_t)last_set * evset + 2 * tb[last_set].nb], s));
            tb[last_set].own_close = true;
        }
        LPR_HIP(hipGetLastError());
        int pr = ov_poll(t, two_streams ? (int)(step & 1) : 0, poll_flags, &pl);
        if (pr != LPR_OK_OPTIMAL) return pr;
        if (pl.error || pl.status == LPR_DEVICE_ERROR) {
            // the staging state is unusable (a head group never arrived): the handle is poisoned
            t->poisoned = true;
            set_error("overlapped pivot loop: a hand-off between the loop heads timed out; the "
                      "tableau handle is no longer usable");
            return LPR_DEVICE_ERROR;
        }
        status = pl.status;
        if (status == kRunning && pl.pending != kRunning && pl.kdone == 0)
            status = pl.pending;  // the end was found and nothing is left to sweep
        if (timed && last_set >= 0) {
            const int64_t full_end = first_full + (pl.applied - start_iter) / K;
            for (int b : {last_set ^ 1, last_set})  // the older batch first
                if (tb[b].live) {
                    int er = read_events(b, full_end);
                    if (er != LPR_OK_OPTIMAL) return er;
                }
        }
        idle_batches = (pl.applied == applied) ? idle_batches + 1 : 0;
        applied = pl.applied;
        exact = true;
        if (status == kRunning && idle_batches >= 3) {
            set_error("overlapped pivot loop made no progress (device status still running)");
            return LPR_DEVICE_ERROR;
        }
        return LPR_OK_OPTIMAL;
    };

    while (status == kRunning) {
        // pivots applied once everything queued so far has run, if no step has met the end
        int64_t base = applied;
        if (!exact) {
            base = start_iter + (step - first_full) * K;
            if (max_iter > 0 && base > max_iter) base = max_iter;
        }
        int nb = nlaunch;
        bool to_limit = false;  // this batch takes the call to its pivot limit
        if (exact && pl.pending != kRunning) {
            nb = 1;  // the end has been found: the staged tail is swept, the outcome published
        } else if (max_iter > 0) {  // the blocks the limit allows (+ the step that only decides)
            const int64_t left = max_iter - base;
            const int64_t need = (left + K - 1) / K + (step == 0 ? 1 : 0);
            if (need <= nb) {
                nb = (int)need;
                to_limit = true;
            }
        }
        if (nb < 1) nb = 1;
        if (base + (int64_t)(nb + 1) * K + 1 > t->log_cap) {
            if (!exact) {
                // The heads write B.log from their own stream: the old buffer must be out of use
                // before it is replaced.  Drain, then size the batch again from the exact state.
                rc = drain();
                if (rc != LPR_OK_OPTIMAL) return rc;
                continue;
            }
            const int64_t log_before = t->log_cap;
            const int32_t* log_ptr = t->log;
            rc = ensure_log(t, base + (int64_t)(nb + 1) * K + 1);
            if (rc != LPR_OK_OPTIMAL) return rc;
            if (t->log_cap != log_before || t->log != log_ptr) {
                rc = ov_set_log(t, two_streams ? (int)(step & 1) : 0);
                if (rc != LPR_OK_OPTIMAL) return rc;
            }
        }
        // A snapshot `lead` steps before the end of the batch -- unless the batch is known to be
        // the call's last (it reaches the pivot limit, or an end is pending): the drain follows.
        int lead = 0;
        if (ahead && !to_limit && nb >= 2 && !(exact && pl.pending != kRunning)) {
            lead = lead_steps < nb / 2 ? lead_steps : nb / 2;
            if (lead < 1) lead = 1;
        }
        const int set = (int)(nbatch & 1);
        // One or two launches per K pivots: plain launches keep the device busy (measured: a
        // captured graph is no faster here, and capturing one costs milliseconds per solve call).
        hipEvent_t* ev = nullptr;
        if (timed) {  // (two sets, sized for full batches at once: creating an event costs ~10 us)
            while ((int)t->ev.size() < 2 * evset) {
                hipEvent_t x;
                LPR_HIP(hipEventCreate(&x));
                t->ev.push_back(x);
            }
            ev = t->ev.data() + (size_t)set * evset;
            tb[set].live = true;
            tb[set].own_close = false;
            tb[set].nb = nb;
            tb[set].g0 = step;
        }
        for (int k = 0; k < nb; ++k, ++step) {
            const int lp = (int)(step & 1);
            const bool tk = timed && (k % tstride == 0);
            const bool snap = lead > 0 && k == nb - lead;
            if (two_streams) {
                rc = ov2_launch_step(t, K, tr, lp, plan.form, tk ? ev[2 * k] : nullptr,
                                     tk ? ev[2 * k + 1] : nullptr, snap ? set : -1);
                if (rc != LPR_OK_OPTIMAL) return rc;
                continue;
            }
            if (snap) {
                rc = ov_snapshot(t, set);
                if (rc != LPR_OK_OPTIMAL) return rc;
            }
            ov_launch_heads(t, K, plan.form);
            if (tk) LPR_HIP(hipEventRecord(ev[2 * k], s));
            ov_launch_sweep(t, tr);
            if (tk) LPR_HIP(hipEventRecord(ev[2 * k + 1], s));
        }
        last_set = set;
        nbatch += 1;
        exact = false;
        if (lead > 0) {
            LPR_HIP(hipGetLastError());
            OvPoll sp;
            rc = ov_snapshot_wait(t, set, &sp);
            if (rc != LPR_OK_OPTIMAL) return rc;
            idle_batches = (sp.applied == applied) ? idle_batches + 1 : 0;
            if (sp.status == kRunning && sp.pending == kRunning && !sp.error && idle_batches < 3) {
                applied = sp.applied;
                // The batch before this one is complete (its last step precedes the snapshot on
                // the engine stream, and so does the start event that closes its last window) and
                // every step of it came before a snapshot that shows no end: all its blocks were
                // full.  hipEventQuery confirms; if it ever did not, the drain below would wait.
                if (!timed || !tb[set ^ 1].live) continue;
                const hipError_t q = hipEventQuery(ev[0]);
                if (q == hipSuccess) {
                    rc = read_events(set ^ 1, INT64_MAX);
                    if (rc != LPR_OK_OPTIMAL) return rc;
                    continue;
                }
                if (q != hipErrorNotReady) LPR_HIP(q);
                (void)hipGetLastError();
            }
        }
        rc = drain();
        if (rc != LPR_OK_OPTIMAL) return rc;
    }
    ov_adopt_buffer(t, pl.cur);
    // z = T[0, cols-1]: the RHS column the heads carry, entry 0
    return finish_call(t, res, status, applied, start_iter, K, &pl.z[applied & 1]);
}

// The value of the test hook LPR_TEST_OV_SPARES (1..4096 spare columns of the condensed layout; 0:
// not set): a small number, so that a short oracle-checked solve re-condenses every few pivots
// (tests/test_condensed_gpu.py).  The rule it overrides: ovc_spares of primal_plan.hpp.
int ovc_spares_hook() {
    if (const char* sp = std::getenv("LPR_TEST_OV_SPARES")) {
        const long v = std::strtol(sp, nullptr, 10);
        if (v >= 1 && v <= 4096) return (int)v;
    }
    return 0;
}

// The two-stream path on the condensed working layout (DESIGN 4b "Condensed layout"): for the
// length of a call the kernels work on buffers that leave out the columns basic when it began --
// exact unit columns that no pivot changes -- so a sweep moves (n + S + 1) / (n + m + 1) of the
// bytes.  Which calls are eligible: PrimalPlan::condensed.
static int solve_condensed(lpr_tableau* t, const lpr_solve_opts& o, const PrimalPlan& plan,
                           lpr_solve_result* res) {
    const int64_t first = t->total_pivots;
    lpr_solve_opts oc = o;
    for (;;) {
        const int64_t done = t->total_pivots - first;
        if (o.max_pivots > 0) oc.max_pivots = o.max_pivots - done;
        bool ok = false;
        int rc = ovc_ensure(t, plan.spares);
        if (rc == LPR_OK_OPTIMAL) rc = ovc_condense(t, &ok);
        if (rc != LPR_OK_OPTIMAL && rc != LPR_OUT_OF_MEMORY) return rc;
        int status;
        if (rc != LPR_OK_OPTIMAL || !ok) {
            // a basic column is not the exact unit column (or there is no room): the full layout
            status = solve_overlapped(t, oc, plan, res);
        } else {
            ovc_enter(t);
            status = solve_overlapped(t, oc, plan, res);
            ovc_leave(t);
            if (status == LPR_DEVICE_ERROR || status == LPR_OUT_OF_MEMORY ||
                status == LPR_BAD_ARGUMENT)
                return status;
            rc = ovc_expand(t);
            if (rc != LPR_OK_OPTIMAL) return rc;
            if (status == kOvLeaveSpares) continue;
            if (status == kOvLeaveNonFinite) {
                if (o.max_pivots > 0) oc.max_pivots = o.max_pivots - (t->total_pivots - first);
                status = solve_overlapped(t, oc, plan, res);
            }
        }
        res->pivots = t->total_pivots - first;
        return status;
    }
}

// The run-time half of the plan: what can fail is expressed on its fields, then it is dispatched.
int solve_kpivot(lpr_tableau* t, const lpr_solve_opts& o, PrimalPlan plan, lpr_solve_result* res) {
    // the second tableau buffer or the heads' stream cannot be had: heads-then-sweep in place
    if (plan.path == PrimalPath::TwoStream && ov_ensure(t, true) != LPR_OK_OPTIMAL)
        plan.path = PrimalPath::InPlace;
    if (plan.path != PrimalPath::TwoStream) return solve_overlapped(t, o, plan, res);
    if (plan.condensed_buffers) {  // (out of memory: solve_condensed meets it again and falls back)
        const int er = ovc_ensure(t, plan.spares);
        if (er != LPR_OK_OPTIMAL && er != LPR_OUT_OF_MEMORY) return er;
    }
    return plan.condensed ? solve_condensed(t, o, plan, res) : solve_overlapped(t, o, plan, res);
}

}  // namespace lpr
