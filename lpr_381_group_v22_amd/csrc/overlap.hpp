// overlap.hpp -- host interface of the K-pivot primal path: the launchers and contexts of
// overlap_kernels.hip and the driver loop of overlap_driver.hip.  Both include it, so a definition
// that drifts from its declaration does not compile.
#pragma once

#include "engine_common.hpp"

namespace lpr {

// ---- overlap_kernels.hip ---------------------------------------------------------------------------
struct OvPoll {
    int32_t status, pending, kdone, cur, error;
    int64_t applied;
    double z[2];  // RHS column entry 0 (= T[0, cols-1]) after an even / odd number of pivots
};
void ov_release(lpr_tableau* t);
int ov_ensure(lpr_tableau* t, bool second_buffer);
int ov_begin(lpr_tableau* t, int64_t iter, int64_t max_iter);
int ov_set_log(lpr_tableau* t, int parity);
void ov_launch_heads(lpr_tableau* t, int K, const OvForm& f);
void ov_launch_sweep(lpr_tableau* t, int tr);
int ov2_begin(lpr_tableau* t);
int ov2_launch_step(lpr_tableau* t, int K, int tr, int lp, const OvForm& f, hipEvent_t ev_start,
                    hipEvent_t ev_stop, int snap_slot);
int ov2_join(lpr_tableau* t);
int ov_snapshot(lpr_tableau* t, int slot);
int ov_snapshot_wait(lpr_tableau* t, int slot, OvPoll* out);
int ov_poll(lpr_tableau* t, int parity, bool with_flags, OvPoll* out);
int ov_read_stamps(lpr_tableau* t, uint64_t* out, int64_t cap, int64_t* count);
void ov_adopt_buffer(lpr_tableau* t, int cur);
void ovc_release(lpr_tableau* t);
int ovc_ensure(lpr_tableau* t, int spares);
int ovc_condense(lpr_tableau* t, bool* ok);
void ovc_enter(lpr_tableau* t);
void ovc_leave(lpr_tableau* t);
int ovc_expand(lpr_tableau* t);

// ---- overlap_driver.hip ----------------------------------------------------------------------------
// the value of the test hook LPR_TEST_OV_SPARES for primal_plan (0: not set)
int ovc_spares_hook();
// A K-pivot plan (TwoStream or InPlace) on `t`: the run-time fallbacks, then the solve.
int solve_kpivot(lpr_tableau* t, const lpr_solve_opts& o, PrimalPlan plan, lpr_solve_result* res);

}  // namespace lpr
