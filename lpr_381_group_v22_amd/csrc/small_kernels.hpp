// small_kernels.hpp -- host interface of the cache-resident primal path (small_kernels.hip), called
// by lpr_engine.hip.  Which tableaux fit: small_fits of primal_plan.hpp.
#pragma once

#include "engine_common.hpp"

namespace lpr {

void small_release(lpr_tableau* t);
int small_ensure(lpr_tableau* t);
int small_upload_state(lpr_tableau* t, int64_t iter, int64_t max_iter);
int small_set_log_cap(lpr_tableau* t);
void small_launch_block(lpr_tableau* t);
int small_poll(lpr_tableau* t, int32_t* status, int64_t* iter);

}  // namespace lpr
