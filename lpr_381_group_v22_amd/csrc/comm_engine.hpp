// comm_engine.hpp -- what the distributed Branch & Bound (bb_engine.hip) asks of a communicator
// (comm_engine.hip).
#pragma once

#include "engine_common.hpp"

namespace lpr {

int comm_rank(const lpr_comm* c);
int comm_world(const lpr_comm* c);
int comm_all_reduce_max(lpr_comm* c, double* v, int n);
int comm_all_gather(lpr_comm* c, const void* send, void* recv, int bytes);

}  // namespace lpr
