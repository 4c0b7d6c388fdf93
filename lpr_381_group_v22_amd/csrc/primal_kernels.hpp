// primal_kernels.hpp -- host launchers of primal_kernels.hip (one-pivot and fused paths, tableau
// construction), called by lpr_engine.hip.
#pragma once

#include "engine_common.hpp"

namespace lpr {

enum : int { kSelEnter = 1, kSelLeave = 2, kSelCommit = 4, kSelFull = 7 };  // launch_select modes

void launch_select(lpr_tableau* t, int mode, int e_in, int r_in, int32_t* out_i);
void launch_bootstrap(lpr_tableau* t);
void launch_pivot_head(lpr_tableau* t);
// variant: low byte selects the tile shape, bit 8 turns the serpentine sweep on
void launch_update(lpr_tableau* t, int variant, int check_status, int dump_next);
void launch_extract(lpr_tableau* t, int n, double* x);
void launch_pivot_fused(lpr_tableau* t, const double* in, double* out);
void launch_build(lpr_tableau* t, int n, int m, const double* d_obj, const double* d_A, int lda,
                  const int32_t* d_ncoef, const int8_t* d_rel, const double* d_rhs, int is_max);
void launch_synthetic(lpr_tableau* t, int m, int n, uint64_t seed);

}  // namespace lpr
