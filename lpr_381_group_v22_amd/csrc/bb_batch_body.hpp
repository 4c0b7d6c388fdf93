// bb_batch_body.hpp -- the one text of the batched Branch & Bound search (DESIGN.md sections 13
// and 23): bb_batch_body<NT, kLds, kNarr> is the body of k_bb_batch (bb_batch_kernels.hip,
// kNarr = false) and of k_bb_batch_narr (bb_batch_narr_kernels.hip, kNarr = true).  With kNarr the
// search also writes what ExecuteBranchAndBound's console text needs (bb_narr_layout.hpp): every
// tableau of every child LP, the score of every pop, the incumbent's tableau.  Those are second
// stores of the lane that computes the value; no lane reads a record, so narration adds no fence
// and no barrier, and the LDS use of a form is that of its un-narrated twin.
#pragma once

#include "batch_device.hpp"
#include "bb_batch_common.hpp"
#include "bb_device_round.hpp"

#pragma clang fp contract(off)

namespace lpr {

namespace {

// Ordering between the lanes of one IP is group_sync<NT, kFenceWorkgroup>() throughout: the DFS
// stack they share is in global memory, so form W fences at workgroup scope.

// Minimum of an int over the NT lanes of one IP; every lane gets it.
template <int NT>
__device__ __forceinline__ int ip_min_int(int v, int* red_i) {
    v = dpp_imin<0xB1, 0xf>(v);
    v = dpp_imin<0x4E, 0xf>(v);
    v = dpp_imin<0x141, 0xf>(v);
    v = dpp_imin<0x140, 0xf>(v);
    v = dpp_imin<0x142, 0xa>(v);
    v = dpp_imin<0x143, 0xc>(v);
    v = __builtin_amdgcn_readlane(v, 63);
    if constexpr (NT == kWave) {
        return v;
    } else {
        const int lane = threadIdx.x & (kWave - 1);
        const int wave = threadIdx.x / kWave;
        __syncthreads();  // protect the slots against the previous use
        if (lane == 0) red_i[wave] = v;
        __syncthreads();
        int r = red_i[0];
        for (int w = 1; w < NT / kWave; ++w) r = min(r, red_i[w]);
        return r;
    }
}

template <int NT>
__device__ __forceinline__ bool ip_any(bool p, int* red_i) {
    return ip_min_int<NT>(p ? 0 : 1, red_i) == 0;
}

// The child-tableau cursors of one IP while a launch runs (kNarr): the descriptor's, held by every
// lane alike, and the slice they address.  Empty where kNarr is false.
struct NarrCursor {
    BBNarrDesc c;
    double* slice;
    // One more tableau of n doubles: where its record goes, or nullptr where it is only counted.
    __device__ __forceinline__ double* push(int64_t n) {
        const int64_t at = kept_push(c.kp, n);
        return at < 0 ? nullptr : slice + at;
    }
};

// The pivot of PerformDualPivot :174-190 / PerformPrimalPivot :257-271, out of place (cur -> out):
// the pivot row divided, then `v == 0.0 ? 0.0`; every other row T - f * p with the product rounded
// (no FMA) and no row skipped for a zero factor.  Every entry written also gets DoDualSimplex's
// -0 -> +0 (:307-313, at the head of both loops, which is then a no-op on what the pivot wrote).
// kNarr: the lane that computes an entry also stores it to the record `rec` (nullptr: not kept).
template <int NT, bool kNarr>
__device__ __forceinline__ void ip_pivot(const double* cur, double* out, double* fcol, int Rc,
                                         int Cc, int pr, int pc, int lane, double* rec) {
    const double p = cur[(size_t)pr * Cc + pc];
    for (int i = lane; i < Rc; i += NT) fcol[i] = cur[(size_t)i * Cc + pc];
    double* const orow = out + (size_t)pr * Cc;
    const double* const crow = cur + (size_t)pr * Cc;
    for (int j = lane; j < Cc; j += NT) {
        double v = ieee_div(crow[j], p);
        if (v == 0.0) v = 0.0;
        orow[j] = v;
        if constexpr (kNarr)
            if (rec) rec[(size_t)pr * Cc + j] = v;
    }
    group_sync<NT, kFenceWorkgroup>();
    for_each_ij<NT>(Rc, Cc, lane, [&](int x, int i, int j) {
        if (i == pr) return;
        const double prod = fcol[i] * orow[j];
        double v = cur[x] - prod;
        if (v == 0.0) v = 0.0;
        out[x] = v;
        if constexpr (kNarr)
            if (rec) rec[x] = v;
    });
    group_sync<NT, kFenceWorkgroup>();
}

// Results of one child LP.
enum : int { kChildSolved = 0, kChildInfeasible = 1, kChildFailed = 2, kChildLimit = 3 };

struct Trace {
    int32_t* q;     // quads (record id, phase, row, col)
    int cap;
    int64_t n;      // exact count
};

__device__ __forceinline__ void trace_push(Trace& t, int lane, int rid, int phase, int row,
                                           int col) {
    if (lane == 0 && t.n < t.cap) {
        int32_t* e = t.q + 4 * t.n;
        e[0] = rid;
        e[1] = phase;
        e[2] = row;
        e[3] = col;
    }
    ++t.n;
}

// AddConstraint :694-803 of ONE branching row (x_var <= bound, or >= bound when `reverse`) on the
// popped node P (Rn x Cn, already rounded by the pop) into A ((Rn + 1) x (Cn + 1)), with the
// oracle's repeated roundings (:702, :747, :799) taken as they are.  keys / list: Cn ints each.
// kNarr: the last pass, which produces the final value of every entry, also stores it to `rec`.
template <int NT, bool kNarr>
__device__ void add_constraint(const double* P, int Rn, int Cn, int nv, int var, double bound,
                               bool reverse, double* A, int32_t* keys, int32_t* list, int lane,
                               int* red_i, double* rec) {
    const int Rc = Rn + 1, Cc = Cn + 1;
    // IdentifyBasicVariables :642-663 on working = RoundTableau(P): each column's sum of rounded
    // entries in row order, and the row of its first 1.0
    for (int k = lane; k < Cn; k += NT) {
        double sum = 0;
        int key = Rn;
        for (int i = 0; i < Rn; ++i) {
            const double w = dn_round4(dn_round4(P[(size_t)i * Cn + k]));
            sum += w;
            if (key == Rn && w == 1.0) key = i;
        }
        sum = dn_round4(sum);
        keys[k] = (fabs(sum - 1.0) <= kBBEps) ? key : -1;
    }
    // the rows of the parent, with the slack column inserted before the RHS (:716-719), rounded
    // three times (:702, :747, :799); the new row (:721-744) rounded twice (its own Math.Round
    // and :747); the final rounding of the new row waits for the elimination
    for_each_ij<NT>(Rc, Cc, lane, [&](int x, int i, int j) {
        double v;
        if (i < Rn) {
            const double s = (j < Cn - 1) ? P[(size_t)i * Cn + j]
                                          : (j == Cn - 1 ? 0.0 : P[(size_t)i * Cn + (Cn - 1)]);
            v = dn_round4(dn_round4(dn_round4(s)));
        } else if (j < nv) {
            v = dn_round4(dn_round4(j == var ? 1.0 : 0.0));
        } else if (j == Cn) {
            v = dn_round4(dn_round4(bound));
        } else if (j == Cn - 1) {
            v = dn_round4(reverse ? -1.0 : 1.0);
        } else {
            v = dn_round4(0.0);
        }
        A[x] = v;
    });
    group_sync<NT, kFenceWorkgroup>();
    // OrderBy(key), a stable sort: the basic columns by (key, column)
    int nb = 0;
    for (int k = 0; k < Cn; ++k) nb += keys[k] >= 0;
    for (int k = lane; k < Cn; k += NT) {
        const int kk = keys[k];
        if (kk < 0) continue;
        int pos = 0;
        for (int k2 = 0; k2 < Cn; ++k2) {
            const int o = keys[k2];
            pos += (o >= 0) && (o < kk || (o == kk && k2 < k));
        }
        list[pos] = k;
    }
    group_sync<NT, kFenceWorkgroup>();
    // the sequential eliminations :756-796, every step parallel over the columns
    double* const crow = A + (size_t)Rn * Cc;
    for (int q = 0; q < nb; ++q) {
        const int colIndex = list[q];
        const double coefficient = dn_round4(crow[colIndex]);
        if (!(fabs(coefficient) > kBBEps)) continue;
        int first = INT_MAX;
        for (int i = lane; i < Rn; i += NT)
            if (fabs(A[(size_t)i * Cc + colIndex] - 1.0) <= kBBEps) {
                first = i;
                break;
            }
        const int pivotRow = ip_min_int<NT>(first, red_i);
        if (pivotRow == INT_MAX) continue;
        const double* const prow = A + (size_t)pivotRow * Cc;
        for (int c = lane; c < Cc; c += NT) {
            const double pivotVal = prow[c];
            const double constraintVal = dn_round4(crow[c]);
            double prod, newVal;
            if (reverse) {
                prod = coefficient * constraintVal;
                newVal = pivotVal - prod;
            } else {
                prod = coefficient * pivotVal;
                newVal = constraintVal - prod;
            }
            crow[c] = dn_round4(newVal);
        }
        group_sync<NT, kFenceWorkgroup>();
    }
    // RoundTableau :799 of the new row, and the -0 -> +0 of the first DoDualSimplex loop head
    for_each_ij<NT>(Rc, Cc, lane, [&](int x, int i, int j) {
        double v = A[x];
        if (i == Rn) v = dn_round4(v);
        if (v == 0.0) v = 0.0;
        A[x] = v;
        if constexpr (kNarr)
            if (rec) rec[x] = v;
    });
    group_sync<NT, kFenceWorkgroup>();
}

// DoDualSimplex :289-468 in tableauOverride mode on the child in *cur (Rc x Cc), ping-ponging with
// *oth: the tableau before the last pivot is always the other buffer.  On kChildSolved *cur holds
// the last tableau.  kNarr: every pivot's tableau goes to the next record of `nc`, and the drop of
// :392-400 steps the cursor back.
template <int NT, bool kNarr>
__device__ int child_lp(double*& cur, double*& oth, double* fcol, int Rc, int Cc, int rid,
                        int max_piv, Trace& tr, NarrCursor& nc, int lane, double* red_v,
                        int* red_i) {
    int npiv = 0;
    const int64_t tab_n = (int64_t)Rc * Cc;
    // dual phase :305-343
    for (;;) {
        bool bad = false;
        Cand c;
        c.v = 0.0;
        c.i = -1;
        for (int i = lane; i < Rc; i += NT) {
            const double x = cur[(size_t)i * Cc + (Cc - 1)];
            if (!(x >= -1e-9)) bad = true;
            if (x < 0 && (c.i < 0 || x < c.v)) {  // Min over the negatives, then IndexOf
                c.v = x;
                c.i = i;
            }
        }
        if (!ip_any<NT>(bad, red_i)) break;
        c = group_cand_min<NT>(c, red_v, red_i);
        if (c.i < 0) return kChildInfeasible;  // PerformDualPivot :118-123 -> null optimum
        const int pr = c.i;
        // :126-154: theta = |T0j / Tprj| over Tprj < 0, else +inf; all 0-or-inf -> 0, else the
        // minimum over theta > 0; IndexOf the first equal
        const double* const r0 = cur;
        const double* const rp = cur + (size_t)pr * Cc;
        bool other = false;
        int first0 = INT_MAX;
        Cand m;
        m.v = 0.0;
        m.i = -1;
        for (int j = lane; j < Cc - 1; j += NT) {
            const double a = rp[j];
            const double th = (a < 0) ? fabs(ieee_div(r0[j], a)) : INFINITY;
            if (!(th == 0 || th == INFINITY)) other = true;
            if (th == 0 && j < first0) first0 = j;
            if (th > 0 && (m.i < 0 || th < m.v)) {
                m.v = th;
                m.i = j;
            }
        }
        const bool any_other = ip_any<NT>(other, red_i);
        int pc;
        if (!any_other) {
            pc = ip_min_int<NT>(first0, red_i);
            if (pc == INT_MAX) pc = -1;
        } else {
            pc = group_cand_min<NT>(m, red_v, red_i).i;  // no theta > 0: minPos = +inf, none equal
        }
        if (pc < 0) return kChildInfeasible;  // tableau[rowIndex][-1] -> (tableau, null) :165-172
        if (npiv >= max_piv) return kChildLimit;
        double* rec = nullptr;
        if constexpr (kNarr) rec = nc.push(tab_n);
        ip_pivot<NT, kNarr>(cur, oth, fcol, Rc, Cc, pr, pc, lane, rec);
        trace_push(tr, lane, rid, 0, pr, pc);
        double* t = cur;
        cur = oth;
        oth = t;
        ++npiv;
    }
    // :345-348
    bool neg = false;
    for (int j = lane; j < Cc - 1; j += NT)
        if (!(cur[j] >= 0)) neg = true;
    if (!ip_any<NT>(neg, red_i)) return kChildSolved;
    // primal phase :352-390
    for (;;) {
        neg = false;
        Cand c;
        c.v = 0.0;
        c.i = -1;
        for (int j = lane; j < Cc - 1; j += NT) {
            const double x = cur[j];
            if (!(x >= 0)) neg = true;
            if (x < 0 && (c.i < 0 || x < c.v)) {
                c.v = x;
                c.i = j;
            }
        }
        if (!ip_any<NT>(neg, red_i)) break;
        c = group_cand_min<NT>(c, red_v, red_i);
        if (c.i < 0) break;  // Min() of nothing throws -> (null, null) -> break
        const int pc = c.i;
        // :221-249: theta_i = b_i / T_i,pc over T_i,pc != 0, else +inf
        bool notneg = false;
        int first0 = INT_MAX;
        Cand m;
        m.v = 0.0;
        m.i = -1;
        for (int i = 1 + lane; i < Rc; i += NT) {
            const double a = cur[(size_t)i * Cc + pc];
            const double th = (a != 0) ? ieee_div(cur[(size_t)i * Cc + (Cc - 1)], a) : INFINITY;
            if (!(th < 0)) notneg = true;
            if (th == 0 && i < first0) first0 = i;
            if (th > 0 && th != INFINITY && (m.i < 0 || th < m.v)) {
                m.v = th;
                m.i = i;
            }
        }
        if (!ip_any<NT>(notneg, red_i)) break;  // every theta < 0 (or none)
        m = group_cand_min<NT>(m, red_v, red_i);
        int pr = m.i;
        if (pr < 0) {
            pr = ip_min_int<NT>(first0, red_i);
            if (pr == INT_MAX) break;
        }
        if (cur[(size_t)pr * Cc + pc] == 0) break;  // :252
        if (npiv >= max_piv) return kChildLimit;
        double* rec = nullptr;
        if constexpr (kNarr) rec = nc.push(tab_n);
        ip_pivot<NT, kNarr>(cur, oth, fcol, Rc, Cc, pr, pc, lane, rec);
        trace_push(tr, lane, rid, 1, pr, pc);
        double* t = cur;
        cur = oth;
        oth = t;
        ++npiv;
    }
    // :392-400: a negative RHS (row 0 included) drops the last tableau
    neg = false;
    for (int i = lane; i < Rc; i += NT)
        if (!(cur[(size_t)i * Cc + (Cc - 1)] >= 0)) neg = true;
    if (ip_any<NT>(neg, red_i)) {
        if constexpr (kNarr) kept_drop(nc.c.kp, tab_n);  // tableaux.RemoveAt(Count - 1) :394
        if (npiv == 0) return kChildFailed;  // pivotColumns.RemoveAt(-1) throws
        double* t = cur;
        cur = oth;
        oth = t;
        trace_push(tr, lane, rid, 2, -1, -1);
    }
    return kChildSolved;
}

// At most `chunk` pops of the DFS of IP k = idx_in[q] by the NT lanes `lane` of sub-group `sub`.
// smem: the dynamic LDS; red_v / red_i: kWave reduction slots each.  An IP that is still running
// when its chunk is used up appends itself to idx_out (n_out counts them).
template <int NT, bool kLds, bool kNarr>
__device__ __forceinline__ void bb_batch_body(const BBBatchBufs& B, const BBNarr& narr, int k,
                                              int sub, int lane, int32_t* __restrict__ idx_out,
                                              int32_t* __restrict__ n_out, int chunk, int slot,
                                              double* smem, double* red_v, int* red_i) {
    BBBatchDesc* const d = B.desc + k;
    const int R0 = d->rows, C0 = d->cols, nv = d->nvars, cap = d->node_cap;
    const int64_t sn = d->slot_n();
    const bool pruning = d->enable_pruning != 0;
    const int max_piv = d->max_child_pivots;
    double* const stack = B.stack + d->stack_off;
    int32_t* const stk = B.stk + d->stk_off;
    double* const xv = B.x + d->x_off;
    double* const vals = B.vals + d->x_off;
    int32_t* const ri = B.rec_i + (int64_t)kBBRecInts * d->rec_off;
    double* const rd = B.rec_d + 2 * d->rec_off;
    int32_t* const pops = B.pops + d->pop_off;
    int32_t* const keys = B.ints + d->int_off;
    int32_t* const list = keys + (C0 + cap);
    double *buf0, *buf1, *fcol;
    if constexpr (kLds) {
        buf0 = smem + (size_t)sub * slot;
        buf1 = buf0 + sn;
        fcol = buf1 + sn;
    } else {
        buf0 = B.work + d->work_off;
        buf1 = buf0 + sn;
        fcol = smem;
    }
    Trace tr;
    tr.q = B.trace + 4 * d->trace_off;
    tr.cap = d->trace_cap;
    tr.n = d->pivots;
    int sp = d->sp, iteration = d->iteration, nrec = d->nrec, found = d->found;
    int best_node = d->best_node;
    int64_t processed = d->processed;
    double best_z = d->best_z;
    int32_t status = d->status;
    // narration (bb_narr_layout.hpp): the IP's cursors and where its records go
    NarrCursor nc;
    int64_t* n_tab_off = nullptr;
    int32_t* n_ntab = nullptr;
    double *n_pop_z = nullptr, *n_pop_vals = nullptr, *n_best = nullptr;
    int32_t* n_pop_flags = nullptr;
    if constexpr (kNarr) {
        nc.c = narr.desc[k];
        nc.slice = narr.slab + nc.c.slab_off;
        n_tab_off = narr.tab_off + d->rec_off;
        n_ntab = narr.ntab + d->rec_off;
        n_pop_z = narr.pop_z + d->pop_off;
        n_pop_flags = narr.pop_flags + d->pop_off;
        n_pop_vals = narr.pop_vals + (int64_t)cap * d->x_off;
        n_best = narr.best + nc.c.best_off;
    }

    for (int p = 0; p < chunk && status == kRunning; ++p) {
        if (sp == 0) {  // the stack emptied
            status = LPR_OK_OPTIMAL;
            break;
        }
        if (++iteration > cap) {  // "Potential infinite loop detected" :1038-1042
            status = LPR_BB_NODE_CAP;
            break;
        }
        const int s = --sp;
        const int id = stk[2 * s], dep = stk[2 * s + 1];
        double* const P = stack + s * sn;
        const int Rn = R0 + dep, Cn = C0 + dep;
        const int64_t pop_i = processed;
        if (lane == 0) pops[processed] = id;
        ++processed;
        // RoundAllTableaux :1047, in place
        for (int x = lane; x < Rn * Cn; x += NT) P[x] = dn_round4(P[x]);
        group_sync<NT, kFenceWorkgroup>();
        const double objVal = dn_round4(P[Cn - 1]);  // GetObjective :892-897
        if (pruning && found && objVal <= best_z) {  // ShouldPrunebranch :985-1004
            if constexpr (kNarr)
                if (lane == 0) {
                    n_pop_z[pop_i] = objVal;
                    n_pop_flags[pop_i] = 0;
                }
            continue;
        }
        // the decision values of CheckIntegerBasicVar :807-827 / ExtractSolution :899-921, IsInteger
        // :595-599, and the branching variable of :829-847 (strict <: the first of the closest)
        bool nonint = false;
        Cand bv;
        bv.v = 0.0;
        bv.i = -1;
        for (int i = lane; i < nv; i += NT) {
            double v = 0.0;
            for (int j = 0; j < Rn; ++j)
                if (fabs(dn_round4(P[(size_t)j * Cn + i]) - 1.0) <= kBBEps) {
                    v = dn_round4(P[(size_t)j * Cn + (Cn - 1)]);
                    break;
                }
            vals[i] = v;
            if constexpr (kNarr) n_pop_vals[pop_i * nv + i] = v;
            if (!dn_is_integer(v)) {
                nonint = true;
                const double dist = fabs((v - floor(v)) - 0.5);
                if (dist < INFINITY && (bv.i < 0 || dist < bv.v)) {
                    bv.v = dist;
                    bv.i = i;
                }
            }
        }
        const bool any_nonint = ip_any<NT>(nonint, red_i);
        bv = group_cand_min<NT>(bv, red_v, red_i);
        group_sync<NT, kFenceWorkgroup>();
        const bool improves = !any_nonint && objVal > best_z;
        if (improves) {  // UpdateOptimalSolution :935-983
            best_z = objVal;
            found = 1;
            best_node = id;
            for (int i = lane; i < nv; i += NT) xv[i] = vals[i];
            if constexpr (kNarr) {  // bestTableau = the popped node, rounded by :1047
                for (int x = lane; x < Rn * Cn; x += NT) n_best[x] = P[x];
                nc.c.best_depth = dep;
            }
        }
        if constexpr (kNarr)
            if (lane == 0) {
                n_pop_z[pop_i] = objVal;
                n_pop_flags[pop_i] = kNarrScored | (any_nonint ? 0 : kNarrInteger) |
                                     (improves ? kNarrIncumbent : 0);
            }
        if (bv.i < 0) continue;  // an integer node :1070-1076
        const int var = bv.i;
        const double bestValue = vals[var];
        const int upperInt = dn_to_int32(ceil(bestValue));  // :870-871
        const int lowerInt = dn_to_int32(floor(bestValue));
        // lower child :1083-1148, then upper :1150-1208; a solved lower child waits in slot s + 1,
        // the upper one goes to the parent's slot s (the parent is no longer read by then)
        int rid_ok[2] = {-1, -1};
        for (int side = 0; side < 2; ++side) {
            const double bound = side == 0 ? (double)lowerInt : (double)upperInt;
            const int rid = nrec++;
            double* cur = buf0;
            double* oth = buf1;
            const int Rc = Rn + 1, Cc = Cn + 1;
            int64_t first_off = 0, made0 = 0;
            double* rec = nullptr;
            if constexpr (kNarr) {
                first_off = nc.c.kp.cur;
                made0 = nc.c.kp.made_n;
                rec = nc.push((int64_t)Rc * Cc);
            }
            add_constraint<NT, kNarr>(P, Rn, Cn, nv, var, bound, side == 1, cur, keys, list, lane,
                                      red_i, rec);
            const int rc = child_lp<NT, kNarr>(cur, oth, fcol, Rc, Cc, rid, max_piv, tr, nc, lane,
                                               red_v, red_i);
            double z = 0.0;
            if (rc == kChildSolved) {  // RoundAllTableaux :1124 / :1187, into its stack slot
                double* const dst = stack + (side == 0 ? s + 1 : s) * sn;
                for (int x = lane; x < Rc * Cc; x += NT) dst[x] = dn_round4(cur[x]);
                z = dn_round4(dn_round4(cur[Cc - 1]));
                rid_ok[side] = rid;
            }
            if (lane == 0) {
                int32_t* const e = ri + (int64_t)kBBRecInts * rid;
                e[0] = id;
                e[1] = side + 1;
                e[2] = dep + 1;
                e[3] = var;
                e[4] = rc == kChildLimit ? LPR_PIVOT_LIMIT : rc;
                rd[2 * rid] = bound;
                rd[2 * rid + 1] = z;
                if constexpr (kNarr) {
                    n_tab_off[rid] = first_off;
                    n_ntab[rid] = (int32_t)(nc.c.kp.made_n - made0);
                }
            }
            group_sync<NT, kFenceWorkgroup>();
            if (rc == kChildLimit) {
                status = LPR_PIVOT_LIMIT;
                break;
            }
        }
        if (status != kRunning) break;
        // push upper first, so the lower child is popped next (:1210-1213)
        if (rid_ok[1] >= 0) {
            if (lane == 0) {
                stk[2 * sp] = rid_ok[1];
                stk[2 * sp + 1] = dep + 1;
            }
            ++sp;
        }
        if (rid_ok[0] >= 0) {
            if (sp == s) {  // the upper child failed: the lower one moves down into slot s
                const double* const src = stack + (s + 1) * sn;
                double* const dst = stack + s * sn;
                for (int x = lane; x < (Rn + 1) * (Cn + 1); x += NT) dst[x] = src[x];
            }
            if (lane == 0) {
                stk[2 * sp] = rid_ok[0];
                stk[2 * sp + 1] = dep + 1;
            }
            ++sp;
        }
        group_sync<NT, kFenceWorkgroup>();
    }

    if (lane == 0) {
        d->sp = sp;
        d->iteration = iteration;
        d->nrec = nrec;
        d->found = found;
        d->best_node = best_node;
        d->processed = processed;
        d->best_z = best_z;
        d->pivots = tr.n;
        d->status = status;
        if constexpr (kNarr) narr.desc[k] = nc.c;
        if (status == kRunning) idx_out[atomicAdd(n_out, 1)] = k;
    }
}

}  // namespace

}  // namespace lpr
