"""Constructed seam items for the single-handle primal paths (TEST ONLY; DESIGN.md sections 4, 4b
and 4c): the cache-resident path (k_small_heads), k_pivot_fused, the one-pivot pair k_bootstrap /
k_pivot_head, the step entry points (k_select) and the loop heads of the K-pivot paths, in place and
two-stream.  Every selection of those kernels is a per-lane scan over a strided walk, a combine
across the lanes of a wave and a combine across waves, workgroups and trips.  The C# takes the
FIRST candidate that wins a strict `<` (PrimalSimplexSolver.cs:152-191), so a kernel that is wrong
on one seam is right on all data but the data that ties exactly across that seam.  tests/
seam_cases.py plants such ties for the batch engines, all at iteration 0; here the plant is live
at a declared pivot `at` of a solve call, so that it is decided by the prologue of a call (at = 0),
from values carried in registers inside a block (1, 15), at the first pivots of the next block
(16, 17: chained through the block being swept in the two-stream form) and two blocks on (33).

Every item declares

    path        "small" | "fused" | "onepivot" | "select" | "kpivot" (PATHS: the opts of each)
    kind        "entering" | "leaving"
    seam        the seam class (SEAMS)
    at          the 0-based pivot at which the plant decides
    block       opts.block of the K-pivot runs (16; 5 on four items.  The cache-resident path has
                no block 5: primal_plan() takes it with block 0 only and its K is kSmallK = 16)
    planted     the tied indices as the log reports them (columns; rows, 1-based by nature)
    winner      the index that must be selected (-1: no candidate, the solve ends unbounded)
    equal       "bits" (the same double), "value" (+0.0 / -0.0), "overflow_all" (every candidate
                ratio is +inf or exactly DBL_MAX) or "overflow_one" (such a row below the seam, the
                only finite minimum across it)
    mutants     the wrong selectors (MUTANTS) that pick another index on this item

The construction: entering plants are twin columns, leaving plants twin rows (RHS included) that
stay bit-identical through any pivot that is not on them.  `at` leader columns with costs -100,
-99, ... come first; each has one positive entry, on a leader row of its own, so the leaders take
the first `at` pivots in a known order.  Each leader row has a small inexact entry in the planted
columns (entering) / each planted row a small negative entry in the leader columns and the leader
rows an entry in the entering column (leaving), so the tied values pass through real multiply /
subtract steps before they are compared.  test_primal_seams_cpu.py proves every declaration on the
C oracle; test_primal_seams_gpu.py runs the items on the device."""
from __future__ import annotations

import re
from pathlib import Path
from types import SimpleNamespace
from typing import List

import numpy as np

import seam_cases as sc
from ref_py import DBL_MAX
from seam_cases import DPP_PAIRS, first_min, free_index, last_wins

CSRC = Path(__file__).resolve().parent.parent / "lpr_381_group_v22_amd" / "csrc"

# ------------------------------------------------------------------------------ the paths
SMALL, FUSED, ONEPIVOT = 0x2000, 0x7ffe, 0x7fff
INPLACE, TWOSTREAM = 0x4008, 0x3008
SPREAD, MEMSIDE, CONDENSED = 0x20000, 0x40000, 1 << 26  # CONDENSED == condensed_cases.FORCE
# path -> [(opts.variant, opts.block or None for the item's own)]
PATHS = dict(
    small=[(0, 0), (SMALL, 0)],
    fused=[(FUSED, 1)],
    onepivot=[(ONEPIVOT, 1)],
    select=[],  # lpr_select_entering / lpr_select_leaving, no solve call
    kpivot=[(INPLACE, None), (INPLACE | SPREAD, None), (INPLACE | MEMSIDE, None),
            (TWOSTREAM, None), (TWOSTREAM | SPREAD, None), (TWOSTREAM | MEMSIDE, None),
            (TWOSTREAM | CONDENSED, None)])
SEAMS = ("pair", "dpp", "wave", "slot", "group", "collector", "stride", "partial", "further")
KINDS = ("entering", "leaving")
EQUALS = ("bits", "value", "overflow_all", "overflow_one")
K_ATS = (0, 1, 15, 16, 17, 33)   # block 16: prologue, in-block, last of a block, next block, ...
ONE_ATS = (0, 1, 2)              # k_bootstrap, then both parity banks of k_pivot_head
BLOCK5_ATS = (4, 5)              # block 5: the last pivot of a block and the first of the next
ATS = dict(small=K_ATS, kpivot=K_ATS, fused=ONE_ATS, onepivot=ONE_ATS, select=(0,))

# the constants of the lane maps, as the kernels' sources state them (pinned by the CPU test)
SMALL_NT, SMALL_MAX_R, SMALL_MAX_LD = 512, 1024, 2048
OV_NT, OV_GROUPS, OV_WPG = 256, 64, 4
HEAD_NT, HEAD_GROUPS, HEAD_ROWS_PER_TRIP = 1024, 32, 8
SELECT_NT, SELECT_UNROLL = 1024, 4
FUSED_NT = 256


def source_constants():
    """The same constants read from the sources."""
    def grab(name, text):
        m = re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*[\w ]+,\s*)*?" + name + r"\s*=\s*(\d+)", text)
        assert m, name
        return int(m.group(1))
    plan = (CSRC / "primal_plan.hpp").read_text()
    small = (CSRC / "small_kernels.hip").read_text()
    over = (CSRC / "overlap_kernels.hip").read_text()
    prim = (CSRC / "primal_kernels.hip").read_text() + (CSRC / "primal_kernels.hpp").read_text() + \
        (CSRC / "engine_common.hpp").read_text()
    m = re.search(r"kOvWPG\s*=\s*kOvNT\s*/\s*(\d+)", over)
    assert m, "kOvWPG"
    prim_k = (CSRC / "primal_kernels.hip").read_text()

    def body(kernel):  # the text of one kernel, up to the next one
        at = prim_k.index("void " + kernel + "(")
        end = prim_k.find("__global__", at)
        return prim_k[at:end if end > 0 else len(prim_k)]

    def launch_nt(kernel):  # threads per workgroup of every launch of the kernel: all the same
        nts = set(re.findall(r"hipLaunchKernelGGL\(\(?" + kernel + r"(?:<\d+>\))?,\s*[^,]+,\s*dim3\((\d+)\)",
                             prim_k))
        assert len(nts) == 1, (kernel, nts)
        return int(nts.pop())

    def unroll(kernel, var):  # the trip of the walk over `var`: `var += U * nt`
        us = set(re.findall(var + r"\s*\+=\s*(\d+)\s*\*\s*nt", body(kernel)))
        assert len(us) == 1, (kernel, var, us)
        return int(us.pop())

    per_group = set(re.findall(r"t->ld / 2 \+ (\d+)\) / (\d+)", prim_k))  # head_groups()
    assert len(per_group) == 1, per_group
    lo, hi = map(int, per_group.pop())
    assert lo + 1 == hi == launch_nt("k_pivot_head")
    assert launch_nt("k_select") == launch_nt("k_bootstrap")
    assert unroll("k_select", "j0") == unroll("k_select", "i0") == unroll("k_bootstrap", "j0")
    assert re.search(r"for \(int j = tid; j < C - 1; j \+= nt\)", body("k_pivot_fused"))
    assert re.search(r"for \(int i = 1 \+ tid; i < R; i \+= nt\)", body("k_pivot_fused"))
    return dict(SMALL_NT=grab("kSmallNT", small), SMALL_MAX_R=grab("kSmallMaxR", plan),
                SMALL_MAX_LD=grab("kSmallMaxLd", plan), SMALL_K=grab("kSmallK", plan),
                OV_NT=grab("kOvNT", plan), OV_GROUPS=grab("kOvGroups", plan),
                OV_WPG=grab("kOvNT", plan) // int(m.group(1)),
                OV_MAX=grab("kOvMax", plan), HEAD_GROUPS=grab("kMaxHeadGroups", prim),
                HEAD_NT=launch_nt("k_pivot_head"),
                HEAD_ROWS_PER_TRIP=unroll("k_pivot_head", "i0"),
                SELECT_NT=launch_nt("k_select"), SELECT_UNROLL=unroll("k_select", "j0"),
                FUSED_NT=launch_nt("k_pivot_fused"))


def align16(x):
    return (x + 15) // 16 * 16


def ov_groups(ld):
    return max(1, min(OV_GROUPS, (ld // 2 + OV_NT - 1) // OV_NT))


def head_groups(ld):
    return max(1, min(HEAD_GROUPS, (ld // 2 + HEAD_NT - 1) // HEAD_NT))


# ------------------------------------------------------------------------------ lane maps
def _pos(trip=0, item=0, lane=0, group=0, xy=0):
    return SimpleNamespace(trip=trip, item=item, lane=lane, wave=lane // 64, group=group, xy=xy)


def walk(path, kind, index, ld, bootstrap=False):
    """index (a column, or a row) -> (trip, item, lane, wave, group, xy) in the kernel that decides
    `kind` on `path`.  bootstrap: the first entering column of a one-pivot call (k_bootstrap)."""
    if path == "small":  # a lane owns pairs t, t + 512 and rows t, t + 512
        p = index // 2 if kind == "entering" else index
        return _pos(item=p // SMALL_NT, lane=p % SMALL_NT, xy=index % 2 if kind == "entering" else 0)
    if path == "fused":  # j = tid + 256 k; i = 1 + tid + 256 k
        p = index if kind == "entering" else index - 1
        return _pos(trip=p // FUSED_NT, lane=p % FUSED_NT)
    if path == "select" or (path == "onepivot" and kind == "entering" and bootstrap):
        span = SELECT_NT * SELECT_UNROLL  # j0 + u 1024 for u < 4, outer += 4096
        return _pos(trip=index // span, item=index % span // SELECT_NT, lane=index % SELECT_NT)
    if path == "onepivot" and kind == "leaving":  # tid + u 1024 for u < 8, then += 8192
        span = HEAD_NT * HEAD_ROWS_PER_TRIP
        return _pos(trip=index // span, item=index % span // HEAD_NT, lane=index % HEAD_NT)
    if path == "onepivot":  # pair c2 = g 1024 + tid, G workgroups, a further trip past 2048 G
        span = head_groups(ld) * HEAD_NT
        c2 = index // 2
        return _pos(trip=c2 // span, group=c2 % span // HEAD_NT, lane=c2 % HEAD_NT, xy=index % 2)
    assert path == "kpivot"
    span = ov_groups(ld) * OV_NT  # pair (row) g 256 + tid, further ones += G 256
    p = index // 2 if kind == "entering" else index
    return _pos(trip=p // span, group=p % span // OV_NT, lane=p % OV_NT,
                xy=index % 2 if kind == "entering" else 0)


def collector(pos):
    """(round, lane) of the heads' collector for the partial of (group, wave)."""
    part = pos.group * OV_WPG + pos.wave
    return part // 64, part % 64


# ------------------------------------------------------------------------------ selectors
# A view is what the planted selection sees in the oracle's tableau after `at` pivots: view.vals
# maps candidate index -> value (smaller wins; ratios below DBL_MAX only), view.raw every ratio
# that passed `a > 1e-9` and `ratio >= 0`, view.pos the lane map.
def _tied(view):
    m = min(view.vals.values())
    return [i for i, v in view.vals.items() if v == m]


def lane_major(view) -> int:
    """Ties go to the lowest lane, then group, then trip: a reduction that never compares indices."""
    def key(i):
        p = view.pos(i)
        return (p.lane, p.group, p.item, p.trip, p.xy)
    return min(_tied(view), key=key)


def pair_y_first(view) -> int:
    """The y half of a lane's double2 is scanned before its x half."""
    return min(_tied(view), key=lambda i: (i // 2, -(i % 2)))


def signed_zero_ordered(view) -> int:
    """-0.0 counts as below +0.0 (a minimum taken on the bit patterns, or v_min's own order)."""
    return min(view.vals, key=lambda i: (view.vals[i], 0 if np.signbit(view.vals[i]) else 1, i))


def first_ratio_unchecked(view) -> int:
    """A lane takes its first ratio without the `< double.MaxValue` test (m.i < 0 || ratio < m.v);
    the lanes are then combined by (value, index)."""
    best = {}
    for i in sorted(view.raw):
        p = view.pos(i)
        lane = (p.group, p.lane)
        if lane not in best or view.raw[i] < best[lane][0]:
            best[lane] = (view.raw[i], i)
    return min(best.values())[1] if best else -1


MUTANTS = dict(last_wins=last_wins, lane_major=lane_major, pair_y_first=pair_y_first,
               signed_zero_ordered=signed_zero_ordered, first_ratio_unchecked=first_ratio_unchecked)
LANE_SEAMS = ("stride", "partial", "further", "collector", "group", "slot")


def mutants_of(path, kind, at, planted, ld):
    """The selectors a tie at `planted` (ascending, the first must win) defeats, from the lane map:
    last_wins always; lane_major when a later index sits lower in (lane, group, item, trip);
    pair_y_first when the y half of the winner's own pair is planted."""
    if len(planted) < 2:
        return ()
    boot = path == "onepivot" and at == 0
    view = SimpleNamespace(vals={i: 0.0 for i in planted},
                           pos=lambda i: walk(path, kind, i, ld, bootstrap=boot))
    out = ["last_wins"]
    if lane_major(view) != planted[0]:
        out.append("lane_major")
    paired = kind == "entering" and path in ("small", "kpivot", "onepivot") and not boot
    if paired and pair_y_first(view) != planted[0]:
        out.append("pair_y_first")
    return tuple(out)


# ------------------------------------------------------------------------------ tableaux
OVERFLOW = ((1e-8, 1e308),                                    # 1e308 / 1e-8 = +inf
            (2.0 ** -29, 2.0 ** 994 * (2.0 - 2.0 ** -52)))    # == DBL_MAX exactly
NBODY = 3


def _free(taken, count, start):
    out, taken = [], set(taken)
    k = start
    while len(out) < count:
        if k not in taken:
            out.append(k)
        k += 1
    return out


def entering_tableau(n, at, planted, slack):
    """n structural columns; the planted twin columns hold the most negative Z entry from pivot `at`
    on.  Rows: Z, `at` leader rows, NBODY body rows."""
    m = at + NBODY
    C = n + (m if slack else 0) + 1
    leaders = _free(planted, at, 9)
    assert max(list(planted) + leaders) < n
    T = np.zeros((m + 1, C))
    j = np.arange(n)
    T[0, :n] = -1.0 - (j % 7) / 8.0
    T[0, list(planted)] = -50.0
    for k, lc in enumerate(leaders):
        T[0, lc] = -100.0 + k
        T[1 + k, lc] = 3.0
        T[1 + k, list(planted)] = 0.001 * (1 + k % 5)
        T[1 + k, -1] = 1.0 + k
    for b in range(NBODY):
        r = at + 1 + b
        T[r, :n] = 1.0 + ((7 * r + 3 * j) % 3)
        T[r, leaders] = 0.0
        T[r, list(planted)] = 1.0 + b
        T[r, -1] = 40.0 + b
    if slack:
        T[1:, n:n + m] = np.eye(m)
    basis = (n if slack else C) + np.arange(m, dtype=np.int32)
    return T, basis, leaders


def leaving_tableau(R, n, at, planted, slack, equal="bits", order=0):
    """R rows; column 0 enters at pivot `at` (leaders are columns 1 .. at) and the planted twin rows
    hold its minimum ratio.  equal: "value": RHS +0.0 / -0.0 on the two planted rows (order 1:
    -0.0 first); "overflow_all": the planted rows are the only candidates and every ratio overflows;
    "overflow_one": the first planted row overflows, the second holds the finite minimum."""
    m = R - 1
    assert n >= at + 3 and max(planted) < R and min(planted) >= 1
    C = n + (m if slack else 0) + 1
    lrows = _free(planted, at, 5)
    assert not lrows or max(lrows) < R
    i = np.arange(R).reshape(-1, 1)
    j = np.arange(n).reshape(1, -1)
    T = np.zeros((R, C))
    T[:, :n] = 1.0 + ((7 * i + 3 * j) % 3)
    T[:, 0] = -1.0 if equal == "overflow_all" else 1.0 + (np.arange(R) % 3)
    T[:, 1:at + 1] = 0.0
    T[:, -1] = 40.0 + (np.arange(R) % 5)
    T[0, :n] = -1.0 - (np.arange(n) % 7) / 8.0
    T[0, 0] = -50.0
    T[0, -1] = 0.0
    untouched = equal in ("overflow_all", "overflow_one")  # the overflowing data must stay exact
    for k, lr in enumerate(lrows):
        T[0, 1 + k] = -100.0 + k
        T[lr, :n] = 0.0
        T[lr, 0] = 0.0 if equal == "overflow_all" else 0.003 * (1 + k % 3)
        T[lr, 1 + k] = 3.0
        T[lr, -1] = 1.0 + k
    for q, p in enumerate(planted):
        T[p, at + 1:n] = 1.0 + (np.arange(at + 1, n) % 3)
        T[p, 1:at + 1] = 0.0 if untouched else -0.001 * (1 + np.arange(at) % 5)
        T[p, 0], T[p, -1] = 1.0, 4.0
        if equal == "value":
            T[p, -1] = (0.0, -0.0)[(q + order) % 2]
        elif equal == "overflow_all" or (equal == "overflow_one" and q == 0):
            T[p, 0], T[p, -1] = OVERFLOW[(q + order) % 2]
    if slack:
        T[1:, n:n + m] = np.eye(m)
    basis = (n if slack else C) + np.arange(m, dtype=np.int32)
    return T, basis, lrows


# ------------------------------------------------------------------------------ items
def _item(**kw):
    kw.setdefault("equal", "bits")
    kw.setdefault("block", 16)
    kw["name"] = "{path}_{kind}_{seam}_at{at}_{w}{t}".format(
        w="_".join(str(p) for p in kw["planted"]), t=kw.pop("tag", ""), **kw)
    return SimpleNamespace(**kw)


def entering_item(path, seam, label, planted, at, n, slack, **kw):
    T, basis, leaders = entering_tableau(n, at, planted, slack)
    return _item(path=path, kind="entering", seam=seam, label=label, at=at, planted=tuple(planted),
                 winner=planted[0],
                 mutants=mutants_of(path, "entering", at, planted, align16(T.shape[1])),
                 T=T, basis=basis, leaders=[(1 + k, c) for k, c in enumerate(leaders)], **kw)


def leaving_item(path, seam, label, planted, at, R, n, slack, equal="bits", order=0, **kw):
    T, basis, lrows = leaving_tableau(R, n, at, planted, slack, equal, order)
    mut = mutants_of(path, "leaving", at, planted, align16(T.shape[1]))
    if equal == "bits":
        winner = planted[0]
    elif equal == "value":
        winner = planted[0]
        mut += ("signed_zero_ordered",) if order == 0 else ()
    elif equal == "overflow_all":
        winner, mut = -1, ("first_ratio_unchecked",)
    else:
        winner, mut = planted[1], ()
    tag = kw.pop("tag", "") + ("" if equal == "bits" else "_" + equal + (str(order) if order else ""))
    return _item(path=path, kind="leaving", seam=seam, label=label, at=at, planted=tuple(planted),
                 winner=winner, mutants=mut, equal=equal, tag=tag, T=T, basis=basis,
                 leaders=[(r, 1 + k) for k, r in enumerate(lrows)], **kw)


def _rotate(plants, ats):
    """One plant of every seam class at every `at`: the plants of a class take turns."""
    for q, at in enumerate(ats):
        for seam, lst in plants.items():
            yield at, seam, lst[q % len(lst)]
    for seam, lst in plants.items():  # more plants than `at`s: the rest take turns as well
        for q in range(len(ats), len(lst)):
            yield ats[q % len(ats)], seam, lst[q]


def _lanes(nt, scale=1, off=0, step=0):
    """(label, positions) of the in-wave pairs, cycling through the waves of a workgroup."""
    out = []
    for q, (lo, hi) in enumerate(DPP_PAIRS):
        base = 64 * ((q + step) % (nt // 64))
        out.append((f"lanes {base + lo}|{base + hi}",
                    (scale * (base + lo) + off, scale * (base + hi) + off)))
    return out


def small_items():
    """R <= 1024, ld <= 2048: no slack block, so both walks reach their second item."""
    out = []
    nt = SMALL_NT
    n = 1400  # pairs 0 .. 699: the second item of lanes 0 .. 187
    ent = dict(
        pair=[("x|y of lane 37", (74, 75)), ("y|x of lanes 37|38", (75, 76)),
              ("x|y of lane 5, second item", (2 * (nt + 5), 2 * (nt + 5) + 1))],
        dpp=_lanes(nt, scale=2),
        wave=[(f"waves {64 * w - 1}|{64 * w}", (128 * w - 1, 128 * w)) for w in (1, 2, 3, 5, 6, 7)],
        slot=[("waves 3|4: lanes 255|256", (511, 512)), ("waves 3|4: lanes 200|300", (401, 600))],
        stride=[("pairs 3|515, decoy 514", (6, 2 * (nt + 2), 2 * (nt + 3))),
                ("item seam: pairs 511|512", (2 * nt - 1, 2 * nt))],
        partial=[("last round 188|699", (2 * 188 + 1, 2 * 699))])
    for at, seam, (label, pos) in _rotate(ent, K_ATS):
        out.append(entering_item("small", seam, label, pos, at, n, False))
    R, nc = 1000, 40  # rows 1 .. 999: the second item of lanes 0 .. 487
    lea = dict(
        dpp=_lanes(nt),
        wave=[(f"waves {64 * w - 1}|{64 * w}", (64 * w - 1, 64 * w)) for w in (1, 2, 3, 5, 6, 7)],
        slot=[("waves 3|4: rows 255|256", (255, 256)), ("waves 3|4: rows 200|300", (200, 300))],
        stride=[("rows 3|515, decoy 514", (3, nt + 2, nt + 3)),
                ("item seam: rows 511|512", (nt - 1, nt))],
        partial=[("last round 488|999", (488, 999))])
    for at, seam, (label, pos) in _rotate(lea, K_ATS):
        out.append(leaving_item("small", seam, label, pos, at, R, nc, False))
    for order in (0, 1):
        out.append(leaving_item("small", "wave", "+0.0|-0.0 at rows 63|64", (63, 64), 0, R, nc,
                                False, equal="value", order=order))
        out.append(leaving_item("small", "stride", "+0.0|-0.0 at rows 7|519", (7, nt + 7), 0, R, nc,
                                False, equal="value", order=order))
    for at in (0, 1):
        out.append(leaving_item("small", "stride", "overflow on both items of lanes 9, 70",
                                (9, 70, nt + 9, nt + 70), at, R, nc, False, equal="overflow_all",
                                order=at))
        out.append(leaving_item("small", "wave", "one overflowing row", (200,), at, R, nc, False,
                                equal="overflow_all", order=at, tag="_single"))
        out.append(leaving_item("small", "stride", "overflow at 9, finite at 521", (9, nt + 9), at, R,
                                nc, False, equal="overflow_one", order=at))
        out.append(leaving_item("small", "wave", "overflow at 63, finite at 64", (63, 64), at, R, nc,
                                False, equal="overflow_one", order=1 - at))
    return out


def _scalar_plants(nt, count, unroll=None):
    """Plants of a scalar walk of `count` positions with stride nt (seam_cases.seam_pairs), plus the
    seams of an unrolled trip of `unroll` strides."""
    plants = dict(dpp=[], wave=[], stride=[], partial=[])
    for seam, label, pos in sc.seam_pairs(nt, count):
        plants[seam].append((label, pos))
    if unroll:
        span = unroll * nt
        plants["stride"] += [(f"unrolled trip {span - 1}|{span}", (span - 1, span)),
                             (f"outer stride 3|{span + 3}, decoy {span + 2}", (3, span + 2, span + 3)),
                             (f"item seam {nt - 1}|{nt}", (nt - 1, nt))]
    return plants


def fused_items():
    out = []
    for at, seam, (label, pos) in _rotate(_scalar_plants(FUSED_NT, 700), ONE_ATS):
        out.append(entering_item("fused", seam, label, pos, at, 701, False))
    for at, seam, (label, pos) in _rotate(_scalar_plants(FUSED_NT, 700), ONE_ATS):
        rows = tuple(p + 1 for p in pos)
        out.append(leaving_item("fused", seam, label, rows, at, 701, 8, False))
    out += _edge_items("fused", 701, 8, False, (64, 65), [("stride", (256, 257))], ats=(0,))
    return out


def _edge_items(path, R, n, slack, wave_pair, others, ats):
    """+0.0 / -0.0 in both orders across a wave seam; every ratio overflowing, on both sides of
    every seam given; one overflowing row below each seam and the finite minimum across it.
    others: [(seam class, (lower row, upper row))]."""
    out = []
    for order in (0, 1):
        out.append(leaving_item(path, "wave", "+0.0|-0.0 at rows %d|%d" % wave_pair, wave_pair, 0,
                                R, n, slack, equal="value", order=order))
    rows = tuple(sorted(set(wave_pair + sum((p for _, p in others), ()))))
    for at in ats:
        out.append(leaving_item(path, "wave", "every ratio overflows: rows " + str(rows), rows, at,
                                R, n, slack, equal="overflow_all", order=at))
        for q, (seam, pair) in enumerate([("wave", wave_pair)] + list(others)):
            out.append(leaving_item(path, seam, "overflow at %d, finite at %d" % pair, pair, at, R,
                                    n, slack, equal="overflow_one", order=(at + q) % 2))
    return out


def select_items():
    """k_select, the step entry points: j0 + u 1024 for u < 4, outer += 4096."""
    out = []
    plants = _scalar_plants(SELECT_NT, 4200, unroll=SELECT_UNROLL)
    for seam, lst in plants.items():
        for label, pos in lst:
            out.append(entering_item("select", seam, label, pos, 0, 4201, False))
            out.append(leaving_item("select", seam, label, pos, 0, 4201, 6, False))
    out += _edge_items("select", 4201, 6, False, (63, 64), [("stride", (1023, 1024))], ats=(0,))
    return out


def onepivot_items():
    out = []
    # the first entering column of a call: k_bootstrap, the scalar walk of k_select
    for seam, lst in _scalar_plants(HEAD_NT, 4200, unroll=SELECT_UNROLL).items():
        for label, pos in (lst[1:] if seam == "stride" else lst[-1:]):
            out.append(entering_item("onepivot", seam, label + " (bootstrap)", pos, 0, 4201, False))
    # later ones: k_pivot_head, pair c2 = g 1024 + tid; G = 3 at ld = 4208
    nt = HEAD_NT
    ent = dict(
        pair=[("x|y of lane 37", (74, 75)), ("y|x of lanes 37|38", (75, 76))],
        dpp=_lanes(nt, scale=2, step=1)[:2] + _lanes(nt, scale=2, step=7)[2:],
        wave=[(f"waves {64 * w - 1}|{64 * w}", (128 * w - 1, 128 * w)) for w in (1, 8, 15)],
        group=[("workgroups 0|1: pairs 1023|1024", (2 * nt - 1, 2 * nt)),
               ("workgroups 1|2: pairs 2047|2048", (4 * nt - 1, 4 * nt))])
    for at in (1, 2):  # a head reads the partials of one parity bank and writes the other
        for seam, lst in ent.items():
            for q, (label, pos) in enumerate(lst):
                if q % 2 != at % 2:
                    out.append(entering_item("onepivot", seam, label, pos, at, 4201, False))
    # the second trip of a head lane: ld > 65 536, G = 32
    span = 2 * HEAD_GROUPS * nt
    for at, (seam, label, pos) in zip((1, 2, 1), (
            ("further", f"trips: columns {span - 1}|{span}", (span - 1, span)),
            ("stride", f"pairs 3|{span // 2 + 3}, decoy {span // 2 + 2}", (6, span + 4, span + 6)),
            ("partial", "last round", (2 * 217 + 1, span + 2 * 216)))):
        out.append(entering_item("onepivot", seam, label, pos, at, span + 440, False))
    # leaving: rows tid + u 1024 for u < 8, then += 8192, in every workgroup
    R = 8300
    plants = _scalar_plants(nt, R - 1)
    span = nt * HEAD_ROWS_PER_TRIP
    plants["stride"] += [(f"unrolled trip {span - 1}|{span}", (span - 1, span)),
                         (f"outer stride 3|{span + 3}, decoy {span + 2}", (3, span + 2, span + 3)),
                         (f"item seam {4 * nt - 1}|{4 * nt}", (4 * nt - 1, 4 * nt))]
    plants["partial"] = [("last round", (8299 - span + 1, 8299))]
    for at, seam, (label, pos) in _rotate(plants, ONE_ATS):
        out.append(leaving_item("onepivot", seam, label, pos, at, R, 6, False))
    out += _edge_items("onepivot", R, 6, False, (63, 64),
                       [("stride", (1023, 1024)), ("stride", (8191, 8192))], ats=(0,))
    return out


def kpivot_items():
    """Standard form (a slack block, the start basis): the condensed layout needs unit columns.
    ld = 720 (G = 2) for the in-group seams, ld > 8192 for the collector's, ld > 32 768 for the
    further pairs; rows: ld <= 512 (G = 1: further rows from 256 on) and G = 2."""
    out = []
    nt = OV_NT
    n_narrow, n_coll = 680, 8700
    span = 2 * OV_GROUPS * nt  # columns per trip of all 64 groups
    n_far = span + 300
    ent = dict(
        pair=[("x|y of lane 37", (74, 75), n_narrow), ("y|x of lanes 37|38", (75, 76), n_narrow),
              ("x|y in group 1", (2 * nt + 10, 2 * nt + 11), n_narrow)],
        dpp=[(lb, pos, n_narrow) for lb, pos in _lanes(nt, scale=2)],
        wave=[(f"waves {64 * w - 1}|{64 * w}", (128 * w - 1, 128 * w), n_narrow) for w in (1, 2, 3)],
        group=[("workgroups 0|1: pairs 255|256", (2 * nt - 1, 2 * nt), n_narrow)],
        collector=[("partials 63|64: columns 8191|8192", (8191, 8192), n_coll),
                   ("partials 3|67, decoy 66", (2 * 64 * 3, 2 * 64 * 66, 2 * 64 * 67), n_coll)],
        further=[(f"owned|further pairs: columns {span - 1}|{span}", (span - 1, span), n_far)],
        stride=[(f"pairs 3|{span // 2 + 3}, decoy {span // 2 + 2}", (6, span + 4, span + 6), n_far)],
        partial=[("last round", (2 * 117 + 1, span + 2 * 116), n_far)])
    for at, seam, (label, pos, n) in _rotate(ent, K_ATS):
        out.append(entering_item("kpivot", seam, label, pos, at, n, True))
    out.append(entering_item("kpivot", "wave", "waves 63|64, block 5", (127, 128), 4, n_narrow, True,
                             block=5, tag="_b5"))
    out.append(entering_item("kpivot", "group", "workgroups 0|1, block 5", (2 * nt - 1, 2 * nt), 5,
                             n_narrow, True, block=5, tag="_b5"))
    # rows: (R, n): G = 1 (further rows 256 ..), G = 2 (a group seam at 255|256, further at 512)
    g1, g2 = (300, 40), (600, 50)
    assert ov_groups(align16(g1[1] + g1[0])) == 1 and ov_groups(align16(g2[1] + g2[0])) == 2
    lea = dict(
        dpp=[(lb, pos, g1) for lb, pos in _lanes(nt)],
        wave=[(f"waves {64 * w - 1}|{64 * w}", (64 * w - 1, 64 * w), g1) for w in (1, 2, 3)],
        group=[("workgroups 0|1: rows 255|256", (nt - 1, nt), g2)],
        further=[("owned|further rows 255|256", (nt - 1, nt), g1),
                 ("owned|further rows 511|512", (2 * nt - 1, 2 * nt), g2)],
        stride=[("rows 3|259, decoy 258", (3, nt + 2, nt + 3), g1),
                ("rows 3|515, decoy 514", (3, 2 * nt + 2, 2 * nt + 3), g2)],
        partial=[("last round 44|299", (44, 299), g1), ("last round 88|599", (88, 599), g2)])
    for at, seam, (label, pos, (R, n)) in _rotate(lea, K_ATS):
        out.append(leaving_item("kpivot", seam, label, pos, at, R, n, True))
    out.append(leaving_item("kpivot", "wave", "waves 63|64, block 5", (63, 64), 5, g1[0], g1[1], True,
                            block=5, tag="_b5"))
    out.append(leaving_item("kpivot", "further", "owned|further rows, block 5", (nt - 1, nt), 4,
                            g1[0], g1[1], True, block=5, tag="_b5"))
    out += _edge_items("kpivot", g2[0], g2[1], True, (63, 64),
                       [("group", (nt - 1, nt)), ("further", (2 * nt - 1, 2 * nt))], ats=(0, 1))
    return out


_ITEMS = {}
_MAKERS = dict(small=small_items, fused=fused_items, onepivot=onepivot_items, select=select_items,
               kpivot=kpivot_items)


def items(path: str) -> List[SimpleNamespace]:
    """The items of one path, built once."""
    if path not in _ITEMS:
        _ITEMS[path] = _MAKERS[path]()
        names = [it.name for it in _ITEMS[path]]
        assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return _ITEMS[path]


def all_items():
    return [it for p in PATHS for it in items(p)]


def ld_of(item):
    return align16(item.T.shape[1])


def pos_of(item):
    """index -> walk position in the kernel that decides the item's plant."""
    ld = ld_of(item)
    boot = item.path == "onepivot" and item.at == 0
    return lambda i: walk(item.path, item.kind, i, ld, bootstrap=boot)


# ------------------------------------------------------------------------------ oracle references
_REFS = {}


def reference(oracle, item):
    """The oracle on the item, once: the tableau after `at` pivots (T_at, log_at), and status,
    pivots, log, basis and tableau after max_pivots = at + 2."""
    if item.name not in _REFS:
        T, b = item.T.copy(), item.basis.copy()
        st0, piv0, log0 = oracle.primal_solve(T, b, item.at) if item.at else (5, 0, np.zeros((0, 2)))
        T_at = T.copy()
        T2, b2 = item.T.copy(), item.basis.copy()
        st, piv, log = oracle.primal_solve(T2, b2, item.at + 2)
        _REFS[item.name] = SimpleNamespace(T_at=T_at, status_at=st0, pivots_at=piv0,
                                           log_at=[tuple(x) for x in np.asarray(log0).tolist()],
                                           status=st, pivots=piv, log=log.tolist(),
                                           basis=b2.tolist(), tbytes=T2.tobytes())
    return _REFS[item.name]


def view_of(oracle, item):
    """The candidates of the planted selection in the oracle's tableau after `at` pivots."""
    T = reference(oracle, item).T_at
    if item.kind == "entering":
        z = T[0, :-1]
        vals = {int(j): float(z[j]) for j in np.nonzero(z < 0)[0]}
        raw = vals
    else:
        e = oracle.find_entering(T)
        a, b = T[1:, e], T[1:, -1]
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            ratio = b / np.where(a > 1e-9, a, 1.0)
        raw = {int(i) + 1: float(ratio[i]) for i in np.nonzero((a > 1e-9) & (ratio >= 0))[0]}
        vals = {i: v for i, v in raw.items() if v < DBL_MAX}
    return SimpleNamespace(rule="first_min", vals=vals, raw=raw, pos=pos_of(item))


# ------------------------------------------------------------------------------ coverage
def _cells():
    out = set()
    for it in all_items():
        out.add((it.path, it.kind, it.equal, it.seam, it.at if it.block == 16 else f"b5:{it.at}"))
    return out


def coverage():
    """{(path, kind, equal): {seam: sorted `at`s}}"""
    table = {}
    for path, kind, equal, seam, at in _cells():
        table.setdefault((path, kind, equal), {}).setdefault(seam, set()).add(at)
    return {k: {s: sorted(v, key=str) for s, v in sorted(d.items())} for k, d in table.items()}


_K = list(K_ATS)
_ONE = list(ONE_ATS)
EXPECTED_COVERAGE = {
    ("small", "entering", "bits"): dict(pair=_K, dpp=_K, wave=_K, slot=_K, stride=_K, partial=_K),
    ("small", "leaving", "bits"): dict(dpp=_K, wave=_K, slot=_K, stride=_K, partial=_K),
    ("small", "leaving", "value"): dict(wave=[0], stride=[0]),
    ("small", "leaving", "overflow_all"): dict(wave=[0, 1], stride=[0, 1]),
    ("small", "leaving", "overflow_one"): dict(wave=[0, 1], stride=[0, 1]),
    ("fused", "entering", "bits"): dict(dpp=_ONE, wave=_ONE, stride=_ONE, partial=_ONE),
    ("fused", "leaving", "bits"): dict(dpp=_ONE, wave=_ONE, stride=_ONE, partial=_ONE),
    ("fused", "leaving", "value"): dict(wave=[0]),
    ("fused", "leaving", "overflow_all"): dict(wave=[0]),
    ("fused", "leaving", "overflow_one"): dict(wave=[0], stride=[0]),
    ("onepivot", "entering", "bits"): dict(pair=[1, 2], dpp=[0, 1, 2], wave=[0, 1, 2],
                                           group=[1, 2], stride=[0, 2], partial=[0, 1],
                                           further=[1]),
    ("onepivot", "leaving", "bits"): dict(dpp=_ONE, wave=_ONE, stride=_ONE, partial=_ONE),
    ("onepivot", "leaving", "value"): dict(wave=[0]),
    ("onepivot", "leaving", "overflow_all"): dict(wave=[0]),
    ("onepivot", "leaving", "overflow_one"): dict(wave=[0], stride=[0]),
    ("select", "entering", "bits"): dict(dpp=[0], wave=[0], stride=[0], partial=[0]),
    ("select", "leaving", "bits"): dict(dpp=[0], wave=[0], stride=[0], partial=[0]),
    ("select", "leaving", "value"): dict(wave=[0]),
    ("select", "leaving", "overflow_all"): dict(wave=[0]),
    ("select", "leaving", "overflow_one"): dict(wave=[0], stride=[0]),
    ("kpivot", "entering", "bits"): dict(pair=_K, dpp=_K, wave=_K + ["b5:4"], group=_K + ["b5:5"],
                                         collector=_K, further=_K, stride=_K, partial=_K),
    ("kpivot", "leaving", "bits"): dict(dpp=_K, wave=_K + ["b5:5"], group=_K,
                                        further=_K + ["b5:4"], stride=_K, partial=_K),
    ("kpivot", "leaving", "value"): dict(wave=[0]),
    ("kpivot", "leaving", "overflow_all"): dict(wave=[0, 1]),
    ("kpivot", "leaving", "overflow_one"): dict(wave=[0, 1], group=[0, 1], further=[0, 1]),
}
