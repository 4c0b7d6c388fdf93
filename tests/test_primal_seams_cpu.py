"""CPU tests of the primal seam items (tests/primal_seam_cases.py): every plant is real.  For every
item the C oracle runs `at` pivots -- exactly the declared leaders, in order -- and in its tableau
the planted values are equal in the declared sense, strictly better than every other candidate,
the oracle's next pivot is the declared winner and every mutant selector the item names picks
another index.  The lane maps are pinned against the constants of the kernels' sources, the planted
positions against the seam class they declare, and the coverage table against the list every later
change must keep.  No item is skipped or filtered."""
import struct

import numpy as np
import pytest

import primal_seam_cases as pc
from ref_py import DBL_MAX

ALL = pc.all_items()
IDS = [it.name for it in ALL]


def bits(v):
    return struct.pack("<d", float(v))


# ------------------------------------------------------------------------------ the plant
@pytest.mark.parametrize("item", ALL, ids=IDS)
def test_plant_is_live_and_mutants_differ(oracle, item):
    ref = pc.reference(oracle, item)
    # the leaders took exactly `at` pivots, in the declared order
    assert ref.pivots_at == item.at and ref.log_at == item.leaders, (item.name, ref.log_at)
    view = pc.view_of(oracle, item)
    vals = view.vals
    if item.equal in ("bits", "value"):
        assert set(item.planted) <= set(vals), (item.name, item.label)
        win = vals[item.winner]
        rest = [v for i, v in vals.items() if i not in item.planted]
        assert rest and all(v > win for v in rest), (item.name, item.label)
        if item.equal == "bits":
            assert {bits(vals[i]) for i in item.planted} == {bits(win)}, (item.name, item.label)
            if item.at:  # the tied values went through real arithmetic: they are not the start's
                w, T0 = item.winner, item.T
                start = T0[0, w] if item.kind == "entering" else T0[w, -1] / T0[w, 0]
                assert bits(start) != bits(win), item.name
                if item.kind == "leaving":  # numerator and denominator both
                    assert ref.T_at[w, -1] != T0[w, -1] and ref.T_at[w, 0] != T0[w, 0], item.name
        else:  # +0.0 and -0.0, in the declared order
            got = [bits(vals[i]) for i in item.planted]
            assert sorted(got) == sorted([bits(0.0), bits(-0.0)]) and win == 0.0, item.name
            assert (got[0] == bits(0.0)) == ("signed_zero_ordered" in item.mutants), item.name
    elif item.equal == "overflow_all":  # every candidate ratio is +inf or exactly DBL_MAX
        assert not vals and set(view.raw) == set(item.planted), (item.name, sorted(view.raw))
        assert all(v in (np.inf, DBL_MAX) for v in view.raw.values()), item.name
        assert item.winner == -1 and ref.status == 1 and ref.pivots == item.at, item.name
    else:  # one overflowing row below the seam, the finite minimum across it
        lo, hi = item.planted
        assert item.equal == "overflow_one" and lo < hi == item.winner
        assert view.raw[lo] in (np.inf, DBL_MAX) and lo not in vals, item.name
        assert all(v > vals[hi] for i, v in vals.items() if i != hi), item.name
    if len(item.planted) > 1 and item.equal != "overflow_one":
        assert len(item.mutants) >= 1, item.name
    assert pc.first_min(view) == item.winner, (item.name, item.label, pc.first_min(view))
    if item.winner >= 0:  # the oracle's next pivot is the winner
        assert ref.pivots > item.at, item.name
        row, col = ref.log[item.at]
        assert (col if item.kind == "entering" else row) == item.winner, (item.name, row, col)
        if item.path == "select":
            T = np.ascontiguousarray(item.T)
            e = oracle.find_entering(T)
            assert (e if item.kind == "entering" else oracle.find_leaving(T, e)) == item.winner
    for name in item.mutants:
        got = pc.MUTANTS[name](view)
        assert got != item.winner, (item.name, item.label, name)
        assert got in item.planted, (item.name, item.label, name, got)


def test_mutant_rule_names_the_lane_seams():
    """Across a stride, an item, a trip, a workgroup or a collector round the later index sits in
    a lower lane: those items defeat lane_major; an x|y pair defeats pair_y_first."""
    for it in ALL:
        if it.equal != "bits":
            continue
        if it.seam in ("stride", "partial", "further", "collector", "group"):
            assert "lane_major" in it.mutants, it.name
        if it.seam in ("dpp", "wave", "pair"):
            assert "lane_major" not in it.mutants, it.name
        if it.seam == "pair":
            assert ("pair_y_first" in it.mutants) == (it.planted[0] % 2 == 0), it.name
    assert {m for it in ALL for m in it.mutants} == set(pc.MUTANTS)


def test_the_walk_positions_of_the_plants():
    """The declared seam of an item is the seam its planted positions sit on."""
    for it in ALL:
        pos = [pc.pos_of(it)(i) for i in it.planted]
        a, b = pos[0], pos[-1]
        lo, hi = it.planted[0], it.planted[-1]
        same_round = (a.trip, a.item, a.group) == (b.trip, b.item, b.group)
        if it.equal == "overflow_all":
            continue
        if it.seam == "pair":
            assert hi == lo + 1 and same_round and b.lane - a.lane == (lo % 2), it.name
        elif it.seam == "dpp":
            assert same_round and a.wave == b.wave, it.name
            assert (a.lane % 64, b.lane % 64) in pc.DPP_PAIRS, it.name
        elif it.seam == "wave":
            assert same_round and b.wave == a.wave + 1 and a.lane % 64 == 63 and b.lane % 64 == 0, \
                it.name
            assert hi == lo + 1, it.name
        elif it.seam == "slot":  # the 16-lane second stage of the small path: waves 0-3 | 4-7
            assert it.path == "small" and a.item == b.item and a.wave <= 3 < b.wave, it.name
        elif it.seam == "group":
            assert a.trip == b.trip and b.group == a.group + 1 and hi == lo + 1, it.name
            assert (a.lane, b.lane) == ({"kpivot": pc.OV_NT, "onepivot": pc.HEAD_NT}[it.path] - 1, 0)
        elif it.seam == "collector":
            ra, rb = pc.collector(a), pc.collector(b)
            assert it.path == "kpivot" and ra[0] == 0 and rb[0] == 1, it.name
            assert rb[1] <= ra[1] and any(pc.collector(p)[1] < ra[1] for p in pos[1:]), it.name
        elif it.seam == "further":
            assert b.trip == a.trip + 1 and hi == lo + 1 and b.lane == 0 and b.group == 0, it.name
        elif it.seam == "stride":
            assert (a.trip, a.item) < (b.trip, b.item), it.name
            key = [(p.lane, p.group) for p in pos]
            assert any(k <= key[0] for k in key[1:]), it.name
        else:
            assert it.seam == "partial", it.name
            assert (a.trip, a.item) < (b.trip, b.item) and (b.group, b.lane) < (a.group, a.lane)


def test_lane_maps_against_the_sources():
    k = pc.source_constants()
    assert k["SMALL_NT"] == pc.SMALL_NT and k["SMALL_MAX_R"] == pc.SMALL_MAX_R == 2 * pc.SMALL_NT
    assert k["SMALL_MAX_LD"] == pc.SMALL_MAX_LD == 4 * pc.SMALL_NT
    assert k["OV_NT"] == pc.OV_NT and k["OV_GROUPS"] == pc.OV_GROUPS and k["OV_WPG"] == pc.OV_WPG
    assert k["HEAD_GROUPS"] == pc.HEAD_GROUPS
    # threads per workgroup and unrolled trips, from the launches and loops of primal_kernels.hip
    assert k["HEAD_NT"] == pc.HEAD_NT and k["HEAD_ROWS_PER_TRIP"] == pc.HEAD_ROWS_PER_TRIP
    assert k["SELECT_NT"] == pc.SELECT_NT and k["SELECT_UNROLL"] == pc.SELECT_UNROLL
    assert k["FUSED_NT"] == pc.FUSED_NT
    assert k["SMALL_K"] == k["OV_MAX"] == 16  # `at` 15 | 16 is a block seam of both
    assert pc.CONDENSED == __import__("condensed_cases").FORCE
    # spot values of the maps
    w = pc.walk
    p = w("small", "entering", 1025, 1408)
    assert (p.item, p.lane, p.xy) == (1, 0, 1)
    p = w("small", "leaving", 999, 48)
    assert (p.item, p.lane, p.wave) == (1, 487, 7)
    p = w("fused", "leaving", 257, 16)
    assert (p.trip, p.lane) == (1, 0)
    p = w("onepivot", "entering", 4096, 4208)
    assert pc.head_groups(4208) == 3 and (p.trip, p.group, p.lane) == (0, 2, 0)
    p = w("onepivot", "entering", 65536, 65984)
    assert pc.head_groups(65984) == 32 and (p.trip, p.group, p.lane) == (1, 0, 0)
    p = w("onepivot", "leaving", 8192, 16)
    assert (p.trip, p.item, p.lane) == (1, 0, 0)
    p = w("select", "entering", 4095, 4208)
    assert (p.trip, p.item, p.lane) == (0, 3, 1023)
    p = w("kpivot", "entering", 8192, 8752)
    assert pc.ov_groups(8752) == 18 and (p.group, p.wave, p.lane) == (16, 0, 0)
    assert pc.collector(p) == (1, 0) and pc.collector(w("kpivot", "entering", 8191, 8752)) == (0, 63)
    p = w("kpivot", "entering", 32768, 33120)
    assert pc.ov_groups(33120) == 64 and (p.trip, p.group, p.lane) == (1, 0, 0)
    p = w("kpivot", "leaving", 512, 656)
    assert pc.ov_groups(656) == 2 and (p.trip, p.group, p.lane) == (1, 0, 0)


def test_every_item_lands_on_the_path_it_declares():
    """primal_plan.hpp's rule, restated: the small items fit the cache-resident path (so variant 0
    / block 0 takes it), no other item is run with variant 0, and the K-pivot shapes have the head
    workgroups their seams need."""
    for it in ALL:
        rows, ld = it.T.shape[0], pc.ld_of(it)
        fits = 2 <= rows <= pc.SMALL_MAX_R and ld <= pc.SMALL_MAX_LD
        if it.path == "small":
            assert fits, it.name
        else:
            assert all(v != 0 for v, _ in pc.PATHS[it.path]), it.name
        if it.path == "kpivot":
            G = pc.ov_groups(ld)
            top = max(pc.pos_of(it)(i).group for i in it.planted)
            assert top < G, (it.name, G)
            slack = it.T[1:, it.basis]
            assert np.array_equal(slack, np.eye(rows - 1)) and not it.T[0, it.basis].any(), it.name
        assert it.T.nbytes <= 12 << 20, (it.name, it.T.nbytes)


def test_coverage_table():
    got = pc.coverage()
    assert got == pc.EXPECTED_COVERAGE, {k: (got.get(k), pc.EXPECTED_COVERAGE.get(k))
                                         for k in set(got) | set(pc.EXPECTED_COVERAGE)
                                         if got.get(k) != pc.EXPECTED_COVERAGE.get(k)}
    assert {it.seam for it in ALL} == set(pc.SEAMS)
    assert {it.equal for it in ALL} == set(pc.EQUALS)
    for path, ats in pc.ATS.items():  # every `at` class of every path, on both kinds
        for kind in pc.KINDS:
            assert {it.at for it in pc.items(path) if it.kind == kind and it.block == 16} >= set(ats)
    assert {it.at for it in pc.items("kpivot") if it.block == 5} == set(pc.BLOCK5_ATS)
    print({p: len(pc.items(p)) for p in pc.PATHS})
