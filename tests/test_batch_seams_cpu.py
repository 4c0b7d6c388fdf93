"""CPU tests of the seam items (tests/seam_cases.py): every plant is real.  For every item the
planted tie (or EPS band) is present at the declared place in the Python restatement, every other
candidate loses to it strictly, the right selection and the C oracle's log give the declared
winner there, every mutant selector the item names picks another index, the oracle and the
restatement agree on the whole item, the shape lands in the declared form, and across the set
every coverage cell has an item.  No item is skipped or filtered."""
import math
import struct

import numpy as np
import pytest

import seam_cases as sc
from ref_py import DBL_MAX, REV_EPS

ALL = [it for eng in ("primal", "revised", "bb") for it in sc.items(eng)]
IDS = [it.name for it in ALL]


def bits(v):
    return struct.pack("<d", float(v))


# ------------------------------------------------------------------------------ the plant
@pytest.mark.parametrize("item", ALL, ids=IDS)
def test_plant_is_live_and_mutants_differ(item):
    view = sc.view_of(item)
    vals = sc._seq_vals(view)
    assert set(item.planted) <= set(vals), (item.name, item.label, sorted(vals)[:8])
    win = vals[item.winner]
    rest = [v for i, v in vals.items() if i not in item.planted]
    if item.equal == "bits":
        assert {bits(vals[i]) for i in item.planted} == {bits(win)}, (item.name, item.label)
        assert all(v > win for v in rest), (item.name, item.label)
    elif item.equal == "value":  # +0.0 first, then -0.0
        assert [bits(vals[i]) for i in item.planted] == [bits(0.0), bits(-0.0)], item.name
        assert all(v > 0 for v in rest), (item.name, item.label)
    elif item.equal == "band":
        assert all(abs(vals[i] - win) <= 3 * REV_EPS for i in item.planted), item.name
        assert len({bits(vals[i]) for i in item.planted}) > 1, item.name
        assert all(v > win + 1e-3 for v in rest), (item.name, item.label)
        assert sc.fold_edge_distance(view) > 1e-12, (item.name, sc.fold_edge_distance(view))
    else:  # "takes": the fold's last takes are the planted indices, in order
        assert item.equal == "takes"
        takes = []
        for hi in range(1, len(view.seq) + 1):
            cur = sc.select(type(view)(**{**vars(view), "seq": view.seq[:hi]}))
            if cur >= 0 and (not takes or takes[-1] != cur):
                takes.append(cur)
        assert tuple(takes[-len(item.planted):]) == item.planted, (item.name, takes)
        assert item.planted[0] % 64 == 63 and item.planted[1] == item.planted[0] + 1
    if len(item.planted) > 1:
        assert len(item.mutants) >= 1, item.name
    assert sc.select(view) == item.winner, (item.name, item.label, sc.select(view))
    for name in item.mutants:
        got = sc.MUTANTS[name](view)
        assert got != item.winner, (item.name, item.label, name)
        assert got in item.planted, (item.name, item.label, name, got)


def test_the_walk_positions_of_the_plants():
    """The declared seam of an item is the seam its planted positions sit on."""
    for it in ALL:
        pos = [i - it.lane0 for i in it.planted]
        lanes = [p % it.nt for p in pos]
        if it.kind == "leaving_dblmax":
            continue
        if it.seam == "dpp":
            lo, hi = lanes
            assert pos[0] // it.nt == pos[1] // it.nt and lo // 64 == hi // 64, it.name
            assert (lo % 64, hi % 64) in sc.DPP_PAIRS, it.name
        elif it.seam == "wave":
            assert pos[1] == pos[0] + 1 and pos[1] % 64 == 0 and pos[1] < it.nt == 256, it.name
        elif it.seam == "stride":
            assert any(b - a == it.nt for a in pos for b in pos) or it.kind == "pivot_row", it.name
            assert pos[0] // it.nt < pos[-1] // it.nt, it.name
            # a planted index other than the winner sits in a lower lane, a round later
            assert any(ln < lanes[0] for ln in lanes[1:]), it.name
        elif it.seam == "partial":
            assert pos[-1] // it.nt > pos[0] // it.nt and lanes[-1] < lanes[0], it.name
        elif it.seam == "window":
            assert it.engine == "revised" and pos[0] // 64 < pos[-1] // 64, it.name
        else:
            assert it.seam == "lane63" and pos[0] % 64 == 63, it.name


def test_dblmax_items_hold_the_sentinel_below_the_seam():
    found = 0
    for it in sc.items("primal"):
        if it.kind != "leaving_dblmax":
            continue
        found += 1
        T, lo = it.T, it.dblmax_row
        e = int(np.argmin(T[0, :-1]))
        ratios = {i: T[i, -1] / T[i, e] for i in range(1, T.shape[0]) if T[i, e] > 1e-9}
        assert ratios[lo] == DBL_MAX and min(ratios) == lo and it.winner == lo + 1
        assert min(ratios.values()) == ratios[it.winner]
    assert found == 3


# ------------------------------------------------------------------------------ the oracle
PRIMAL_STATUS = {"optimal": 0, "unbounded": 1, "limit": 5}
REV_STATUS = {"optimal": 0, "unbounded": 1, "infeasible_basis": 2, "limit": 5}


@pytest.mark.parametrize("item", sc.items("primal"), ids=[i.name for i in sc.items("primal")])
def test_primal_oracle_takes_the_winner_and_agrees_with_python(oracle, item):
    ref = sc.primal_ref(oracle, item)
    assert ref["pivots"] > item.at, item.name
    row, col = ref["log"][item.at]
    got = col if item.kind == "entering" else row
    assert got == item.winner, (item.name, item.label, got)
    p = sc.py_primal(item.T)
    assert PRIMAL_STATUS[p.solve(sc.PRIMAL_PIVOTS)] == ref["status"]
    assert p.log == [tuple(v) for v in ref["log"][:ref["pivots"]].tolist()]
    assert np.array(p.t).tobytes() == ref["T"].tobytes(), item.name


@pytest.mark.parametrize("item", sc.items("revised"), ids=[i.name for i in sc.items("revised")])
def test_revised_oracle_takes_the_winner_and_agrees_with_python(oracle, item):
    from ref_py import PyRevised
    ref = sc.revised_ref(oracle, item)
    assert ref["iterations"] > item.at, item.name
    row, enter, _ = ref["log"][item.at]
    got = enter if item.kind == "enter_fold" else row
    assert got == item.winner, (item.name, item.label, got)
    probe = sc.revised_probe(item)
    assert (probe["leaving"], probe["entering"]) == (row, enter), item.name
    p = PyRevised(*item.model)
    assert item.at + 1 < sc.REV_CAP
    assert REV_STATUS[p.solve(sc.REV_CAP)] == ref["status"]
    assert p.log == [tuple(v) for v in ref["log"].tolist()]
    assert np.array(p.Binv).tobytes() == ref["Binv"].tobytes(), item.name
    assert p.basic == ref["basis"].tolist()


@pytest.mark.parametrize("item", sc.items("bb"), ids=[i.name for i in sc.items("bb")])
def test_bb_oracle_takes_the_winner_and_agrees_with_python(oracle, item):
    import ref_py_bb as rb
    ref = sc.bb_ref(oracle, item)
    assert len(ref["records"]) == 3 and ref["records"][1]["status"] == 0, (item.name, ref["records"])
    assert len(ref["trace"]) <= 16, (item.name, ref["trace"])
    assert sc.bb_observed(ref, item) == sc.bb_expected(item), (item.name, item.label, ref["trace"])
    bb = rb.BranchAndBound(item.nv, sc.BB_CAP)
    p = bb.Execute([list(map(float, row)) for row in item.T.tolist()])
    assert (ref["status"] == 6) == p["capped"] and ref["processed"] == p["processed"]
    assert ref["pop_order"] == bb.pop_order and ref["records"] == bb.records
    assert ref["trace"] == bb.trace, item.name
    assert bits(ref["z"]) == bits(p["z"]) and ref["found"] == (p["x"] is not None)
    if item.kind == "pivot_row":  # the other row would give the other column
        c = sc.bb_child(item)
        assert c.child[-1][1] == -2.0 and c.child[-1][2] == 0.0, c.child[-1]


def test_bb_fractions_survive_the_rounding(oracle):
    """Every entry of every B&B root is exact at 4 decimals: RoundTableau leaves the roots alone."""
    for it in sc.items("bb"):
        assert oracle.bb_round_tableau(it.T).tobytes() == it.T.tobytes(), it.name


# ------------------------------------------------------------------------------ forms, coverage
def test_every_item_lands_in_the_form_it_declares():
    from lpr_381_group_v22_amd import revised_batch as rb
    for it in ALL:
        if it.engine == "primal":
            rows, cols = it.T.shape
            fp = rows * (cols + 1)
            want = 0 if fp <= 2016 else (1 if fp <= 20352 else 2)
            assert rows <= 1024 and cols <= 2048
            assert sc.primal_form(rows, cols) == want == it.form, it.name
        elif it.engine == "revised":
            assert rb.pick_form(it.m, it.n) == it.form, it.name
            assert len(it.model[0]) == it.n and len(it.model[1]) == it.m
        else:
            from test_bb_batch_gpu import form_of
            assert form_of(it.T, sc.BB_CAP) == sc.bb_form(it.T) == it.form, it.name
        assert it.nt == (64 if it.form == 0 else 256)
    from lpr_381_group_v22_amd import revised_batch as rb
    assert 8 * rb.footprint(64, 1) > rb.MAX_LDS_W  # no ratio window seam in form W


def test_walks_are_as_long_as_the_issue_asks():
    for it in ALL:
        if it.engine == "primal" and it.kind == "entering":
            assert it.T.shape[1] - 1 > 2 * it.nt, it.name
        elif it.engine == "primal":
            assert it.T.shape[0] > 2 * it.nt + 1, it.name
        elif it.engine == "revised":
            assert (it.n >= 128 and it.kind == "enter_fold") or it.m >= 130, it.name
        elif it.kind == "bv":
            assert it.nv >= (70 if it.form == 0 else 260), it.name
        elif it.kind in ("dual_row", "primal_row", "primal_first0", "pivot_row"):
            assert it.T.shape[0] + 1 > it.nt, it.name
        else:
            assert it.T.shape[1] - 1 > it.nt, it.name


def test_coverage_table():
    forms, seams = sc.coverage_cells()
    assert forms == sc.EXPECTED_FORM_CELLS, set(forms) ^ set(sc.EXPECTED_FORM_CELLS)
    assert seams == sc.EXPECTED_SEAM_CELLS, set(seams) ^ set(sc.EXPECTED_SEAM_CELLS)
    assert {eng: tuple(sorted({it.kind for it in sc.items(eng)})) for eng in sc.KINDS} == \
        {eng: tuple(sorted(k)) for eng, k in sc.KINDS.items()}
    # every seam class and every mutant is used somewhere
    assert {it.seam for it in ALL} == set(sc.SEAMS)
    assert {m for it in ALL for m in it.mutants} == set(sc.MUTANTS)
    count = {}
    for it in ALL:
        count[(it.engine, it.seam)] = count.get((it.engine, it.seam), 0) + 1
    print(sorted(count.items()))
    assert sum(count.values()) == len(ALL) and all(math.isfinite(v) for v in count.values())


def test_tie_stats_keeps_its_return_value_with_a_probe():
    """The probe only listens: the instrumented fold returns what it returned without one."""
    import revised_batch_cases as rc
    for mdl in rc.tie_models()[:8]:
        probe = []
        assert rc.tie_stats(mdl, 50, probe=probe) == rc.tie_stats(mdl, 50)
        assert [p["it"] for p in probe] == list(range(len(probe)))
