"""GPU tests of the primal seam items (tests/primal_seam_cases.py) on the single-handle primal
paths: the cache-resident path (k_small_heads; the default and forced), k_pivot_fused, k_bootstrap /
k_pivot_head, the step entry points (k_select) and the loop heads of the K-pivot paths -- in place
and two-stream, each also spread over the chip and with memory-side hand-offs, the two-stream form
also on the condensed layout (DESIGN.md sections 4, 4b, 4c).  Every item runs with max_pivots =
at + 2 and is compared with the oracle run on it alone: the planted pivot first, with a message
that names the seam (the C# takes the first of the tied candidates, and a reduction that is wrong
on one lane, wave, workgroup, trip or collector seam changes exactly that entry), then status,
pivot count, pivot log, basis and every byte of the tableau.  No item is skipped or filtered."""
import numpy as np
import pytest

import primal_seam_cases as pc

pytestmark = pytest.mark.gpu


def seam_of(it, what):
    return (f"{it.name} [{what}]: {it.kind} at pivot {it.at}, {it.label}: the tie at {it.planted} "
            f"must go to {it.winner}")


def run_items(engine, oracle, its, variant, block, what, want_block):
    """Every item through lpr_primal_solve; the planted pivots of all items are judged first."""
    from lpr_381_group_v22_amd import Tableau
    wrong_seams, wrong_rest = [], []
    for it in its:
        ref = pc.reference(oracle, it)
        tab = Tableau.from_array(engine, it.T, it.basis)
        res = tab.solve(max_pivots=it.at + 2, variant=variant,
                        block=it.block if block is None else block)
        log = tab.pivot_log().tolist()
        if it.winner < 0:
            seam_ok = res.status == 1 and res.pivots == it.at
        else:
            seam_ok = len(log) > it.at and log[it.at][1 if it.kind == "entering" else 0] == it.winner
        if not seam_ok:
            wrong_seams.append(seam_of(it, what) + f"; status {res.status}, log {log[it.at:]}")
        elif not (res.status == ref.status and res.pivots == ref.pivots and log == ref.log and
                  tab.basis().tolist() == ref.basis and tab.read().tobytes() == ref.tbytes):
            wrong_rest.append((it.name, what, res.status, ref.status, res.pivots, ref.pivots))
        assert res.block == (it.block if want_block is None else want_block), (it.name, res.block)
        tab.destroy()
    assert not wrong_seams, "\n".join(wrong_seams)
    assert not wrong_rest, wrong_rest


@pytest.mark.parametrize("variant,block", pc.PATHS["small"], ids=["default", "forced"])
def test_cache_resident_path_seams(engine, oracle, variant, block):
    run_items(engine, oracle, pc.items("small"), variant, block, f"small {variant:#x}", 16)


def test_fused_path_seams(engine, oracle):
    (variant, block), = pc.PATHS["fused"]
    run_items(engine, oracle, pc.items("fused"), variant, block, "fused", 1)


def test_one_pivot_path_seams(engine, oracle):
    (variant, block), = pc.PATHS["onepivot"]
    run_items(engine, oracle, pc.items("onepivot"), variant, block, "one-pivot", 1)


def test_step_entry_point_seams(engine, oracle):
    """lpr_select_entering / lpr_select_leaving (k_select) on the tableau as uploaded."""
    from lpr_381_group_v22_amd import Tableau
    wrong = []
    for it in pc.items("select"):
        T = np.ascontiguousarray(it.T)
        e_ref = oracle.find_entering(T)
        tab = Tableau.from_array(engine, it.T, it.basis)
        e = tab.select_entering()
        got = e if it.kind == "entering" else tab.select_leaving(e_ref)
        want = e_ref if it.kind == "entering" else oracle.find_leaving(T, e_ref)
        assert want == it.winner, it.name
        if e != e_ref or got != it.winner:
            wrong.append(seam_of(it, "k_select") + f"; got column {e}, {it.kind} {got}")
        assert tab.read().tobytes() == it.T.tobytes(), it.name
        tab.destroy()
    assert not wrong, "\n".join(wrong)


K_IDS = ["inplace", "inplace-spread", "inplace-memside", "two-stream", "two-stream-spread",
         "two-stream-memside", "two-stream-condensed"]


@pytest.mark.parametrize("variant,block", pc.PATHS["kpivot"], ids=K_IDS)
def test_k_pivot_heads_seams(engine, oracle, variant, block):
    """Condensed: the winner is by ORIGINAL column index; a shape the condensed layout cannot hold
    (more than 32 767 columns) runs on the full layout under the same options."""
    run_items(engine, oracle, pc.items("kpivot"), variant, block, f"K-pivot {variant:#x}", None)
