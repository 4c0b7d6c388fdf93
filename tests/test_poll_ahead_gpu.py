"""GPU tests of the K-pivot driver's polls ahead of the queue's end (csrc/overlap_driver.hip,
solve_overlapped; the snapshots of csrc/overlap_kernels.hip): in a batch of nb steps the host reads a
snapshot of the control block `lead` steps before the end and queues the next batch behind the steps
still running.  No kernel changed, so nothing a solve leaves may change: status, pivot count, pivot
log, basis and every byte of the tableau against the oracle, wherever the end of the solve falls
relative to a snapshot, under pivot limits, across a re-allocation of the log, and with the event
timing on.  LPR_TEST_POLL_LEAD (read when a tableau handle is created) fixes `lead` in steps.

The shapes and references are those of ov_step_cases.py; `batch` is given in pivots, so a batch is
batch / block steps."""
import contextlib
import os

import pytest

import ov_step_cases as cs

pytestmark = pytest.mark.gpu

OV2, SEQ = 0x3008, 0x4008      # two streams / heads then an in-place sweep, forced on small shapes
VARIANTS = [OV2, SEQ]
IDS = ["two-stream", "in-place"]
BLOCKS = (4, 16)
STEPS = (2, 3, 5, 8)           # steps per batch (batch = steps x block)
LEADS = (1, 2, 64)             # the hook's value; 64 is clipped to nb / 2 by the driver
# (m, n, kind, pivots before the free-running call): the full solves of ov_step_cases (50 / 43,
# 121, 33 / 7 pivots) and, so that every step behind a snapshot four steps deep meets an end, the
# 121-pivot solve again after a first call of 5 pivots
FULL = [(40, 60, "optimal", 0), (40, 60, "unbounded", 0), (300, 700, "optimal", 0),
        (300, 700, "optimal", 5), (8, 3000, "optimal", 0), (8, 3000, "unbounded", 0)]


@contextlib.contextmanager
def hooks(lead, log_cap=None):
    """The test hooks a tableau handle reads when it is created."""
    env = {"LPR_TEST_POLL_LEAD": str(lead)}
    if log_cap:
        env["LPR_TEST_LOG_CAP"] = str(log_cap)
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def lead_of(hook, nb):
    """The driver's rule: the hook's value, at least 1, at most half the batch."""
    return max(1, min(hook, nb // 2))


def run_legs(engine, oracle, m, n, kind, legs, variant, block, nb, lead, log_cap=None):
    """`legs` (0 = no limit) on one handle; the state after each against the oracle's."""
    from lpr_381_group_v22_amd import Tableau
    T0, b0, states = cs.reference(oracle, m, n, kind, legs)
    with hooks(lead, log_cap):
        tab = Tableau.from_array(engine, T0, b0)
    total = 0
    for leg, (st, piv, log, basis, tbytes) in zip(legs, states):
        res = tab.solve(max_pivots=leg, block=block, batch=nb * block, variant=variant)
        total += piv
        tag = (m, n, kind, legs, leg, hex(variant), block, nb, lead)
        assert res.block == block, tag
        assert (res.status, res.pivots, res.total_pivots) == (st, piv, total), \
            (tag, res.status, res.pivots, res.total_pivots, st, piv, total)
        if st == 5:
            assert res.pivots == leg, tag  # a limit is met exactly
        assert tab.pivot_log(1 << 16).tolist()[total - piv:] == log, tag
        assert tab.basis().tolist() == basis, tag
        assert tab.read().tobytes() == tbytes, tag
    tab.destroy()
    return states[-1][0]


def end_classes(pivots, block, nb, lead):
    """Where the end of a free-running call of `pivots` pivots falls.  The heads of step e =
    pivots // block (counted from 0 within the call) are the ones that look for pivot number
    `pivots` and find the end, in both forms.  Batch b is steps [b * nb, (b + 1) * nb) and its
    snapshot shows the state after the steps before (b + 1) * nb - lead."""
    e = pivots // block
    b, r = divmod(e, nb)
    out = set()
    if r == nb - lead - 1:
        out.add("snapshot-step")            # the last step the snapshot shows: it shows the end
    if r >= nb - lead:
        out.add(("behind", lead, r - (nb - lead)))  # in the j-th of the `lead` steps behind it
    if r == 0:
        out.add("batch-first")
    if b == 0 and r < nb - lead:
        out.add("before-first-snapshot")
    return out


def test_grid_puts_the_end_on_every_side_of_a_snapshot(oracle):
    """The grid of the free-running test below, from the oracle's pivot counts alone."""
    seen = set()
    for m, n, kind, before in FULL:
        legs = (before, 0) if before else (0,)
        states = cs.reference(oracle, m, n, kind, legs)[2]
        assert len(states) == len(legs)
        for block in BLOCKS:
            for nb in STEPS:
                for hook in LEADS:
                    seen |= end_classes(states[-1][1], block, nb, lead_of(hook, nb))
    want = {"snapshot-step", "batch-first", "before-first-snapshot"}
    for lead in {lead_of(h, nb) for h in LEADS for nb in STEPS}:
        want |= {("behind", lead, j) for j in range(lead)}
    assert want <= seen, sorted(map(str, want - seen))


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_free_running_solves_vs_oracle(engine, oracle, variant, block):
    """Solves to the end, optimal and unbounded: the end is found in the step a snapshot shows last,
    in each of the steps queued behind one, in the first step of a batch and before the first
    snapshot (test_grid_puts_the_end_on_every_side_of_a_snapshot)."""
    for m, n, kind, before in FULL:
        legs = (before, 0) if before else (0,)
        for nb in STEPS:
            for hook in sorted({lead_of(h, nb) for h in LEADS}):
                st = run_legs(engine, oracle, m, n, kind, legs, variant, block, nb, hook)
                assert st == (0 if kind == "optimal" else 1)
    # the value the driver takes when the hook is clipped (64 -> nb / 2), once
    run_legs(engine, oracle, 300, 700, "optimal", (0,), variant, block, 8, 64)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_pivot_limits_on_one_handle_vs_oracle(engine, oracle, variant, block):
    """Legs of 16, 23, 9 and 17 pivots on one handle: every limit is met exactly, total_pivots adds
    up, the state after every leg is the oracle's (so the sweep direction and the live buffer a call
    hands on are those of its final poll)."""
    for m, n in ((40, 60), (300, 700), (8, 3000)):
        for nb in STEPS:
            for hook in sorted({lead_of(h, nb) for h in LEADS}):
                run_legs(engine, oracle, m, n, "optimal", cs.LEGS, variant, block, nb, hook)


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_log_growth_behind_a_snapshot(engine, oracle, variant):
    """The log starts at 16 pairs and is re-allocated several times inside one call whose batches
    are two, three and five steps: the driver drains before it replaces the buffer, and no entry is
    dropped (run_legs compares the whole log)."""
    for block, nb, hook in ((4, 2, 1), (4, 5, 2), (16, 2, 1), (16, 3, 1), (16, 5, 2)):
        run_legs(engine, oracle, 300, 700, "optimal", (0,), variant, block, nb, hook, log_cap=16)
        run_legs(engine, oracle, 300, 700, "optimal", cs.LEGS, variant, block, nb, hook, log_cap=16)


def timed_counts(engine, T0, b0, variant, block, nb, lead, stride, limit):
    from lpr_381_group_v22_amd import Tableau
    with hooks(lead):
        tab = Tableau.from_array(engine, T0, b0)
    res = tab.solve(max_pivots=limit, time_kernels=stride, block=block, batch=nb * block,
                    variant=variant)
    out = (res.status, res.pivots, tab.kernel_stats()[0], tab.step_stats()[0])
    tab.destroy()
    return out


def counts_by_rule(variant, block, nb, stride, pivots, limit):
    """(launches, steps) the driver's rule counts in a first call on a handle that applies `pivots`
    pivots.  The steps that sweep a full block are the call's steps first .. first + pivots // block
    - 1 (first = 1 with two streams, whose step 0 only decides).  Step k of a BATCH is sampled when k
    is a multiple of the stride; a sampled full step counts as a launch; its window runs to the next
    sampled step of the batch or to the batch's end, and counts its steps if they are all full.
    Batches are nb steps; under a pivot limit a batch is cut to the blocks the limit still allows,
    plus one step in the call's first batch (the step that only decides)."""
    first = 1 if variant == OV2 else 0
    full_end = first + pivots // block
    batches, step = [], 0
    while step < full_end + 1:
        n = nb
        if limit:
            left = limit - min(limit, max(0, step - first) * block)
            n = min(nb, -(-left // block) + (1 if step == 0 else 0))
        if n < 1:
            break
        batches.append((step, n))
        step += n
    launches = steps = 0
    for g0, n in batches:
        for k in range(0, n, stride):
            if first <= g0 + k < full_end:
                launches += 1
                kn = min(k + stride, n)
                if g0 + kn <= full_end:
                    steps += kn - k
    return launches, steps


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_event_counts_do_not_depend_on_the_snapshots(engine, oracle, variant, stride):
    """opts.time_kernels with batches of a few steps, so that the events of a batch are read while
    later batches are queued or running: the launches and the step windows counted are those of
    the driver's rule (counts_by_rule: the rule before the snapshots, batch by batch), with every
    lead.  With stride 1 the rule counts every sweep that applied a full block, and its window,
    once: the counts are the full blocks applied, and those of the same call made as ONE batch of
    64 steps (the call ends inside it).  With stride 2 the sampled steps and the ends of the windows
    are taken per batch, so the counts are those of the one-batch call only while every batch is an
    even number of steps: asserted for the free-running call with batches of 2 and 8.  (A pivot
    limit cuts batches short: 100 pivots in blocks of 4, in place, are 12 batches of 2 steps and one
    of ONE step, whose window of one step counts, 25 steps timed; as a single batch they are 26
    steps, the last one idle, and the window [24, 26) that holds it does not count, 24.  The rule is
    kept as it was, so that the benchmark's launches / steps_timed stay comparable.)"""
    T0, b0, states = cs.reference(oracle, 300, 700, "optimal", (0,))
    pivots = states[-1][1]
    for block in BLOCKS:
        for limit in (0, 100):   # to the end (121 pivots) / a limit inside a block
            done = min(pivots, limit) if limit else pivots
            head = ((5 if limit else 0), done)
            one = timed_counts(engine, T0, b0, variant, block, 64, 1, stride, limit)
            assert one == head + counts_by_rule(variant, block, 64, stride, done, limit), one
            if stride == 1:
                assert one[2:] == (done // block, done // block), (block, limit, one)
            for nb in STEPS:
                for hook in sorted({lead_of(h, nb) for h in LEADS}):
                    got = timed_counts(engine, T0, b0, variant, block, nb, hook, stride, limit)
                    tag = (hex(variant), block, limit, nb, hook, stride, got, one)
                    assert got == head + counts_by_rule(variant, block, nb, stride, done, limit), tag
                    if stride == 1 or (limit == 0 and nb % 2 == 0):
                        assert got == one, tag
