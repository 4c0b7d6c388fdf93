"""GPU tests of the device text formatter (lpr_text_*, lpr_batch_trace_text; DESIGN.md section
25): every block the device writes is the bytes of the host ``Format`` after its title line --
cell by cell at the edges of the {v:F3} rule (also against tests/ref_py_text.py), on random bit
patterns, at the seams of the kernels' work split, and for every kept record of traced batches in
every form -- and the calls refuse what the ABI says they refuse."""
import ctypes as C

import numpy as np
import pytest

import batch_trace_cases as tc
import text_cases

pytestmark = pytest.mark.gpu


def host_body(T, nvars):
    from lpr_381_group_v22_amd.table_iteration_formater import Format, title_line
    return Format(np.asarray(T), nvars, "q")[len(title_line("q")):]


def device_bodies(engine, tableaux, nvars):
    from lpr_381_group_v22_amd.table_iteration_formater import format_bodies
    return format_bodies(tableaux, nvars, engine=engine)


# ------------------------------------------------------------------- cells
def test_cells_at_the_edges_of_the_rule(engine):
    from ref_py_text import py_fixed
    tabs = text_cases.cell_tableaux()
    assert {t.shape[1] for t in tabs} == set(range(1, 9)) and all(t.shape[0] == 1 for t in tabs)
    got = device_bodies(engine, tabs, 0)
    for T, body in zip(tabs, got):
        assert body == host_body(T, 0), [float(v).hex() for v in T[0]]
        cells = body.split("\r\n")[2].split("\t")[1:-1]
        assert cells == [py_fixed(float(v), 3) for v in T[0]], [float(v).hex() for v in T[0]]


def test_random_bit_patterns(engine):
    T = text_cases.random_bits_tableau()
    assert T.shape == (400, 500)
    got = device_bodies(engine, [T], 7)[0]
    want = host_body(T, 7)
    if got != want:  # name the first cell that differs
        g, w = got.split("\r\n"), want.split("\r\n")
        for i, (a, b) in enumerate(zip(g, w)):
            if a != b:
                ca, cb = a.split("\t"), b.split("\t")
                j = next(q for q in range(min(len(ca), len(cb))) if ca[q] != cb[q])
                raise AssertionError((i, j, ca[j], cb[j], float(T[max(i - 2, 0), j - 1]).hex()))
    assert got == want


# ------------------------------------------------------------------- seams
def test_seams_in_one_call(engine):
    blocks = text_cases.seam_blocks()
    got = device_bodies(engine, [T for T, _ in blocks], [nv for _, nv in blocks])
    assert len(got) == len(blocks)
    for q, ((T, nv), body) in enumerate(zip(blocks, got)):
        assert body == host_body(T, nv), (q, T.shape, nv)


@pytest.mark.parametrize("q", [0, 4, 6, 16, 28, 50])
def test_one_block_alone(engine, q):
    """count = 1: the same block without neighbours."""
    T, nv = text_cases.seam_blocks()[q]
    assert device_bodies(engine, [T], nv) == [host_body(T, nv)]


def test_offsets_and_partial_reads(engine):
    from lpr_381_group_v22_amd import _native as N
    from lpr_381_group_v22_amd.table_iteration_formater import format_device
    blocks = text_cases.seam_blocks()[:12]
    want = [host_body(T, nv) for T, nv in blocks]
    text = format_device([T for T, _ in blocks], [nv for _, nv in blocks], engine=engine)
    assert text.Count == len(blocks) and text.Bytes == sum(len(w) for w in want)
    assert text.offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert text.KernelMs > 0.0
    at, n = int(text.offsets[3]) + 5, 40
    out = np.zeros(n, dtype=np.uint8)
    N.check(N.lib.lpr_text_read(text._h, at, n, N._ptr(out, C.c_uint8)), "lpr_text_read")
    assert out.tobytes().decode("ascii") == "".join(want)[at:at + n]
    text.destroy()


def test_many_rows_cross_the_scan_tiles(engine):
    """More rows than one scan tile (2048) and than one pass of the top scan (256 tiles): 600 000
    one-cell rows in three blocks, the expected text built from the three distinct lines."""
    from lpr_381_group_v22_amd.table_iteration_formater import F3
    vals = [1.5, -20.25, 1e15]
    rows = 200000
    tabs = [np.full((rows, 1), v) for v in vals]
    got = device_bodies(engine, tabs, 0)
    for v, body in zip(vals, got):
        lines = body.split("\r\n")
        assert lines[0] == "-" * 80 and lines[1] == "Table\tRHS" and lines[-1] == ""
        assert len(lines) == rows + 3
        cell = F3(v)
        assert lines[2] == "Z\t" + cell + "\t"
        assert lines[3:-1] == [f"{i}\t{cell}\t" for i in range(1, rows)]


def test_more_wave_tasks_than_one_grid_holds(engine):
    """A pass launches at most 65 536 workgroups of four waves and its waves stride over the
    tasks: 262 144 + 7 one-cell blocks (a wave task each) make some waves take a second task."""
    count = 65536 * 4 + 7
    vals, nvs = [0.5, -1234.5675, 1e15], [0, 1, 2]
    want = {(v, nv): host_body(np.array([[v]]), nv) for v in vals for nv in nvs}
    pick_v = [vals[(k * 7) % 3] for k in range(count)]
    pick_n = [nvs[(k // 3) % 3] for k in range(count)]
    flat = np.asarray(pick_v).reshape(count, 1, 1)
    got = device_bodies(engine, list(flat), pick_n)
    assert len(got) == count
    for k in (0, 1, 262143, 262144, 262145, count - 1):
        assert got[k] == want[(pick_v[k], pick_n[k])], k
    assert got == [want[(v, nv)] for v, nv in zip(pick_v, pick_n)]


# ------------------------------------------------------------------- traced batches
def _batches():
    plain = [(n, c) for n, c in tc.all_cases() if not n.startswith("form_")]
    return [("cases", [c for _, c in plain], tc.TRACE_CAP, tc.CAP),
            ("forms", [c for _, c in tc.form_models()], tc.SHAPE_PIVOTS + 2, tc.SHAPE_PIVOTS)]


def _traced(engine, cases, trace_cap, max_pivots, variant):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    b = PrimalSimplexBatch(tc.models_of(cases), engine=engine, log_cap=tc.CAP, trace_cap=trace_cap)
    b.Solve(max_pivots=max_pivots, variant=variant)
    return b


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_traced_batch_texts(engine, which, variant):
    name, cases, cap, piv = _batches()[which]
    b = _traced(engine, cases, cap, piv, variant)
    seen = set()
    for k in range(b.Count):
        seen.add(b.Status[k])
        assert b.IterationSnapshotsDevice(k) == b.IterationSnapshots(k), (name, variant, k)
        if b.Iterations[k] + 1 > cap:  # a tie-heavy case: both refuse a console text with gaps
            for console in (b.ConsoleText, b.ConsoleTextDevice):
                with pytest.raises(ValueError, match=f"TraceCap keeps {cap}"):
                    console(k)
        else:
            assert b.ConsoleTextDevice(k) == b.ConsoleText(k), (name, variant, k)
    assert b.all_snapshot_texts() == [b.IterationSnapshots(k) for k in range(b.Count)]
    if which == 0:
        assert {tc.OPTIMAL, tc.UNBOUNDED} <= seen
    b.destroy()


def test_record_cap_limit_and_second_solve(engine):
    import lp_cases
    cases = [lp_cases.readme_option1(), tc.cap_lp(), tc.zero_pivot_lp(), lp_cases.sample_option1()]
    b = _traced(engine, cases, tc.SMALL_TRACE_CAP, 2, 0)
    assert b.Status[1] == tc.LIMIT
    text = b.FormatTrace()
    assert b.FormatTrace() is text  # kept until the next Solve
    fb = text.first_block.tolist()
    for k in range(b.Count):
        kept = min(1 + b.Iterations[k], tc.SMALL_TRACE_CAP)
        assert fb[k + 1] - fb[k] == kept + (1 if b._ended(k) else 0), k
        assert b.IterationSnapshotsDevice(k) == b.IterationSnapshots(k), k
    assert not b._ended(1)  # stopped by max_pivots: no final block
    b.Solve(max_pivots=tc.CAP)
    fresh = b.FormatTrace()
    assert fresh is not text and fresh.first_block.tolist() != fb
    assert b.Iterations[1] + 1 > tc.SMALL_TRACE_CAP
    for k in range(b.Count):
        snaps = b.IterationSnapshotsDevice(k)
        assert snaps == b.IterationSnapshots(k), k
        assert len(snaps) == min(1 + b.Iterations[k], tc.SMALL_TRACE_CAP) + 1
    with pytest.raises(ValueError, match="TraceCap keeps 3"):
        b.ConsoleText(1)
    with pytest.raises(ValueError, match="TraceCap keeps 3"):
        b.ConsoleTextDevice(1)
    assert b.ConsoleTextDevice(2) == b.ConsoleText(2)
    b.destroy()


def test_negative_zero_and_read_only(engine):
    from lpr_381_group_v22_amd import PrimalSimplexBatch
    T, basis = tc.negative_zero_tableau()
    b = PrimalSimplexBatch.from_tableaux([T], [basis], engine=engine, trace_cap=8)
    b.Solve(max_pivots=tc.CAP)
    before = (b.status_arrays(), b.GetFinalTableau(0).tobytes(), b.trace_packed()[0].tobytes())
    snaps = b.IterationSnapshotsDevice(0)
    assert snaps == b.IterationSnapshots(0)
    assert not any("-0.000" in s for s in snaps)
    assert b.ConsoleTextDevice(0) == b.ConsoleText(0)
    after = (b.status_arrays(), b.GetFinalTableau(0).tobytes(), b.trace_packed()[0].tobytes())
    for x, y in zip(before[0], after[0]):
        assert x.tobytes() == y.tobytes()
    assert before[1:] == after[1:]
    b.destroy()


def test_text_outlives_its_batch(engine):
    import lp_cases
    b = _traced(engine, [lp_cases.readme_option1(), tc.unbounded_later_lp()], 16, tc.CAP, 0)
    from lpr_381_group_v22_amd.primal_batch import snapshots_from_bodies
    want = [b.IterationSnapshots(k) for k in range(b.Count)]
    assert b.Status == [tc.OPTIMAL, tc.UNBOUNDED]
    text = b.FormatTrace()
    about = [(b.Shape(k)[2], b.Status[k], b.FinalZ[k], b.SolutionVector[k]) for k in range(b.Count)]
    b._text = None
    b.destroy()
    # read only now: the handle holds the text, nothing of the batch
    fb = text.first_block.tolist()
    for k, (n, st, z, x) in enumerate(about):
        bodies = [text.block(i) for i in range(fb[k], fb[k + 1])]
        assert snapshots_from_bodies(bodies[:-1], n, st, bodies[-1], z, x) == want[k], k
    text.destroy()


# ------------------------------------------------------------------- ABI errors
def _err():
    from lpr_381_group_v22_amd import _native as N
    return N.lib.lpr_last_error().decode()


def test_abi_errors(engine):
    import lp_cases
    import lpr_381_group_v22_amd as pkg
    from lpr_381_group_v22_amd import PrimalSimplexBatch, _native as N
    lib = N.lib
    h = C.c_void_p()
    # an untraced batch
    b = PrimalSimplexBatch(tc.models_of([lp_cases.readme_option1()]), engine=engine)
    assert lib.lpr_batch_trace_text(b._h, None, C.byref(h)) == N.LPR_BAD_ARGUMENT
    assert "lpr_batch_trace_text" in _err() and "not traced" in _err()
    b.destroy()
    # a NULL out
    b = PrimalSimplexBatch(tc.models_of([lp_cases.readme_option1()]), engine=engine, trace_cap=4)
    assert lib.lpr_batch_trace_text(b._h, None, None) == N.LPR_BAD_ARGUMENT
    assert "lpr_batch_trace_text" in _err() and "null out" in _err()
    b.destroy()
    rows = np.array([1, 2, 0], dtype=np.int32)
    cols = np.array([1, 2, 3], dtype=np.int32)
    nv = np.array([0, 0, 0], dtype=np.int32)
    data = np.zeros(16)
    args = lambda r, c, n: (N._ptr(r, C.c_int32), N._ptr(c, C.c_int32), N._ptr(n, C.c_int32),
                            N._ptr(data, C.c_double))
    assert lib.lpr_text_format_tableaux(engine._h, 3, *args(rows, cols, nv), None) == \
        N.LPR_BAD_ARGUMENT
    assert "lpr_text_format_tableaux" in _err()
    # a bad shape at index k
    assert lib.lpr_text_format_tableaux(engine._h, 3, *args(rows, cols, nv), C.byref(h)) == \
        N.LPR_BAD_ARGUMENT
    assert "lpr_text_format_tableaux: block 2 is 0 x 3" in _err()
    rows[2], nv[1] = 1, -1
    assert lib.lpr_text_format_tableaux(engine._h, 3, *args(rows, cols, nv), C.byref(h)) == \
        N.LPR_BAD_ARGUMENT
    assert "block 1 is 2 x 2 with nvars -1" in _err()
    assert lib.lpr_text_format_tableaux(engine._h, 0, *args(rows, cols, nv), C.byref(h)) == \
        N.LPR_BAD_ARGUMENT
    assert "count=0" in _err()
    # a read beyond bytes
    nv[1] = 0
    N.check(lib.lpr_text_format_tableaux(engine._h, 3, *args(rows, cols, nv), C.byref(h)), "format")
    nbytes = C.c_int64()
    N.check(lib.lpr_text_info(h, None, C.byref(nbytes), None), "info")
    out = np.zeros(8, dtype=np.uint8)
    assert lib.lpr_text_read(h, nbytes.value - 4, 5, N._ptr(out, C.c_uint8)) == N.LPR_BAD_ARGUMENT
    assert "lpr_text_read: bytes [" in _err() and f"of a text of {nbytes.value} bytes" in _err()
    assert lib.lpr_text_read(h, nbytes.value - 4, 4, N._ptr(out, C.c_uint8)) == 0
    assert out[:4].tobytes() == b"0\t\r\n"
    assert lib.lpr_text_offsets_read(h, None) == N.LPR_BAD_ARGUMENT
    assert lib.lpr_text_destroy(h) == 0
    assert lib.lpr_text_destroy(None) == N.LPR_BAD_ARGUMENT
    # orphaned by lpr_engine_close: every call but destroy refuses; two handles destroyed in turn
    eng2 = pkg.Engine(0)
    h1, h2 = C.c_void_p(), C.c_void_p()
    for hh in (h1, h2):
        N.check(lib.lpr_text_format_tableaux(eng2._h, 3, *args(rows, cols, nv), C.byref(hh)), "fmt")
    eng2.close()
    blocks = C.c_int64()
    assert lib.lpr_text_info(h1, C.byref(blocks), None, None) == N.LPR_BAD_ARGUMENT
    assert "orphaned" in _err()
    assert lib.lpr_text_read(h2, 0, 1, N._ptr(out, C.c_uint8)) == N.LPR_BAD_ARGUMENT
    assert "orphaned" in _err()
    assert lib.lpr_text_destroy(h1) == 0 and lib.lpr_text_destroy(h2) == 0
