"""Branch & Bound instances for the parity tests (TEST ONLY).  Every instance goes through the
reference's own route (Program.cs option 3): model -> x_i <= 1 rows appended -> PrimalSimplexSolver
-> FinalTableau -> BranchAndBoundAdapter.SolveFromPrimal.

Provides: the product-route cases (all_bb_cases, primal_final_tableau), and the edge instances the
cases never reach (flag_room_cases, tall_cases, widest_lds_case, big_value_cases; edge_cases /
edge_case by name).  Constructed roots that tie a selection of the batched search exactly across a
lane, wave, stride or last-round seam are not here but in seam_cases.py (bb_items), built with the
same widening and heightening that leaves a root's basic columns alone."""
from __future__ import annotations

import numpy as np

import lp_cases
from ref_py import PyConstraint, parse_model_text, program_option1_constraints


def knapsack_sample():
    _, obj, cons, _ = parse_model_text(lp_cases.SAMPLE_MODEL)
    return obj, program_option1_constraints(len(obj), cons)


def random_binary_program(n: int, mcons: int, seed: int):
    """max c x, A x <= b, x binary (after the x_i <= 1 rows): small positive integers so that the
    LP relaxation is fractional and the 4-decimal rounding of the reference is exercised."""
    rng = np.random.RandomState(seed)
    c = rng.randint(1, 20, size=n).astype(float)
    A = rng.randint(1, 15, size=(mcons, n)).astype(float)
    b = np.floor(A.sum(axis=1) * rng.uniform(0.3, 0.6, size=mcons))
    cons = [PyConstraint(A[i].tolist(), "<=", float(b[i])) for i in range(mcons)]
    return c.tolist(), program_option1_constraints(n, cons)


def fractional_program(n: int, mcons: int, seed: int, big_m: float = 0.0):
    """Non-integer data: exercises Math.Round(x, 4) on values that are not short decimals.
    big_m > 0 appends the row  M x0 + x1 <= 0.6 M + 0.37  (entries >= 1e11 in the tableaux)."""
    rng = np.random.RandomState(seed)
    c = np.round(rng.uniform(1, 9, size=n), 3)
    A = np.round(rng.uniform(0.5, 7, size=(mcons, n)), 3)
    b = np.round(A.sum(axis=1) * rng.uniform(0.35, 0.65, size=mcons), 2)
    cons = [PyConstraint(A[i].tolist(), "<=", float(b[i])) for i in range(mcons)]
    if big_m:
        row = [0.0] * n
        row[0], row[1] = big_m, 1.0
        cons.append(PyConstraint(row, "<=", 0.6 * big_m + 0.37))
    return c.tolist(), program_option1_constraints(n, cons)


def huge_relaxation_value():
    """An instance (found by tools/fuzz_bb_gpu.py, seed 2955) where a child's relaxation puts
    1.1e15 into a decision variable: `(int)Math.Floor(v)` (:870-871) is then out of int's range and
    the bound of BOTH children becomes int.MinValue (x64 cvttsd2si)."""
    rng = np.random.RandomState(2955)
    n, mc = int(rng.randint(3, 14)), int(rng.randint(1, 6))
    gen = random_binary_program if rng.randint(0, 2) else fractional_program
    return gen(n, mc, int(rng.randint(0, 1 << 30)))


def all_bb_cases():
    cases = [("knapsack_sample", knapsack_sample())]
    for (n, mc, seed) in [(4, 1, 0), (5, 2, 1), (6, 2, 2), (8, 3, 3), (10, 2, 4), (7, 4, 5)]:
        cases.append((f"binary_{n}v{mc}c_s{seed}", random_binary_program(n, mc, seed)))
    for (n, mc, seed) in [(4, 2, 10), (6, 3, 11), (9, 2, 12)]:
        cases.append((f"frac_{n}v{mc}c_s{seed}", fractional_program(n, mc, seed)))
    cases.append(("huge_relaxation_value", huge_relaxation_value()))
    return cases


def primal_final_tableau(oracle, obj, cons):
    """Oracle PrimalSimplexSolver on the instance; returns (status, FinalTableau, n)."""
    o, A, ncoef, rel, rhs = lp_cases.flatten(obj, cons)
    T, basis = oracle.primal_build(o, A, rel, rhs, True, ncoef)
    st, piv, log = oracle.primal_solve(T, basis)
    return st, T, len(obj)


# ---- edge instances: shapes and magnitudes the cases above never reach ------------------------
# Each builder returns dicts  name, T (the root tableau), nvars, max_depth, cap (DFS node cap),
# tag (the edge it hits), and min_children (children the oracle's DFS must solve at that cap, so
# that the tree stays a real one).  tests/test_bb_edges_gpu.py runs them on the device,
# tests/test_bb_edge_cases.py checks on the oracle that each still hits its edge.

LD_ALIGN = 16
ELIMINATE_LDS_COLS = 36864   # kBBEliminateLdsMax / sizeof(int): widest align16(cols + max_depth)
ROWS_CAP_MAX = 65535         # rows + max_depth


def align16(x: int) -> int:
    return (x + LD_ALIGN - 1) // LD_ALIGN * LD_ALIGN


def legacy_flag_room(rows: int, cols: int, nvars: int, max_depth: int) -> int:
    """Bytes the -0.0 flags had when they sat in the score row behind z and the nvars decision
    values: 8 (ld - 1 - nvars).  The flags need rows_cap = rows + max_depth bytes."""
    return 8 * (align16(cols + max_depth) - 1 - nvars)


def _edge(name, T, nvars, max_depth, tag, min_children, cap=None):
    cap = min(20, max_depth) if cap is None else cap
    return dict(name=name, T=np.ascontiguousarray(T, dtype=np.float64), nvars=nvars,
                max_depth=max_depth, cap=cap, tag=tag, min_children=min_children)


def _product_root(oracle, gen, *args, **kw):
    st, T, n = primal_final_tableau(oracle, *gen(*args, **kw))
    assert st == 0, (gen.__name__, args)
    return T, n


def flag_room_cases(oracle):
    """Genuine product-route tableaux with nvars raised up to cols - 1: the -0.0 flag bytes
    (rows_cap of them) fit the old room exactly, overflow it by one, or by far.  Across the set:
    cols + max_depth = 0, 1, 15 (mod 16), rows_cap = 0, 1, 15 (mod 16), cols = 0, 1, 63 (mod 64)
    and nvars > 256 (several blocks in k_bb_gather_info / k_bb_node_info)."""
    spec = [  # generator, (n, mcons, seed), nvars (None: cols - 1), max_depth, tag, min children
        (fractional_program, (8, 120, 1), 126, 7, "flag_exact", 8),
        (fractional_program, (12, 250, 1), 253, 9, "flag_exact", 15),
        (fractional_program, (12, 250, 1), 253, 10, "flag_over_by_1", 15),
        (fractional_program, (8, 250, 1), 254, 6, "flag_over_by_1", 10),
        (fractional_program, (6, 250, 1), 238, 8, "flag_over_by_1", 8),
        (random_binary_program, (40, 300, 1), None, 26, "flag_over", 35),
        (random_binary_program, (3, 120, 1), None, 17, "flag_over", 15),
        (random_binary_program, (3, 121, 1), None, 15, "flag_over", 15),
        (random_binary_program, (3, 122, 1), None, 14, "flag_over", 14),
    ]
    out = []
    for gen, args, nvars, md, tag, kids in spec:
        T, _ = _product_root(oracle, gen, *args)
        nv = T.shape[1] - 1 if nvars is None else nvars
        short = "frac" if gen is fractional_program else "bin"
        out.append(_edge(f"{tag}_{short}{args[0]}x{args[1]}s{args[2]}_nv{nv}_md{md}", T, nv, md,
                         tag, kids))
    return out


def _tall(T, extra, seed):
    """T with `extra` rows appended that leave its unit (basic) columns alone: rows > cols."""
    rng = np.random.RandomState(seed)
    C = T.shape[1]
    basic = [j for j in range(C - 1) if np.sum(T[:, j] == 1.0) == 1 and np.sum(T[:, j] != 0) == 1]
    add = np.round(rng.uniform(0, 3, size=(extra, C)), 2)
    add[:, basic] = 0.0
    add[:, -1] = np.round(rng.uniform(5, 50, size=extra), 3)
    return np.vstack([T, add])


def tall_cases(oracle):
    """Not simplex tableaux, but lpr_bb_create takes any rows x cols: rows > cols with
    nvars = cols - 1, two columns (one variable and the RHS), nvars = 0."""
    out = []
    T, _ = _product_root(oracle, fractional_program, 6, 3, 11)
    t = _tall(T, T.shape[1] - T.shape[0] + 6, 0)
    out.append(_edge("tall_frac6x3_nv_all", t, t.shape[1] - 1, 12, "tall", 12))
    T, _ = _product_root(oracle, random_binary_program, 8, 3, 3)
    t = _tall(T, T.shape[1] - T.shape[0] + 6, 0)
    out.append(_edge("tall_bin8x3_nv_all", t, t.shape[1] - 1, 12, "tall", 10))
    rng = np.random.RandomState(0)
    t = np.zeros((300, 2))
    t[:, 0] = np.round(rng.uniform(-1, 2, size=300), 1)
    t[0, 0] = 0.5
    t[3, 0] = 1.0
    t[:, 1] = np.round(rng.uniform(0, 5, size=300), 3)
    out.append(_edge("tall_two_columns_300_rows", t, 1, 24, "tall_cols2", 30))
    T, n = _product_root(oracle, fractional_program, 4, 2, 10)
    t = _tall(T, T.shape[1] - T.shape[0] + 6, 0)
    out.append(_edge("tall_nvars0", t, 0, 8, "nvars0", 0))
    return out


def widest_lds_case(oracle, max_depth: int = 8, extra_cols: int = 0):
    """A genuine tableau widened with non-basic columns before the RHS (reduced cost > 0, short
    decimal entries: still a final tableau) to align16(cols + max_depth) = 36 864 columns, the
    widest k_bb_eliminate ranks in LDS; extra_cols > 0 goes past it."""
    T, n = _product_root(oracle, fractional_program, 6, 2, 3)
    R, C = T.shape
    add = ELIMINATE_LDS_COLS - max_depth - C + extra_cols
    rng = np.random.RandomState(36864)
    W = np.round(rng.uniform(-2, 3, size=(R, add)), 2)
    W[0] = np.round(rng.uniform(0.5, 4, size=add), 2)
    wide = np.hstack([T[:, :-1], W, T[:, -1:]])
    return _edge("widest_lds", wide, n, max_depth, "widest_lds", 6)


BIG_M = (1e12, 3.7e13, 2.5e15, 4e16)


def big_value_cases(oracle):
    """A big-M row (M x0 + x1 <= 0.6 M + 0.37): parents that hold entries >= 1e11 (slot.big, the
    separate rounding and scoring kernels); M >= 1e16 hits Math.Round's identity branch."""
    out = []
    for M in BIG_M:
        T, n = _product_root(oracle, fractional_program, 8, 3, 5, big_m=M)
        out.append(_edge(f"big_m_{M:.1e}", T, n, 24, "big", 12, cap=40))
    return out


def edge_cases(oracle, widest=True):
    out = flag_room_cases(oracle) + tall_cases(oracle) + big_value_cases(oracle)
    if widest:
        out.append(widest_lds_case(oracle))
    return out


_EDGE_CACHE = {}


def edge_case(oracle, name):
    """One edge instance by name (built once per process)."""
    if not _EDGE_CACHE:
        for c in edge_cases(oracle):
            _EDGE_CACHE[c["name"]] = c
    return _EDGE_CACHE[name]


EDGE_CASE_NAMES = [
    "flag_exact_frac8x120s1_nv126_md7", "flag_exact_frac12x250s1_nv253_md9",
    "flag_over_by_1_frac12x250s1_nv253_md10", "flag_over_by_1_frac8x250s1_nv254_md6",
    "flag_over_by_1_frac6x250s1_nv238_md8", "flag_over_bin40x300s1_nv380_md26",
    "flag_over_bin3x120s1_nv126_md17", "flag_over_bin3x121s1_nv127_md15",
    "flag_over_bin3x122s1_nv128_md14",
    "tall_frac6x3_nv_all", "tall_bin8x3_nv_all", "tall_two_columns_300_rows", "tall_nvars0",
    "big_m_1.0e+12", "big_m_3.7e+13", "big_m_2.5e+15", "big_m_4.0e+16",
    "widest_lds",
]
