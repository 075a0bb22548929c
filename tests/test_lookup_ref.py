"""CPU tests of the lookup argument's host side: tests/lookup_ref.py (the serial restatement of permuted_cols and the checker of the
argument) on cases worked by hand from evm/src/lookup.rs:67-131, the STARK "L" of tests/lookup_instances.py through
tests/stark_ref.py, and StarkAsm.eval_lookups."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generic_prove_ref as gr  # noqa: E402
import lookup_instances as li  # noqa: E402
import lookup_model  # noqa: E402
import lookup_ref as lr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = lr.P
HASHERS = {"poseidon": gr.PoseidonHasher(), "keccak": gr.KeccakHasher()}

# (inputs, table, permuted_table), each worked through the loop of lookup.rs:95-128. i walks the sorted inputs S, j the sorted
# table T; "stack" is unused_table_vals, "inds" is unused_table_inds.
HAND_WORKED = [
    # S = [5, 5], T = [5, 7]. (i 0, j 0): 5 == 5, permuted_table[0] = 5, i 1, j 1. (1, 1): 5 < 7 and the stack is empty: inds = [1],
    # i 2: the loop ends. T[1] = 7 goes onto the stack: stack = [7]. zip: permuted_table[1] = 7.
    ([5, 5], [5, 7], [5, 7]),
    # S = [1, 1, 9], T = [0, 3, 9]. (0, 0): 1 > 0, push 0, j 1. (0, 1): 1 < 3, pop 0: permuted_table[0] = 0, i 1. (1, 1): 1 < 3 and the
    # stack is empty: inds = [1], i 2. (2, 1): 9 > 3, push 3, j 2. (2, 2): 9 == 9, permuted_table[2] = 9; the loop ends with
    # stack = [3], inds = [1]: permuted_table[1] = 3. The second 1 comes too early for 3 (3 is pushed only when 9 arrives): it waits
    # in inds and gets 3 from the zip.
    ([1, 1, 9], [0, 3, 9], [0, 3, 9]),
    # LIFO: S = [4, 4, 9], T = [0, 3, 9]. (0, 0): 4 > 0, push 0. (0, 1): 4 > 3, push 3: stack = [0, 3], j 2. (0, 2): 4 < 9, pop 3:
    # permuted_table[0] = 3. (1, 2): 4 < 9, pop 0: permuted_table[1] = 0. (2, 2): 9 == 9. The value pushed last is taken first.
    ([4, 4, 9], [0, 3, 9], [3, 0, 9]),
    # every input below every table value: S = [1, 2], T = [5, 6]. (0, 0): 1 < 5, empty stack, inds = [0]. (1, 0): 2 < 5, inds =
    # [0, 1]; i = 2 ends the loop with j = 0: both table values go onto the stack in order, stack = [5, 6]; zip: [5, 6].
    ([1, 2], [5, 6], [5, 6]),
    # every input above every table value: S = [8, 9], T = [1, 2]. (0, 0): 8 > 1, push 1. (0, 1): 8 > 2, push 2; j = 2 ends the loop
    # with i = 0 and stack = [1, 2]. Both inputs are post-loop: inds = [0, 1], and the zip hands the stack out from the BOTTOM:
    # permuted_table = [1, 2] — a pop would have given 8 the 2.
    ([8, 9], [1, 2], [1, 2]),
    # a deferred input and a post-loop input together: S = [1, 6, 7], T = [2, 3, 5]. (0, 0): 1 < 2, empty: inds = [0]. (1, 0), (1, 1),
    # (1, 2): 6 > 2, 3, 5: stack = [2, 3, 5], j 3 ends the loop with i = 1. inds = [0, 1, 2]: permuted_table = [2, 3, 5].
    ([1, 6, 7], [2, 3, 5], [2, 3, 5]),
]


@pytest.mark.parametrize("inputs,table,expected", HAND_WORKED)
def test_hand_worked_cases(inputs, table, expected):
    pi, pt = lr.permuted_cols(inputs, table)
    assert pi == sorted(inputs) and pt == expected
    if set(inputs) <= set(table):
        lr.check_lookup_argument(inputs, table, pi, pt)


def test_any_representative_is_canonicalised():
    """p is 0, p + 1 is 1, 2^64 - 1 is 2^32 - 2 (lookup.rs:79-88 canonicalises before it sorts)"""
    pi, pt = lr.permuted_cols([P, (1 << 64) - 1, P + 1], [1, 0, (1 << 32) - 2])
    assert pi == [0, 1, (1 << 32) - 2] and pt == pi


def _random_case(rng, n):
    kind = rng.integers(0, 4)
    if kind == 0:  # a range check against a counter
        return [int(x) for x in rng.integers(0, n, size=n)], list(range(n))
    if kind == 1:  # heavy duplicates on both sides, every input in the table
        table = [int(x) for x in rng.integers(0, max(1, n // 3), size=n)]
        return [table[int(k)] for k in rng.integers(0, n, size=n)], table
    if kind == 2:  # full-width words in any representation
        table = [int(x) for x in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)]
        return [table[int(k)] for k in rng.integers(0, n, size=n)], table
    return [int(x) for x in rng.permutation(n)], list(range(n))


def test_the_checker_accepts_the_restatement_on_random_cases():
    rng = np.random.default_rng(5)
    for _ in range(300):
        inputs, table = _random_case(rng, int(rng.integers(1, 40)))
        lr.check_lookup_argument(inputs, table, *lr.permuted_cols(inputs, table))


def test_the_decomposition_of_the_kernels_equals_the_serial_loop():
    """tests/lookup_model.py (events, the (sum, min) scan, levels, the sort by level) against the restatement: the hand-worked cases,
    3000 random small cases of every kind with heavy duplicates, and two lengths with full-width words and with a range check"""
    rng = np.random.default_rng(11)
    cases = [(i, t) for i, t, _ in HAND_WORKED] + [([1], [1]), ([1], [2]), ([2], [1])]
    for _ in range(3000):
        n = int(rng.integers(1, 13))
        r = int(rng.choice([2, 4, 8, 20]))
        cases.append(([int(x) for x in rng.integers(0, r, size=n)], [int(x) for x in rng.integers(0, r, size=n)]))
        cases.append(_random_case(rng, n))
    for n in (1000, 4097):
        cases.append(([int(x) for x in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)], [int(x) for x in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)]))
        cases.append(([int(x) for x in rng.integers(0, n, size=n)], list(range(n))))
        cases.append(([int(x) for x in rng.integers(0, n // 3, size=n)], [int(x) for x in rng.integers(0, n // 2, size=n)]))
    for inputs, table in cases:
        assert lookup_model.permuted_cols_by_events(inputs, table) == lr.permuted_cols(inputs, table), (inputs, table)


def test_the_checker_rejects_what_the_constraints_reject():
    inputs, table = [2, 0, 2, 1], [0, 1, 2, 3]
    pi, pt = lr.permuted_cols(inputs, table)
    assert (pi, pt) == ([0, 1, 2, 2], [0, 1, 2, 3])
    for bad_pi, bad_pt in (([0, 1, 2, 3], pt), (pi, [0, 1, 3, 2]), (pi, [0, 1, 2, 2]), ([2, 0, 1, 2], [2, 0, 1, 3])):
        with pytest.raises(AssertionError):
            lr.check_lookup_argument(inputs, table, bad_pi, bad_pt)
    with pytest.raises(AssertionError):  # an input outside the table: no permuted table can satisfy the rows
        lr.check_lookup_argument([9, 0, 1, 2], table, *lr.permuted_cols([9, 0, 1, 2], table))


def test_the_trace_of_l_satisfies_the_argument():
    for degree_bits in (1, 4, 6):
        trace, pis = li.L.make_trace(degree_bits, seed=degree_bits)
        n = 1 << degree_bits
        assert pis == [] and len(trace) == 6 and all(0 <= x < n for x in trace[li.V])
        lr.check_lookup_argument(trace[li.V], trace[li.C0], trace[li.PV], trace[li.PT])
        if degree_bits > 3:
            counts = np.bincount(trace[li.V], minlength=n)
            assert (counts == 0).sum() >= n // 4 and counts.max() >= 3  # unused counter values, values hit many times
    assert li.L.pairs == [[(li.V, li.PV)], [(li.C0, li.PT)]]


# no arity 1: its leaves are 4 elements, which KeccakHash<25> cannot hash
_FRI = {4: dict(rate_bits=1, cap_height=1, arity_bits=(2,)), 6: dict(rate_bits=2, cap_height=2, arity_bits=(3,))}


@pytest.mark.parametrize("degree_bits,hasher", [(4, "poseidon"), (6, "poseidon"), (4, "keccak"), (6, "keccak")])
def test_l_proves_and_verifies_with_both_evaluators(degree_bits, hasher):
    fp = si.fri_params(**_FRI[degree_bits])
    trace, pis = li.L.make_trace(degree_bits, seed=degree_bits)
    h = HASHERS[hasher]
    nch = li.NUM_CHALLENGES[hasher]
    by_program = sr.prove(h, li.L, nch, fp, trace, pis)
    by_closure = sr.prove(h, li.L, nch, fp, trace, pis, evaluator="closure")
    assert sr.proof_bytes(h, by_program) == sr.proof_bytes(h, by_closure)
    assert sr.verify(h, li.L, nch, fp, by_program)
    assert sr.verify(h, li.L, nch, fp, by_program, evaluator="closure")


def test_a_value_outside_the_range_is_rejected():
    """One v = n + 5: permuted_cols still fills its columns, but the largest permuted input is neither a repeat of the row above nor
    the table value beside it. L's quotient_degree_factor is a power of two, so the prover has no tail of the quotient to check
    ("Quotient has failed"): it returns a proof, and the verifier rejects it."""
    degree_bits, fp, h = 4, si.fri_params(**_FRI[4]), HASHERS["poseidon"]
    n = 1 << degree_bits
    v = li.l_values(degree_bits, seed=9)
    v[5] = n + 5
    trace = li.l_trace_from_values(v)
    with pytest.raises(AssertionError):
        lr.check_lookup_argument(trace[li.V], trace[li.C0], trace[li.PV], trace[li.PT])
    proof = sr.prove(h, li.L, 2, fp, trace, [])
    with pytest.raises(AssertionError, match="Mismatch between evaluation and opening of quotient polynomial"):
        sr.verify(h, li.L, 2, fp, proof)
    good = sr.prove(h, li.L, 2, fp, li.L.make_trace(degree_bits, seed=9)[0], [])
    assert sr.verify(h, li.L, 2, fp, good)


def test_eval_lookups_emits_lookup_rs_19_to_33():
    from plonky2_gpu_amd import stark as ps

    a = ps.StarkAsm()
    a.eval_lookups(7, 9)
    instrs, imms = a.program()
    assert imms == []
    r = [int(x) for x in instrs[:, 1]]
    local_in, next_table, next_in, diff_prev, diff_table, product = r[:6]
    assert len({local_in, next_table, next_in, diff_prev, diff_table, product}) == 6
    assert [tuple(int(x) for x in row) for row in instrs] == [
        (ps.LOAD_WIRE, local_in, 7, 0),  # local_perm_input
        (ps.LOAD_NEXT, next_table, 9, 0),  # next_perm_table
        (ps.LOAD_NEXT, next_in, 7, 0),  # next_perm_input
        (ps.SUB, diff_prev, next_in, local_in),  # diff_input_prev
        (ps.SUB, diff_table, next_in, next_table),  # diff_input_table
        (ps.MUL, product, diff_prev, diff_table),
        (ps.EMIT, 0, product, 0),  # yield_constr.constraint(diff_input_prev * diff_input_table)
        (ps.EMIT_LAST_ROW, 0, diff_table, 0),  # yield_constr.constraint_last_row(diff_input_table)
    ]
    sr.validate_program(instrs, imms, 10, 0)


def test_lookup_pairs_are_the_singletons_of_memory_stark():
    from plonky2_gpu_amd.lookup import lookup_pairs

    assert lookup_pairs([(1, 0, 2, 3), (8, 0, 6, 5)]) == [[(1, 2)], [(0, 3)], [(8, 6)], [(0, 5)]]
    assert lookup_pairs([]) == []
