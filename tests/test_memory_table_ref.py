"""The memory table on the CPU: tests/memory_table_ref.py (the reference's trace generator and constraints restated from the Rust)
against a hand-worked example and against its own constraints; tests/memory_table_model.py (the device's one-sort construction
restated) against that literal model; plonky2_gpu_amd/memory_table.py (the constraints as a register program, the columns, the CTL
columns) and the native emitter gl_memory_table_program against the restatement. Everything is exact; nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import lookup_ref  # noqa: E402
import memory_table_instances as mi  # noqa: E402
import memory_table_model as mm  # noqa: E402
import memory_table_ref as mr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = mr.P
_cache = {}


def _program():
    from plonky2_gpu_amd import memory_table as mt

    if "program" not in _cache:
        _cache["program"] = mt.program()
    return _cache["program"]


def _provable(seed=0, extra=0, degree_bits=None):
    key = ("provable", seed, extra, degree_bits)
    if key not in _cache:
        _cache[key] = mr.trace_of_words(mi.provable(seed, extra), degree_bits)[0]
    return _cache[key]


# ---------------------------------------------------------------- the trace
def test_the_doc_comment_s_example_with_the_code_s_numbers():
    """memory_stark.rs:159-161: "say there are 32 memory operations, and a particular address is accessed at timestamps 20 and 100.
    80 would fail the range check, so this method would add two dummy reads to the same address, say at timestamps 50 and 80."
    The code: max_rc = 32.next_power_of_two() - 1 = 31; 100 - 20 = 80 > 31 pushes a dummy at 20 + 31 = 51; 100 - 51 = 49 > 31
    pushes one at 51 + 31 = 82; 100 - 82 = 18 ends the loop. 51 and 82, not 50 and 80.
    The other 30 operations are at addresses 1 .. 30 of the same segment (no gap), so the vector after fill_gaps has 34 elements, its
    last is the dummy at 82, and pad_memory_ops repeats THAT 30 times: the padding stands in the middle of the 64-row trace, rows
    3 .. 32, between the dummy at 82 (row 2) and the access at 100 (row 33)."""
    ops = [mr.MemoryOp(True, 20, False, 0, 0, 0, [9] * 8), mr.MemoryOp(True, 100, False, 0, 0, 0, [7] * 8)]
    ops += [mr.MemoryOp(True, 200 + a, False, 0, 0, a, [a] * 8) for a in range(1, 31)]
    assert len(ops) == 32
    cols, rows = mr.generate_trace(ops)
    assert rows == 34 and len(cols) == 26 and len(cols[0]) == 64
    ts, virt, flt, rd = cols[mr.TIMESTAMP], cols[mr.ADDR_VIRTUAL], cols[mr.FILTER], cols[mr.IS_READ]
    assert ts[:3] == [20, 51, 82] and ts[3:33] == [82] * 30 and ts[33] == 100
    assert virt[:34] == [0] * 34 and virt[34:] == list(range(1, 31))
    assert flt[:34] == [1] + [0] * 32 + [1] and rd[:34] == [0] + [1] * 32 + [0]
    assert [cols[mr.value_limb(0)][r] for r in (0, 1, 2, 3, 32, 33, 34)] == [9, 0, 0, 0, 0, 7, 1]
    assert cols[mr.RANGE_CHECK][:35] == [31, 31] + [0] * 30 + [18, 0, 0]  # 51 - 20, 82 - 51, the padding, 100 - 82, address 0 -> 1 -> 2
    assert cols[mr.VIRTUAL_FIRST_CHANGE][:35] == [0] * 33 + [1, 1] and cols[mr.VIRTUAL_FIRST_CHANGE][63] == 0
    assert cols[mr.COUNTER] == list(range(64))
    for c in range(mr.VIRTUAL_FIRST_CHANGE + 1, mr.RANGE_CHECK):
        assert cols[c] == [0] * 64
    assert [cols[c][63] for c in (mr.CONTEXT_FIRST_CHANGE, mr.SEGMENT_FIRST_CHANGE, mr.VIRTUAL_FIRST_CHANGE, mr.RANGE_CHECK)] == [0] * 4
    lookup_ref.check_lookup_argument(cols[mr.RANGE_CHECK], cols[mr.COUNTER], cols[mr.RANGE_CHECK_PERMUTED], cols[mr.COUNTER_PERMUTED])


def test_virtual_address_dummies_and_equal_keys_in_list_order():
    """4 operations (max_rc 3): addresses 0 and 9 ask for dummies at 4 and 8 with timestamp 0; the two operations with the same key
    keep their list order; without a dummy the padding repeats the largest operation, at the end"""
    w = mi.words([1, 1, 1, 1], [5, 5, 1, 1], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [9, 9, 0, 0], [[1] * 8, [2] * 8, [3] * 8, [4] * 8])
    cols, rows = mr.trace_of_words(w)
    assert rows == 6 and cols.shape == (26, 8)
    assert cols[mr.ADDR_VIRTUAL].tolist() == [0, 0, 4, 8, 8, 8, 9, 9] and cols[mr.TIMESTAMP].tolist() == [1, 1, 0, 0, 0, 0, 5, 5]
    assert cols[mr.value_limb(3)].tolist() == [3, 4, 0, 0, 0, 0, 1, 2] and cols[mr.FILTER].tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
    cols, rows = mr.trace_of_words(w[:3])  # 9, 9, 0 under max_rc 3 as well: the same dummies
    assert rows == 5 and cols[mr.ADDR_VIRTUAL].tolist() == [0, 4, 8, 8, 8, 8, 9, 9] and cols[mr.FILTER].tolist() == [1, 0, 0, 0, 0, 0, 1, 1]
    cols, rows = mr.trace_of_words(mi.no_gap(5))
    assert rows == 5 and cols[mr.FILTER].tolist()[5:] == [0, 0, 0] and cols[mr.IS_READ].tolist()[5:] == [1, 1, 1]
    assert (cols[: mr.OP_WORDS, 5:] == cols[: mr.OP_WORDS, 4:5]).sum() >= 3 * 12  # all but filter and kind


def test_the_reference_s_assert_on_context_gaps():
    w = mi.words([1, 1], [1, 2], [0, 0], [0, 6], [0, 0], [0, 0], np.zeros((2, 8)))
    with pytest.raises(AssertionError, match="Range check of 5 is too large"):
        mr.trace_of_words(w)
    assert mr.trace_of_words(w, degree_bits=3)[0][mr.RANGE_CHECK, 0] == 5


FAMILIES = [("small_keys", 2), ("small_keys", 3), ("small_keys", 65), ("small_keys", 257), ("mixed", 5), ("mixed", 64), ("mixed", 300),
            ("in_order", 65), ("reversed", 65), ("one_address", 40), ("at_the_top", 33), ("one_long_gap", 4), ("no_gap", 64), ("wide", 2500)]


def _family(name, num_ops):
    if name == "one_long_gap":
        return mi.one_long_gap()
    if name in ("in_order", "reversed"):
        return mi.in_order(num_ops, reverse=name == "reversed")
    return getattr(mi, name)(num_ops)


@pytest.mark.parametrize("name,num_ops", FAMILIES)
def test_the_one_sort_construction_gives_the_reference_s_rows(name, num_ops):
    """tests/memory_table_model.py — the device's decomposition — against the literal two-sort model, on every family the GPU test
    uses, at the smallest height and at one two bits above it"""
    w = _family(name, num_ops)
    if name == "wide":  # few operations per group: close the context and segment gaps the draw left open
        for c in (mr.ADDR_CONTEXT, mr.ADDR_SEGMENT):
            w[:, c] = np.searchsorted(np.unique(w[:, c]), w[:, c]) * 1000
    exp, rows = mr.trace_of_words(w)
    assert mm.rows_needed(w) == rows == mr.rows_needed(w)
    bits = exp.shape[1].bit_length() - 1
    for degree_bits in (bits, bits + 2):
        if degree_bits != bits:
            exp = mr.trace_of_words(w, degree_bits)[0]
        got = mm.trace_rows(w, degree_bits)
        bad = np.argwhere(got[: mr.COUNTER + 1] != exp[: mr.COUNTER + 1])
        assert bad.size == 0, ("first (column, row) that differs", bad[0].tolist(), len(bad))


# ---------------------------------------------------------------- the constraints on the trace
@pytest.mark.parametrize("seed,extra,degree_bits", [(0, 0, None), (1, 3, None), (2, 6, 6)])
def test_every_constraint_holds_on_every_row(seed, extra, degree_bits):
    """dummies of both kinds, padding rows in the middle, the wrap-around row included"""
    cols = _provable(seed, extra, degree_bits)
    n = cols.shape[1]
    assert n == (64 if degree_bits else 32)
    flt = cols[mr.FILTER].tolist()
    first_padding = 3 + 6 + 1 + 2  # behind the three accesses of address 0, six dummies, the read at 3 and two dummies
    assert flt[first_padding : first_padding + n - 18 - extra] == [0] * (n - 18 - extra) and flt[first_padding + n - 18 - extra] == 1
    assert cols[mr.TIMESTAMP, first_padding - 1] == 33 and cols[mr.ADDR_VIRTUAL, 3:9].tolist() == [16, 32, 48, 64, 80, 96]
    assert mr.violations(cols) == []
    assert mr.satisfies_its_constraints(cols)


def test_an_instance_the_reference_s_own_constraints_reject():
    """a timestamp-gap dummy reads 0 where the address holds something else: the value constraint of the row before it fails. The
    reference's trace generator and its constraints disagree there; the model keeps both as they are."""
    w = mi.words([1, 1], [1, 9], [0, 1], [0, 0], [0, 0], [0, 0], [[5] * 8, [5] * 8])
    cols = mr.trace_of_words(w)[0]  # max_rc 1: dummies at 2 .. 8
    assert cols.shape == (26, 16) and cols[mr.FILTER].tolist()[:9] == [1] + [0] * 8
    bad = mr.violations(cols)
    assert {(r, g) for r, g, _ in bad} == {(0, "values"), (14, "values")} and len(bad) == 16


TAMPER = {
    # (column, row, new value) -> [(row, group, index)]
    "the filter of a padding row": ((mr.FILTER, 13, 2), [(13, "filter_boolean", 0)]),  # it is a read: (1 - filter) * 0 stays 0
    "the filter of a write": ((mr.FILTER, 27, 0), [(27, "dummy_is_read", 0)]),
    "a dummy turned into a write": ((mr.IS_READ, 5, 0), [(5, "dummy_is_read", 0)]),
    # row 0 and row 1 share their address: with the flag set address_unchanged becomes 0, still boolean, and every product with the
    # (zero) address differences stays 0 — only the range check sees it: 1 (0 - 0 - 1) against the timestamp difference 1
    "a first-change flag": ((mr.VIRTUAL_FIRST_CHANGE, 0, 1), [(0, "range_check", 0)]),
    # row 27, the write at 50, stands before segment 1 (address 5, timestamp 6): address_unchanged becomes -1 and meets the segment,
    # address and timestamp differences; the context does not change
    "a first-change flag of 2": ((mr.SEGMENT_FIRST_CHANGE, 27, 2), [(27, "flags_boolean", 1), (27, "flags_boolean", 3), (27, "no_change_before", 4),
                                                                   (27, "no_change_before", 5), (27, "range_check", 0)]),
    "a range check": ((mr.RANGE_CHECK, 9, 3), [(9, "range_check", 0)]),
    "a value limb of a read": ((mr.value_limb(2), 1, 77), [(0, "values", 2), (1, "values", 2)]),
    "a timestamp": ((mr.TIMESTAMP, 10, 19), [(9, "range_check", 0), (10, "range_check", 0)]),
    # row 0 is the NEXT row of the last one: there the permuted input falls from the largest range check to 0, so the product
    # needs the table value beside it, and the last-row constraint asks for it outright
    "a permuted table value": ((mr.COUNTER_PERMUTED, 0, 5), [(31, "lookup", 0), (31, "lookup", 1)]),
}


@pytest.mark.parametrize("what", sorted(TAMPER))
def test_one_changed_cell_breaks_exactly_the_constraints_it_should(what):
    """the trace of provable(0): rows 0 .. 2 address 0 (write, read, read), 3 .. 8 the dummies to address 100, 9 the read at 3,
    10 .. 11 the dummies at 18 and 33, 12 .. 25 the padding, 26 the read at 43"""
    (column, row, value), expected = TAMPER[what]
    cols = _provable().copy()
    assert cols[mr.IS_READ, 5] == 1 and cols[mr.FILTER, 13] == 0 and cols[mr.TIMESTAMP, 10] == 18 and cols[mr.COUNTER_PERMUTED, 0] == 0
    cols[column, row] = value
    assert mr.violations(cols) == expected


# ---------------------------------------------------------------- the program
def test_program_and_closures_agree_on_random_rows():
    instrs, immediates = _program()
    rng = np.random.default_rng(26)
    for _ in range(16):
        local, nxt = ([int(v) % P for v in rng.integers(0, 1 << 64, size=mr.NUM_COLUMNS, dtype=np.uint64)] for _ in range(2))
        z_last, l_first, l_last = (int(v) % P for v in rng.integers(0, 1 << 64, size=3, dtype=np.uint64))
        consumer = sr.Consumer(sr.Base, [3], z_last, l_first, l_last)
        sr.run_program(sr.Base, instrs, immediates, local, nxt, [], consumer)
        factor = {mr.ALL: 1, mr.TRANSITION: z_last, mr.LAST_ROW: l_last}
        exp = [v * factor[kind] % P for kind, v in mr.eval_constraints(local, nxt)]
        assert len(consumer.emitted) == len(exp) == 23 and all(exp)
        assert consumer.emitted == exp


def test_program_validates_and_the_native_emitter_gives_the_same_words():
    from plonky2_gpu_amd import memory_table as mt

    instrs, immediates = _program()
    sr.validate_program(instrs, immediates, mt.NUM_COLUMNS, 0)
    assert instrs.dtype == np.uint16 and immediates == [1]
    n_instrs, n_immediates, num_constraints = mt.native_program()
    assert n_instrs.shape == instrs.shape and (n_instrs == instrs).all()
    assert n_immediates == list(immediates)
    assert num_constraints == 23 == mt.NUM_CONSTRAINTS == sum(int(op) in (sr.EMIT, sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW) for op in instrs[:, 0])
    kinds = [int(op) for op in instrs[:, 0] if int(op) in (sr.EMIT, sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW)]
    assert kinds == [sr.EMIT] * 6 + [sr.EMIT_TRANSITION] * 7 + [sr.EMIT] * 9 + [sr.EMIT_LAST_ROW]
    desc = mt.stark_desc(5, 2, si.fri_params(rate_bits=1))
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.quotient_degree_factor) == (26, 0, 3, 2)
    assert desc.pairs == mr.MemoryTableStark.pairs == [[(22, 24)], [(23, 25)]] and desc.num_zs == 2


def test_columns_are_the_reference_s():
    from plonky2_gpu_amd import memory_table as mt

    names = ("NUM_CHANNELS VALUE_LIMBS FILTER TIMESTAMP IS_READ ADDR_CONTEXT ADDR_SEGMENT ADDR_VIRTUAL VALUE_START CONTEXT_FIRST_CHANGE "
             "SEGMENT_FIRST_CHANGE VIRTUAL_FIRST_CHANGE RANGE_CHECK COUNTER RANGE_CHECK_PERMUTED COUNTER_PERMUTED NUM_COLUMNS OP_WORDS").split()
    for name in names:
        assert getattr(mt, name) == getattr(mr, name), name
    assert [mt.value_limb(i) for i in range(8)] == [mr.value_limb(i) for i in range(8)] == list(range(6, 14))
    assert (mt.FILTER, mt.TIMESTAMP, mt.IS_READ, mt.RANGE_CHECK, mt.COUNTER_PERMUTED, mt.NUM_COLUMNS) == (0, 1, 2, 22, 25, 26)


def test_ctl_columns_are_the_operation_and_the_filter():
    from plonky2_gpu_amd import memory_table as mt

    data, flt = mt.ctl_data(), mt.ctl_filter()
    assert len(data) == 13 and all(len(c.terms) == 1 and c.terms[0][1] == 1 and c.constant == 0 for c in data + [flt])
    assert [c.terms[0][0] for c in data] == [mr.IS_READ, mr.ADDR_CONTEXT, mr.ADDR_SEGMENT, mr.ADDR_VIRTUAL] + [mr.value_limb(i) for i in range(8)] + [mr.TIMESTAMP]
    w = mi.provable()
    cols = _provable()
    looked = sorted(tuple(ctl_ref.eval_column(sr.Base, c, [int(v) for v in cols[:, r]]) for c in data)
                    for r in range(32) if ctl_ref.eval_column(sr.Base, flt, [int(v) for v in cols[:, r]]))
    order = [mr.IS_READ, mr.ADDR_CONTEXT, mr.ADDR_SEGMENT, mr.ADDR_VIRTUAL] + list(range(6, 14)) + [mr.TIMESTAMP]
    assert looked == sorted(tuple(int(row[c]) for c in order) for row in w)  # the rows with filter 1 are the operations, all of them


def test_ops_to_words():
    from plonky2_gpu_amd import memory_table as mt

    value = sum((k + 1) << (32 * k) for k in range(8))
    w = mt.ops_to_words([(1, 7, 0, 2, 3, 4, value), (0, 8, 1, 5, 6, 9, [9, 8, 7, 6, 5, 4, 3, 2])])
    assert w.dtype == np.uint64 and w.tolist() == [[1, 7, 0, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8], [0, 8, 1, 5, 6, 9, 9, 8, 7, 6, 5, 4, 3, 2]]
    ops = mr.ops_from_words(w)
    assert ops[0].into_row()[:14] == w[0].tolist() and ops[1].sorting_key() == (5, 6, 9, 8)
    with pytest.raises(ValueError):
        mt.ops_to_words([(1, 7, 0, 2, 3, 4, 1 << 256)])


# ---------------------------------------------------------------- one whole proof
def test_the_reference_prover_proves_the_table_and_its_verifier_accepts():
    """32 rows, rate 2, 2 challenges: stark_ref proves the program (two permutation Zs) and verifies with the program and with the
    closures"""
    from oracle import accel

    instrs, immediates = _program()
    stark = mr.MemoryTableStark(instrs, immediates)
    fp = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))
    cols = _provable()
    assert mr.satisfies_its_constraints(cols)
    trace = [[int(v) for v in col] for col in cols]
    hasher = gr.PoseidonHasher()
    with accel.c_backend():
        proof = sr.prove(hasher, stark, 2, fp, trace, [])
        assert sr.verify(hasher, stark, 2, fp, proof)
        assert sr.verify(hasher, stark, 2, fp, proof, evaluator="closure")
    assert len(proof["openings"]["local_values"]) == 26 and len(proof["openings"]["quotient_polys"]) == 4 and len(proof["openings"]["permutation_zs"]) == 2
