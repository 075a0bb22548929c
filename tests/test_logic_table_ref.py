"""The logic table on the CPU: tests/logic_table_ref.py (the reference's rows and constraints restated from the Rust) against direct
big-integer arithmetic and against its own constraints; plonky2_gpu_amd/logic_table.py (the constraints as a register program, the
columns, the CTL columns) and the native emitter gl_logic_table_program against the restatement. Everything is exact; nothing
here needs a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import logic_table_instances as li  # noqa: E402
import logic_table_ref as lr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = lr.P
EMITS = (sr.EMIT, sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW)
_cache = {}


def _program():
    from plonky2_gpu_amd import logic_table as lt

    if "program" not in _cache:
        _cache["program"] = lt.program()
    return _cache["program"]


def _trace(family="mixed", num_ops=13, degree_bits=None):
    key = (family, num_ops, degree_bits)
    if key not in _cache:
        _cache[key] = lr.trace_of_words(li.FAMILIES[family](num_ops), degree_bits)
    return _cache[key]


def _int(limbs):
    return sum(int(x) << (32 * j) for j, x in enumerate(limbs))


# ---------------------------------------------------------------- the trace
@pytest.mark.parametrize("family", sorted(li.FAMILIES))
def test_rows_against_big_integer_arithmetic(family):
    """every column of every row from Python's own &, | and ^ on 256-bit integers; the rows behind the operations are zero"""
    w = li.FAMILIES[family](21)
    cols = lr.trace_of_words(w)
    assert cols.shape == (523, 32) and not cols[:, 21:].any()
    seen = set()
    for r, rec in enumerate(w):
        op, a, b = int(rec[0]), _int(rec[1:9]), _int(rec[9:17])
        seen.add(op)
        assert [int(cols[f, r]) for f in (lr.IS_AND, lr.IS_OR, lr.IS_XOR)] == [int(op == f) for f in range(3)]
        assert sum(int(cols[3 + i, r]) << i for i in range(256)) == a and sum(int(cols[259 + i, r]) << i for i in range(256)) == b
        assert set(cols[3:515, r].tolist()) <= {0, 1}
        assert sum(int(cols[515 + i, r]) << (32 * i) for i in range(8)) == (a & b, a | b, a ^ b)[op]
        assert all(int(cols[515 + i, r]) < 1 << 32 for i in range(8))
    assert seen == ({"and_only": {0}, "or_only": {1}, "xor_only": {2}}.get(family, {0, 1, 2}))


def test_the_families_are_what_they_say():
    w = li.edge_limbs(64)
    assert set(w[:, 1:].reshape(-1).tolist()) == {0, (1 << 32) - 1, 1 << 31}
    w = li.equal_inputs(64)
    assert (w[:, 1:9] == w[:, 9:17]).all()
    cols = lr.trace_of_words(w)
    for r in range(64):
        assert (cols[515:523, r] == (0 if w[r, 0] == 2 else w[r, 1:9])).all()


def test_padding_follows_min_rows():
    """generate_trace_rows pads to max(len, min_rows).next_power_of_two(); a STARK of this package has at least two rows"""
    assert lr.trace_of_words(li.random_ops(0)).shape == (523, 2) and not lr.trace_of_words(li.random_ops(0)).any()
    assert lr.trace_of_words(li.random_ops(1)).shape == (523, 2)
    assert lr.trace_of_words(li.random_ops(2)).shape == (523, 2)
    assert lr.trace_of_words(li.random_ops(3)).shape == (523, 4)
    assert lr.trace_of_words(li.random_ops(33)).shape == (523, 64)
    wide = lr.trace_of_words(li.random_ops(3), 4)
    assert wide.shape == (523, 16) and (wide[:, :4] == lr.trace_of_words(li.random_ops(3))).all() and not wide[:, 4:].any()
    assert len(lr.generate_trace_rows([], 0)) == 1 and len(lr.generate_trace_rows(lr.ops_from_words(li.random_ops(5)), 9)) == 16


# ---------------------------------------------------------------- the constraints on the trace
@pytest.mark.parametrize("family,num_ops,degree_bits", [("mixed", 13, None), ("edge_limbs", 8, None), ("equal_inputs", 5, 4), ("random", 0, 1)])
def test_every_constraint_holds_on_every_row(family, num_ops, degree_bits):
    """all 520, through the program's interpreter and through the closures, padding rows included"""
    cols = _trace(family, num_ops, degree_bits)
    instrs, immediates = _program()
    assert lr.violations(cols) == []
    for r in range(cols.shape[1]):
        local = [int(v) for v in cols[:, r]]
        consumer = sr.Consumer(sr.Base, [3], 1, 1, 1)
        sr.run_program(sr.Base, instrs, immediates, local, local, [], consumer)
        assert consumer.emitted == [0] * 520 == lr.eval_constraints(local)


TAMPER = {
    # (column, row, change) -> [(row, group, index)]; row 2 of mixed(13) is of the equal-inputs family, rows 5 and 11 are XORs: a
    # flipped bit changes x + y - 2 x_land_y by 2^j (1 - 2 other bit), never by zero (under AND and OR the other bit can hide it)
    "a flipped bit of input0": ((3 + 32 * 5 + 7, 5, "flip"), [(5, "result", 5)]),
    "a flipped bit of input1": ((259 + 32 * 2 + 31, 11, "flip"), [(11, "result", 2)]),
    "a flipped bit of input0 in a padding row": ((3 + 200, 14, "flip"), []),  # no flag is set: both coefficients are zero
    "a bit of input1 set to 2 in a padding row": ((259 + 9, 15, 2), [(15, "input1_bit", 9)]),
    "a wrong result limb": ((515 + 3, 2, "flip"), [(2, "result", 3)]),
    "a result limb in a padding row": ((515 + 0, 13, 1), [(13, "result", 0)]),
}


@pytest.mark.parametrize("what", sorted(TAMPER))
def test_one_changed_cell_breaks_exactly_the_constraints_it_should(what):
    """through the closures and through the program: the same constraints, and only they, are non-zero"""
    (column, row, change), expected = TAMPER[what]
    cols = _trace().copy()
    assert cols.shape == (523, 16)
    cols[column, row] = cols[column, row] ^ np.uint64(1) if change == "flip" else change
    assert lr.violations(cols) == expected
    instrs, immediates = _program()
    local = [int(v) for v in cols[:, row]]
    consumer = sr.Consumer(sr.Base, [3], 1, 1, 1)
    sr.run_program(sr.Base, instrs, immediates, local, local, [], consumer)
    assert [lr.group_of(k) for k, v in enumerate(consumer.emitted) if v] == [g[1:] for g in expected]


def test_a_bit_set_to_2_in_an_and_row():
    """row 3 of mixed(13) is an AND: sum_coeff 0, and_coeff 1. Where the other input's bit is 0 the product stays 0 and the bit check
    alone fails; where it is 1 the limb's result constraint fails with it."""
    cols = _trace()
    assert [int(cols[f, 3]) for f in range(3)] == [1, 0, 0]
    y_bits = cols[259 + 224 : 259 + 256, 3].tolist()
    for y_bit, extra in ((0, []), (1, [(3, "result", 7)])):
        j = y_bits.index(y_bit)
        tampered = cols.copy()
        tampered[3 + 224 + j, 3] = 2
        assert lr.violations(tampered) == [(3, "input0_bit", 224 + j)] + extra
        instrs, immediates = _program()
        local = [int(v) for v in tampered[:, 3]]
        consumer = sr.Consumer(sr.Base, [3], 1, 1, 1)
        sr.run_program(sr.Base, instrs, immediates, local, local, [], consumer)
        assert [(3,) + lr.group_of(k) for k, v in enumerate(consumer.emitted) if v] == [(3, "input0_bit", 224 + j)] + extra


# ---------------------------------------------------------------- the program
def test_program_and_closures_agree_on_random_rows():
    instrs, immediates = _program()
    rng = np.random.default_rng(523)
    for _ in range(8):
        local, nxt = ([int(v) % P for v in rng.integers(0, 1 << 64, size=lr.NUM_COLUMNS, dtype=np.uint64)] for _ in range(2))
        consumer = sr.Consumer(sr.Base, [3], 5, 7, 11)
        sr.run_program(sr.Base, instrs, immediates, local, nxt, [], consumer)
        exp = lr.eval_constraints(local)
        assert len(consumer.emitted) == len(exp) == 520 and all(exp)
        assert consumer.emitted == exp


def test_program_validates_and_the_native_emitter_gives_the_same_words():
    from plonky2_gpu_amd import logic_table as lt

    instrs, immediates = _program()
    sr.validate_program(instrs, immediates, lt.NUM_COLUMNS, 0)  # registers below 64, accumulators below 4, the ACC contract
    assert instrs.dtype == np.uint16 and immediates == [1 << k for k in range(16)]
    n_instrs, n_immediates, num_constraints = lt.native_program()
    assert n_instrs.shape == instrs.shape and (n_instrs == instrs).all()
    assert n_immediates == list(immediates)
    assert num_constraints == 520 == lt.NUM_CONSTRAINTS == lr.NUM_CONSTRAINTS == sum(int(op) in EMITS for op in instrs[:, 0])
    assert all(int(op) == sr.EMIT for op in instrs[:, 0] if int(op) in EMITS)
    accs = [int(row[1]) for row in instrs if int(row[0]) == sr.ACC]
    assert accs and max(accs) < 4
    desc = lt.stark_desc(5, 2, si.fri_params(rate_bits=1))
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.quotient_degree_factor) == (523, 0, 3, 2)
    assert desc.pairs == lr.LogicTableStark.pairs == [] and desc.num_zs == 0


def test_one_block_over_all_32_weights_breaks_the_accumulator_s_contract():
    """why the recompositions are cut in two: the emitter refuses, and so does the validator"""
    from plonky2_gpu_amd.stark import StarkAsm

    a = StarkAsm()
    with pytest.raises(ValueError, match="overflow"):
        for z in range(32):
            a.acc(a.local(3 + z), 1 << z)


def test_columns_are_the_reference_s():
    from plonky2_gpu_amd import logic_table as lt

    assert (lt.IS_AND, lt.IS_OR, lt.IS_XOR, lt.INPUT0, lt.INPUT1, lt.RESULT, lt.NUM_COLUMNS) == (0, 1, 2, 3, 259, 515, 523)
    assert (lt.IS_AND, lt.IS_OR, lt.IS_XOR, lt.INPUT0, lt.INPUT1, lt.RESULT, lt.NUM_COLUMNS) == \
        (lr.IS_AND, lr.IS_OR, lr.IS_XOR, lr.INPUT0.start, lr.INPUT1.start, lr.RESULT.start, lr.NUM_COLUMNS)
    assert (lt.OP_WORDS, lt.VAL_BITS, lt.PACKED_LEN, lt.PACKED_LIMB_BITS) == (17, 256, 8, 32) == (lr.OP_WORDS, lr.VAL_BITS, lr.PACKED_LEN, lr.PACKED_LIMB_BITS)
    assert (lt.OP_AND, lt.OP_OR, lt.OP_XOR) == (0, 1, 2)
    assert lt.limb_bit_cols_for_input(lt.INPUT1) == [list(r) for r in lr.limb_bit_cols_for_input(lr.INPUT1)]


def test_ctl_columns_are_the_operation_and_the_filter():
    from plonky2_gpu_amd import logic_table as lt

    data, flt = lt.ctl_data(), lt.ctl_filter()
    assert len(data) == 27
    assert [c.terms for c in data[:3]] == [[(0, 1)], [(1, 1)], [(2, 1)]]
    for i in range(8):
        assert data[3 + i].terms == [(3 + 32 * i + j, 1 << j) for j in range(32)]
        assert data[11 + i].terms == [(259 + 32 * i + j, 1 << j) for j in range(32)]
        assert data[19 + i].terms == [(515 + i, 1)]
    assert flt.terms == [(0, 1), (1, 1), (2, 1)] and all(c.constant == 0 for c in data + [flt])
    w = li.mixed(13)
    cols = _trace()
    rows = [[int(v) for v in cols[:, r]] for r in range(16)]
    looked = [tuple(ctl_ref.eval_column(sr.Base, c, row) for c in data) for row in rows if ctl_ref.eval_column(sr.Base, flt, row)]
    results = [[(x & y, x | y, x ^ y)[int(rec[0])] for x, y in zip(rec[1:9].tolist(), rec[9:17].tolist())] for rec in w]
    assert looked == [tuple([int(rec[0] == f) for f in range(3)] + rec[1:].tolist() + res) for rec, res in zip(w, results)]


def test_ops_to_words():
    from plonky2_gpu_amd import logic_table as lt

    x = sum((k + 1) << (32 * k) for k in range(8))
    w = lt.ops_to_words([(lt.OP_XOR, x, [9, 8, 7, 6, 5, 4, 3, 2]), (lt.OP_AND, 0, (1 << 256) - 1)])
    assert w.dtype == np.uint64 and w.shape == (2, 17)
    assert w.tolist() == [[2, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6, 5, 4, 3, 2], [0] + [0] * 8 + [(1 << 32) - 1] * 8]
    ops = lr.ops_from_words(w)
    assert (ops[0].operator, ops[0].input0) == (lr.XOR, x) and ops[1].result == 0
    assert lt.ops_to_words([]).shape == (0, 17)
    with pytest.raises(ValueError):
        lt.ops_to_words([(0, 1 << 256, 0)])
    with pytest.raises(ValueError):
        lt.ops_to_words([(0, [1] * 7, 0)])


# ---------------------------------------------------------------- compiling in units, device-free
def test_the_description_splits_and_precompiles_without_a_device(tmp_path, monkeypatch):
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import stark as pstark

    desc = lt.stark_desc(5, 2, si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,)))
    units = pstark.split_program(desc, 0)
    assert len(units) >= 1 and units[0][1][0] == 0 and units[-1][1][1] == 520
    assert all(units[k][1][1] == units[k + 1][1][0] for k in range(len(units) - 1))  # every constraint in exactly one unit, in order
    assert sum(int(op) in EMITS for unit, _ in units for op in np.asarray(unit).reshape(-1, 4)[:, 0]) == 520
    monkeypatch.setenv("PLONKY2_HIP_KERNEL_CACHE", str(tmp_path))
    pstark.precompile(desc, "poseidon", unit_instrs=0)
    assert any(tmp_path.iterdir())


# ---------------------------------------------------------------- one whole proof
def test_the_reference_prover_proves_the_table_and_its_verifier_accepts():
    """16 rows, rate 2, 2 challenges: stark_ref proves the program and verifies with the program and with the closures"""
    from oracle import accel

    instrs, immediates = _program()
    stark = lr.LogicTableStark(instrs, immediates)
    fp = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))
    trace = [[int(v) for v in col] for col in _trace()]
    hasher = gr.PoseidonHasher()
    with accel.c_backend():
        proof = sr.prove(hasher, stark, 2, fp, trace, [])
        assert sr.verify(hasher, stark, 2, fp, proof)
        assert sr.verify(hasher, stark, 2, fp, proof, evaluator="closure")
    assert len(proof["openings"]["local_values"]) == 523 and len(proof["openings"]["quotient_polys"]) == 4
