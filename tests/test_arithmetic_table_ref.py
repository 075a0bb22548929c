"""The arithmetic table on the CPU: tests/arithmetic_table_ref.py (the reference's generate functions and constraints restated from
the Rust, and this project's definition of the table's rows) against direct big-integer arithmetic and against its own
constraints; plonky2_gpu_amd/arithmetic_table.py (the constraints as a register program, the columns, the CTL columns) and the
native emitter gl_arithmetic_table_program against the restatement; tests/arithmetic_table_model.py (the device's division) against
Python's divmod, with the branches the instance list takes; and the constraint degree the reference declares against the one its
constraints have. Everything is exact; nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arithmetic_table_instances as ai  # noqa: E402
import arithmetic_table_model as am  # noqa: E402
import arithmetic_table_ref as ar  # noqa: E402
import ctl_ref  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = ar.P
EMITS = (sr.EMIT, sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW)
KIND_OF_EMIT = {sr.EMIT: ar.PLAIN, sr.EMIT_TRANSITION: ar.TRANSITION, sr.EMIT_LAST_ROW: ar.LAST_ROW}
_cache = {}


def _program():
    from plonky2_gpu_amd import arithmetic_table as at

    if "program" not in _cache:
        _cache["program"] = at.program()
    return _cache["program"]


def _trace(name, *args):
    key = (name,) + args
    if key not in _cache:
        w = getattr(ai, name)(*args)
        _cache[key] = (w, ar.trace_of_words(w))
    return _cache[key]


def _run(local, nxt, z_last=1, first=1, last=1):
    instrs, immediates = _program()
    consumer = sr.Consumer(sr.Base, [3], z_last, first, last)
    sr.run_program(sr.Base, instrs, immediates, local, nxt, [], consumer)
    return consumer.emitted


def _off_the_last_row(local, nxt):
    """the closures' values where the last-row constraint does not count"""
    return [0 if kind == ar.LAST_ROW else v for kind, v in ar.eval_constraints(local, nxt)]


# ---------------------------------------------------------------- the trace
def test_results_against_big_integer_arithmetic():
    """every operator's result as the table holds it from Python's own arithmetic on 256-bit integers (the EVM semantics of
    arithmetic/mod.rs; a zero modulus or denominator gives 0), the row count, the second rows' flags and the zero cells"""
    from plonky2_gpu_amd import arithmetic_table as at

    w, cols = _trace("edge")
    ops = ar.ops_from_words(w)
    assert {op for op, *_ in ops} == set(range(10))
    r = 0
    for op, in0, in1, in2 in ops:
        rows = [[int(v) for v in cols[:, r + k]] for k in range(2 if op in ar.MODULAR else 1)]
        assert [rows[0][f] for f in range(12)] == [int(f == op) for f in range(12)]
        assert ar.value_of(rows[0][12:28]) == in0 and ar.value_of(rows[0][28:44]) == in1
        m = 1 << 256
        expected = {ai.ADD: (in0 + in1) % m, ai.MUL: in0 * in1 % m, ai.SUB: (in0 - in1) % m, ai.LT: int(in0 < in1), ai.GT: int(in0 > in1),
                    ai.DIV: in0 // in2 if in2 else 0, ai.MOD: in0 % in2 if in2 else 0, ai.ADDMOD: (in0 + in1) % in2 if in2 else 0,
                    ai.SUBMOD: (in0 - in1) % in2 if in2 else 0, ai.MULMOD: in0 * in1 % in2 if in2 else 0}[op]
        assert ar.result_of_rows(op, rows) == expected == at.result(op, in0, in1, in2), (ar.NAMES[op], hex(in0), hex(in1), hex(in2))
        if op in ar.MODULAR:
            assert ar.value_of(rows[0][44:60]) == in2  # the modulus as given: zero stays zero
            assert rows[1][:12] == [0] * 12 and rows[1][76:] == [0] * 16 and rows[1][59] == int(in2 == 0)
            if op == ai.DIV:
                assert ar.value_of(rows[0][60:76]) == (in0 % in2 if in2 else in0)  # the remainder
        elif op in (ai.ADD, ai.SUB):
            assert rows[0][60:] == [0] * 32
        else:
            assert rows[0][76:] == [0] * 16
            if op in (ai.LT, ai.GT):
                assert rows[0][45:60] == [0] * 15
        assert all(v < P for row in rows for v in row)
        r += len(rows)
    assert r == ar.num_rows(w) and not cols[:, r:].any()


def test_signed_values_are_stored_as_p_minus_magnitude():
    """SUBMOD with in0 < in1 and a small modulus: a large negative quotient, limb by limb p - |limb|; an exact multiple gives a zero
    remainder of a negative input"""
    lv, nv = ar.rows_of_op(ai.SUBMOD, 0, ai.MAX, 1)
    assert lv[76:92] == [P - 0xFFFF] * 16 and nv[12:28] == [0] * 16 and ar.value_of(lv[60:76]) == 0
    lv, nv = ar.rows_of_op(ai.SUBMOD, 0, 21, 7)
    assert lv[76] == P - 3 and lv[60:76] == [0] * 16
    lv, nv = ar.rows_of_op(ai.SUBMOD, 3, 10, 1 << 255)
    assert ar.value_of(lv[60:76]) == (1 << 255) - 7 and lv[76] == P - 1
    lv, nv = ar.rows_of_op(ai.MULMOD, ai.MAX, ai.MAX, 1)
    assert ar.value_of(lv[76:92] + nv[12:28]) == ai.MAX * ai.MAX  # the 512-bit quotient
    (lv,) = ar.rows_of_op(ai.MUL, ai.MAX, ai.MAX, 0)
    assert any(v > P // 2 for v in lv[60:76])  # mul's aux carries are negative


def test_padding_and_shapes():
    assert ar.trace_of_words(ai.words([])).shape == (92, 2) and not ar.trace_of_words(ai.words([])).any()
    assert ar.trace_of_words(ai.words([(ai.ADD, 1, 2, 0)])).shape == (92, 2)
    assert ar.trace_of_words(ai.words([(ai.MOD, 1, 0, 2)])).shape == (92, 2)  # a modular operation's second row on row n - 1
    assert ar.trace_of_words(ai.words([(ai.MOD, 1, 0, 2), (ai.ADD, 1, 2, 0)])).shape == (92, 4)
    w = ai.every_operator()
    assert ar.num_rows(w) == 16 and ar.trace_of_words(w).shape == (92, 16)
    wide = ar.trace_of_words(w, 6)
    assert wide.shape == (92, 64) and (wide[:, :16] == ar.trace_of_words(w)).all() and not wide[:, 16:].any()
    with pytest.raises(AssertionError):
        ar.trace_of_words(w, 3)


# ---------------------------------------------------------------- the device's division
def test_the_division_model_divides():
    rng = np.random.default_rng(512)
    for _ in range(2000):
        d = int.from_bytes(rng.bytes(32), "little") >> int(rng.integers(0, 256)) or 1
        n = int.from_bytes(rng.bytes(64), "little") >> int(rng.integers(0, 512))
        assert am.divide(n, d) == divmod(n, d)
    for _, op, a, b, m in ai.DIVISION:
        n, d = ai.numerator_and_modulus(op, a, b, m)
        assert am.divide(n, d) == divmod(n, d)


def test_the_instance_list_takes_every_branch_of_the_division():
    """the quotient-digit estimate exact, one too large, two too large, the add-back, the estimate cut to 2^32 - 1, and every limb
    shift of the divisor's normalisation, over the divisions the edge list makes the device do"""
    total = am.Counters()
    for op, in0, in1, in2 in ar.ops_from_words(ai.edge()):
        if op in ar.MODULAR and in2:
            n, d = ai.numerator_and_modulus(op, in0, in1, in2)
            assert am.divide(n, d, total) == divmod(n, d)
    counts = total.as_dict()
    print(counts, total.limb_shift, total.top_equal)
    assert all(v > 0 for v in counts.values()), counts
    assert all(v > 0 for v in total.limb_shift) and total.top_equal > 0
    for name, op, a, b, m in ai.DIVISION:  # each found operand takes the branch it was found for
        c = am.Counters()
        am.divide(*ai.numerator_and_modulus(op, a, b, m), c)
        assert getattr(c, name) > 0, name


# ---------------------------------------------------------------- the constraints on the trace
@pytest.mark.parametrize("name,args", [("edge", ()), ("mixed", (23,)), ("every_operator", ())])
def test_every_constraint_holds_on_every_row(name, args):
    """all 246, through the program's interpreter and through the closures, second rows and padding rows included; the program and
    the closures give the same values"""
    w, cols = _trace(name, *args)
    n = cols.shape[1]
    if name != "edge":
        assert ar.violations(cols) == []
    for r in range(n):
        local, nxt = [int(v) for v in cols[:, r]], [int(v) for v in cols[:, (r + 1) % n]]
        if r == n - 1:
            nxt = [int(v) for v in np.random.default_rng(r).integers(0, P, size=92, dtype=np.uint64)]  # transitions do not count there
        closures = ar.eval_constraints(local, nxt)
        emitted = _run(local, nxt)
        assert emitted == [v for _, v in closures]
        for k, (kind, v) in enumerate(closures):
            if kind == ar.PLAIN or (kind == ar.TRANSITION and r != n - 1) or (kind == ar.LAST_ROW and r == n - 1):
                assert v == 0, (r, ar.group_of(k))


def test_the_emits_are_of_the_reference_s_kinds_in_its_order():
    instrs, _ = _program()
    kinds = [KIND_OF_EMIT[int(op)] for op in instrs[:, 0] if int(op) in EMITS]
    lv = [0] * 92
    assert kinds == [kind for kind, _ in ar.eval_constraints(lv, lv)]
    assert kinds[:83] == [ar.PLAIN] * 83 and kinds[83] == ar.LAST_ROW and kinds[84:] == [ar.TRANSITION] * 162


def test_rows_without_a_flag_satisfy_everything_whatever_their_cells():
    """the reference's generate_eval_consistency_not_modular tests: every constraint is filtered"""
    rng = np.random.default_rng(0x6FEB)
    for _ in range(4):
        local, nxt = ([int(v) for v in rng.integers(0, P, size=92, dtype=np.uint64)] for _ in range(2))
        local[:12] = [0] * 12
        assert _run(local, nxt, 5, 7, 11) == [0] * 246
        assert [v for _, v in ar.eval_constraints(local, nxt)] == [0] * 246


def test_program_and_closures_agree_on_random_rows():
    rng = np.random.default_rng(92)
    for _ in range(4):
        local, nxt = ([int(v) for v in rng.integers(0, P, size=92, dtype=np.uint64)] for _ in range(2))
        exp = [v for _, v in ar.eval_constraints(local, nxt)]
        assert _run(local, nxt) == exp and all(exp)


@pytest.mark.parametrize("op", sorted(ar.NAMES))
def test_a_corrupted_output_limb_breaks_a_constraint(op):
    """the reference's zero_modulus tests' second half, for every operator: one limb of the result changed"""
    rng = np.random.default_rng(op)
    for in2 in ((0, 12345 << 70) if op in ar.MODULAR else (0,)):
        rows = ar.rows_of_op(*ai.any_op(op, ai.MAX - 99, (1 << 200) + 5, in2))
        lv, nv = rows[0], rows[1] if len(rows) == 2 else [0] * 92
        assert _off_the_last_row(lv, nv) == [0] * 246 == _run(lv, nv, last=0)
        out = {ai.DIV: 76, ai.LT: 44, ai.GT: 44}.get(op, 60 if op in ar.MODULAR else 44)
        limb = out if op in (ai.LT, ai.GT) else out + int(rng.integers(0, 16))
        lv = list(lv)
        lv[limb] = (lv[limb] + 1 + int(rng.integers(0, 0xFFFE))) % P
        values = _run(lv, nv, last=0)
        assert any(values) and values == _off_the_last_row(lv, nv)


@pytest.mark.parametrize("op", ar.MODULAR)
def test_a_zero_modulus_gives_a_zero_result(op):
    rng = np.random.default_rng(op)
    for _ in range(3):
        a, b = (int.from_bytes(rng.bytes(32), "little") for _ in range(2))
        lv, nv = ar.rows_of_op(*ai.any_op(op, a, b, 0))
        assert ar.result_of_rows(op, [lv, nv]) == 0 and nv[59] == 1
        assert _run(lv, nv, last=0) == [0] * 246


# ---------------------------------------------------------------- the program
def test_program_validates_and_the_native_emitter_gives_the_same_words():
    from plonky2_gpu_amd import arithmetic_table as at

    instrs, immediates = _program()
    sr.validate_program(instrs, immediates, at.NUM_COLUMNS, 0)  # registers below 64, accumulators below 4, the ACC contract
    assert instrs.dtype == np.uint16 and sorted(immediates) == sorted([1 << 16, pow(1 << 16, P - 2, P), 1])
    regs = [int(row[1]) for row in instrs if int(row[0]) not in EMITS + (sr.ACC,)]
    assert max(regs) < 64 and not any(int(row[0]) == sr.ACC for row in instrs)
    n_instrs, n_immediates, num_constraints = at.native_program()
    assert n_instrs.shape == instrs.shape and (n_instrs == instrs).all()
    assert n_immediates == list(immediates)
    assert num_constraints == 246 == at.NUM_CONSTRAINTS == ar.NUM_CONSTRAINTS == sum(int(op) in EMITS for op in instrs[:, 0])
    desc = at.stark_desc(5, 2, si.fri_params(rate_bits=2))
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.quotient_degree_factor) == (92, 0, 5, 4)
    assert desc.pairs == ar.ArithmeticTableStark.pairs == [] and desc.num_zs == 0
    assert at.stark_desc(5, 2, si.fri_params(rate_bits=1), constraint_degree=3).quotient_degree_factor == 2


def test_columns_are_the_reference_s():
    from plonky2_gpu_amd import arithmetic_table as at

    assert [at.IS_ADD, at.IS_MUL, at.IS_SUB, at.IS_DIV, at.IS_MOD, at.IS_ADDMOD, at.IS_SUBMOD, at.IS_MULMOD, at.IS_LT, at.IS_GT, at.IS_SHL,
            at.IS_SHR] == list(range(12))
    assert (at.GENERAL_INPUT_0, at.GENERAL_INPUT_1, at.GENERAL_INPUT_2, at.GENERAL_INPUT_3, at.AUX_INPUT_0_LO, at.NUM_COLUMNS) == \
        (12, 28, 44, 60, 76, 92) == (ar.GENERAL_INPUT_0.start, ar.GENERAL_INPUT_1.start, ar.GENERAL_INPUT_2.start, ar.GENERAL_INPUT_3.start,
                                     ar.AUX_INPUT_0_LO.start, ar.NUM_COLUMNS)
    assert (at.MODULAR_QUO_INPUT_HI, at.MODULAR_AUX_INPUT, at.MODULAR_MOD_IS_ZERO, at.MODULAR_OUT_AUX_RED) == (12, 28, 59, 60) == \
        (ar.MODULAR_QUO_INPUT_HI.start, ar.MODULAR_AUX_INPUT.start, ar.MODULAR_MOD_IS_ZERO, ar.MODULAR_OUT_AUX_RED.start)
    assert len(ar.MODULAR_AUX_INPUT) == 31 and ar.MODULAR_AUX_INPUT.stop == 59
    assert [at.OP_ADD, at.OP_MUL, at.OP_SUB, at.OP_DIV, at.OP_MOD, at.OP_ADDMOD, at.OP_SUBMOD, at.OP_MULMOD, at.OP_LT, at.OP_GT] == list(range(10))
    assert at.OP_WORDS == 25 == ar.OP_WORDS and [at.rows_of(op) for op in range(10)] == [1, 1, 1, 2, 2, 2, 2, 2, 1, 1]


def test_ctl_columns_are_the_operation_and_the_filter():
    from plonky2_gpu_amd import arithmetic_table as at

    w, cols = _trace("every_operator")
    ops = ar.ops_from_words(w)
    rows = [[int(v) for v in cols[:, r]] for r in range(cols.shape[1])]
    limbs = lambda v: [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]  # noqa: E731
    looked = {}
    for kind in ("binary", "modular", "div"):
        data, flt = at.ctl_data(kind), at.ctl_filter(kind)
        assert all(c.constant == 0 for c in data + [flt])
        looked[kind] = [tuple(ctl_ref.eval_column(sr.Base, c, row) for c in data) for row in rows if ctl_ref.eval_column(sr.Base, flt, row)]
        assert all(ctl_ref.eval_column(sr.Base, flt, row) in (0, 1) for row in rows)
    assert len(at.ctl_data("binary")) == 5 + 24 and len(at.ctl_data("modular")) == 4 + 32 and len(at.ctl_data("div")) == 24
    assert at.ctl_filter("binary").terms == [(0, 1), (1, 1), (2, 1), (8, 1), (9, 1)] and at.ctl_filter("div").terms == [(3, 1)]
    assert at.ctl_filter("modular").terms == [(4, 1), (5, 1), (6, 1), (7, 1)]
    assert at.ctl_data("div")[8].terms == [(44, 1), (45, 1 << 16)] and at.ctl_data("div")[23].terms == [(90, 1), (91, 1 << 16)]
    assert looked["binary"] == [tuple([int(op == f) for f in (0, 1, 2, 8, 9)] + limbs(a) + limbs(b) + limbs(at.result(op, a, b, m)))
                                for op, a, b, m in ops if op in ar.ONE_ROW]
    assert looked["modular"] == [tuple([int(op == f) for f in (4, 5, 6, 7)] + limbs(a) + limbs(b) + limbs(m) + limbs(at.result(op, a, b, m)))
                                 for op, a, b, m in ops if op in ar.MODULAR and op != ai.DIV]
    assert looked["div"] == [tuple(limbs(a) + limbs(m) + limbs(a // m)) for op, a, b, m in ops if op == ai.DIV]


def test_ops_to_words():
    from plonky2_gpu_amd import arithmetic_table as at

    x = sum((k + 1) << (32 * k) for k in range(8))
    w = at.ops_to_words([(at.OP_MULMOD, x, [9, 8, 7, 6, 5, 4, 3, 2], 5), (at.OP_ADD, 0, (1 << 256) - 1, 0)])
    assert w.dtype == np.uint64 and w.shape == (2, 25)
    assert w.tolist() == [[7, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6, 5, 4, 3, 2, 5, 0, 0, 0, 0, 0, 0, 0], [0] + [0] * 8 + [(1 << 32) - 1] * 8 + [0] * 8]
    assert (w == ai.words([(7, x, sum(v << (32 * j) for j, v in enumerate([9, 8, 7, 6, 5, 4, 3, 2])), 5), (0, 0, ai.MAX, 0)])).all()
    assert at.ops_to_words([]).shape == (0, 25)
    with pytest.raises(ValueError):
        at.ops_to_words([(0, 1 << 256, 0, 0)])
    with pytest.raises(ValueError):
        at.ops_to_words([(0, [1] * 7, 0, 0)])
    with pytest.raises(ValueError):
        at.result(10, 1, 2, 3)


# ---------------------------------------------------------------- the constraint degree
FP3 = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))
FP5 = si.fri_params(rate_bits=2, cap_height=1, arity_bits=(2,))


def _prove_and_verify(cols, constraint_degree, fp, evaluator="program"):
    from oracle import accel

    instrs, immediates = _program()
    stark = ar.ArithmeticTableStark(instrs, immediates, constraint_degree)
    trace = [[int(v) for v in col] for col in cols]
    hasher = gr.PoseidonHasher()
    with accel.c_backend():
        proof = sr.prove(hasher, stark, 1, fp, trace, [])
        return sr.verify(hasher, stark, 1, fp, proof, evaluator=evaluator)


def _small_trace(with_div):
    """eight rows; column 59 (limb 15 of GENERAL_INPUT_2, mod_is_zero on a second row) is not the zero column: an ADD's result and
    a modulus reach into it"""
    ops = [(ai.ADD, (1 << 255) + 7, 2, 0), (ai.MULMOD, ai.MAX, ai.MAX - 4, (1 << 255) + 3), (ai.SUBMOD, 3, 1 << 100, 977)]
    ops.append((ai.DIV, (1 << 255) + 12345, 0, (1 << 70) + 1) if with_div else (ai.MOD, (1 << 255) + 12345, 0, (1 << 70) + 1))
    cols = ar.trace_of_words(ai.words(ops))
    assert cols.shape == (92, 8) and ar.violations(cols) == [] and cols[59].any() and bool(cols[ar.IS_DIV].any()) == with_div
    return cols


def test_a_trace_with_a_div_row_is_refused_at_the_reference_s_declared_degree_3():
    """constraint_degree() says 3 (arithmetic_stark.rs:104-106), but modular.rs:350 adds mod_is_zero * lv[IS_DIV] to the output's
    limb 0 and the less-than then yields filter * t * (2^16 - t) with that t: degree 5 wherever the IS_DIV column is not the zero
    polynomial. With quotient_degree_factor 2 the quotient does not fit its two chunks and the verifier's check at zeta fails."""
    with pytest.raises(AssertionError, match="Mismatch between evaluation and opening of quotient polynomial"):
        _prove_and_verify(_small_trace(with_div=True), 3, FP3)


def test_the_same_trace_verifies_at_degree_5():
    assert _prove_and_verify(_small_trace(with_div=True), 5, FP5)


def test_a_trace_without_div_rows_verifies_at_degree_3():
    """IS_DIV is the zero polynomial: the degree falls back to the reference's 3"""
    assert _prove_and_verify(_small_trace(with_div=False), 3, FP3)


# ---------------------------------------------------------------- one whole proof
def test_the_reference_prover_proves_a_trace_of_every_operator_and_its_verifier_accepts():
    """32 rows holding every operator, degree 5, rate 4: stark_ref proves the program and verifies with the program and with the
    closures"""
    from oracle import accel

    w = np.concatenate([ai.every_operator(), ai.mixed(10)])
    cols = ar.trace_of_words(w)
    assert cols.shape == (92, 32) and {int(x) for x in w[:, 0]} == set(range(10))
    instrs, immediates = _program()
    stark = ar.ArithmeticTableStark(instrs, immediates)
    trace = [[int(v) for v in col] for col in cols]
    hasher = gr.PoseidonHasher()
    with accel.c_backend():
        proof = sr.prove(hasher, stark, 2, FP5, trace, [])
        assert sr.verify(hasher, stark, 2, FP5, proof)
        assert sr.verify(hasher, stark, 2, FP5, proof, evaluator="closure")
    assert len(proof["openings"]["local_values"]) == 92 and len(proof["openings"]["quotient_polys"]) == 8
