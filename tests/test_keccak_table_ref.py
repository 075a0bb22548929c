"""The Keccak-f table on the CPU: tests/keccak_table_ref.py (the reference's trace generator and constraints restated from the Rust)
against Keccak-f itself, and plonky2_gpu_amd/keccak_table.py (the constraints as a register program, the CTL columns) and the
native emitter gl_keccak_table_program against that restatement. Everything is exact; nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import keccak_ref  # noqa: E402
import keccak_table_ref as kr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = kr.P
_cache = {}


def _inputs(count, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(count, 25), dtype=np.uint64)


def _rows(count, n):
    if (count, n) not in _cache:
        _cache[count, n] = kr.generate_trace_rows(_inputs(count), n)
    return _cache[count, n]


def _program():
    from plonky2_gpu_amd import keccak_table as kt

    if "program" not in _cache:
        _cache["program"] = kt.program()
    return _cache["program"]


# ---------------------------------------------------------------- the trace
def test_output_limbs_are_keccak_f():
    """keccak_correctness_test (keccak_stark.rs:591-622) against tests/keccak_ref.py instead of tiny_keccak: 3 random inputs, the zero
    state, the all-ones state"""
    inputs = np.concatenate([_inputs(3), np.zeros((1, 25), dtype=np.uint64), np.full((1, 25), (1 << 64) - 1, dtype=np.uint64)])
    rows = kr.generate_trace_rows(inputs, 128)
    exp = keccak_ref.keccak_f1600(inputs)
    for k in range(len(inputs)):
        assert kr.outputs_of(rows, k) == [int(v) for v in exp[k]], k
    # the padding permutation behind them (rows 120 .. 127: cut after 8 rounds) starts from the zero state like permutation 3
    assert (rows[120:128] == rows[72:80]).all()
    assert rows.max() < 1 << 32 and kr.NUM_COLUMNS == 2430


@pytest.mark.parametrize("count,n", [(1, 32), (3, 128)])
def test_every_constraint_holds_on_every_row(count, n):
    rows = _rows(count, n)
    assert len(kr.eval_constraints([0] * kr.NUM_COLUMNS, [0] * kr.NUM_COLUMNS)) == kr.NUM_CONSTRAINTS == 842
    for r in range(n):
        assert kr.violated(rows, r) == [], r


def _violations(rows):
    out = []
    for r in range(len(rows)):
        for k in kr.violated(rows, r):
            group, base = kr.group_of(k), 0
            for name, count in kr.GROUPS:
                if name == group:
                    break
                base += count
            out.append((r, group, k - base))
    return out


# (column, row, bit of the cell that is flipped) -> [(row, group, index within the group)] of the constraints that break. Indices:
# c_prime / a_prime_parity 64 x + z; a_from_a_prime / a_prime_prime / next_input 2 (5 x + y) + limb.
TAMPER = {
    # round 5's flag on its own row: the two transitions around it, and A'''[0, 0]'s low limb — RC[5] = 0x80000001 has bits 0 and 31
    "a step flag": ((kr.reg_step(5), 5, 0), [(4, "round_flags_transition", 4), (5, "round_flags_transition", 5), (5, "a_prime_prime_prime_0_0", 0)]),
    # A[2, 3]'s low limb: the previous row's output and this row's recomposition from A', C, C'. Nothing ties it to C: the gap
    "an A limb": ((kr.reg_a(2, 3), 7, 9), [(6, "next_input", 26), (7, "a_from_a_prime", 26)]),
    # C[1, 10] enters C'[1, 10], C'[2, 10] (as C[x - 1]) and C'[0, 11] (as C[x + 1, z - 1]) and the low limbs of A[1, y] — and no
    # constraint that would tie C to the xor of A's bits: the reference's known gap, pinned as it is
    "a C bit": ((kr.reg_c(1, 10), 7, 0), [(7, "c_prime", 11), (7, "c_prime", 74), (7, "c_prime", 138)] + [(7, "a_from_a_prime", 10 + 2 * y) for y in range(5)]),
    "a C' bit": ((kr.reg_c_prime(1, 10), 7, 0), [(7, "c_prime", 74)] + [(7, "a_from_a_prime", 10 + 2 * y) for y in range(5)] + [(7, "a_prime_parity", 74)]),
    # A'[2, 3, 40]: A[2, 3]'s high limb, the parity of column (2, 40), and as bit 55 of B[3, 3] = rotl(A'[2, 3], 15) the high limbs of
    # A''[1, 3], A''[2, 3] and A''[3, 3]
    "an A' bit": ((kr.reg_a_prime(2, 3, 40), 7, 0), [(7, "a_from_a_prime", 27), (7, "a_prime_parity", 168), (7, "a_prime_prime", 17), (7, "a_prime_prime", 27),
                                                  (7, "a_prime_prime", 37)]),
    "an A'' limb": ((kr.reg_a_prime_prime(3, 1) + 1, 7, 4), [(7, "a_prime_prime", 33), (7, "next_input", 33)]),
    "an A''[0, 0] bit": ((kr.reg_a_prime_prime_0_0_bit(33), 7, 0), [(7, "a_prime_prime_0_0_bits", 1), (7, "a_prime_prime_prime_0_0", 1)]),
    "an A'''[0, 0] limb": ((kr.reg_a_prime_prime_prime(0, 0), 7, 2), [(7, "a_prime_prime_prime_0_0", 0), (7, "next_input", 0)]),
    # row 24 follows a round-23 row: its input is bound by its own row's constraints only, no transition reaches across permutations
    "an A limb behind a last round": ((kr.reg_a(4, 4), 24, 3), [(24, "a_from_a_prime", 48)]),
}


@pytest.mark.parametrize("what", sorted(TAMPER))
def test_one_flipped_bit_breaks_exactly_the_constraints_the_reference_has(what):
    (column, row, bit), expected = TAMPER[what]
    rows = _rows(1, 32).copy()
    rows[row, column] ^= np.uint64(1 << bit)
    assert _violations(rows) == expected


# ---------------------------------------------------------------- the program
def test_program_and_closures_agree_on_random_rows():
    """16 row pairs of uniformly random field elements (no valid trace): the interpreter of tests/stark_ref.py on program() gives the
    closures' values one by one, in order, each times its kind's factor"""
    instrs, immediates = _program()
    rng = np.random.default_rng(7)
    for _ in range(16):
        local, nxt = ([int(v) % P for v in rng.integers(0, 1 << 64, size=kr.NUM_COLUMNS, dtype=np.uint64)] for _ in range(2))
        z_last, l_first, l_last = (int(v) % P for v in rng.integers(0, 1 << 64, size=3, dtype=np.uint64))
        consumer = sr.Consumer(sr.Base, [3], z_last, l_first, l_last)
        sr.run_program(sr.Base, instrs, immediates, local, nxt, [], consumer)
        factor = {kr.ALL: 1, kr.TRANSITION: z_last, kr.FIRST_ROW: l_first}
        exp = [v * factor[kind] % P for kind, v in kr.eval_constraints(local, nxt)]
        assert len(consumer.emitted) == len(exp) == 842
        assert consumer.emitted == exp


def test_program_validates_and_the_native_emitter_gives_the_same_words():
    from plonky2_gpu_amd import keccak_table as kt

    instrs, immediates = _program()
    sr.validate_program(instrs, immediates, kt.NUM_COLUMNS, 0)
    assert instrs.dtype == np.uint16 and 40000 < instrs.shape[0] < 65536 and all(0 <= v < 1 << 32 for v in immediates)
    n_instrs, n_immediates, num_constraints = kt.native_program()
    assert n_instrs.shape == instrs.shape and (n_instrs == instrs).all()
    assert n_immediates == list(immediates)
    assert num_constraints == 842 == sum(int(op) in (sr.EMIT, sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW) for op in instrs[:, 0])
    desc = kt.stark_desc(5, 2, si.fri_params(rate_bits=1))
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.pairs, desc.quotient_degree_factor) == (2430, 0, 3, [], 2)


def test_column_functions_are_the_reference_s():
    from plonky2_gpu_amd import keccak_table as kt

    assert kt.NUM_COLUMNS == kr.NUM_COLUMNS
    for x in range(5):
        for y in range(5):
            assert kt.reg_a(x, y) == kr.reg_a(x, y) and kt.reg_a_prime_prime(x, y) == kr.reg_a_prime_prime(x, y)
            assert kt.reg_a_prime_prime_prime(x, y) == kr.reg_a_prime_prime_prime(x, y)
            for z in range(64):
                assert kt.reg_a_prime(x, y, z) == kr.reg_a_prime(x, y, z) and kt.reg_b(x, y, z) == kr.reg_b(x, y, z)
        for z in range(64):
            assert kt.reg_c(x, z) == kr.reg_c(x, z) and kt.reg_c_prime(x, z) == kr.reg_c_prime(x, z)
    assert [kt.reg_step(i) for i in range(24)] == list(range(24))
    assert [kt.reg_a_prime_prime_0_0_bit(i) for i in range(64)] == [kr.reg_a_prime_prime_0_0_bit(i) for i in range(64)]
    assert [kt.reg_output_limb(i) for i in range(50)] == [kr.reg_output_limb(i) for i in range(50)]


def test_ctl_columns_are_inputs_outputs_and_the_last_round():
    from plonky2_gpu_amd import keccak_table as kt

    inputs = _inputs(3)
    rows, exp = _rows(3, 128), keccak_ref.keccak_f1600(inputs)
    data, flt = kt.ctl_data(), kt.ctl_filter()
    assert len(data) == 100 and all(len(c.terms) == 1 and c.constant == 0 for c in data + [flt])
    limbs = lambda words: [int(w) >> (32 * h) & 0xFFFFFFFF for w in words for h in range(2)]  # noqa: E731
    for r in range(128):
        row = [int(v) for v in rows[r]]
        assert ctl_ref.eval_column(sr.Base, flt, row) == (1 if r % 24 == 23 else 0)
    for k in range(3):
        first, last = [int(v) for v in rows[24 * k]], [int(v) for v in rows[24 * k + 23]]
        assert [ctl_ref.eval_column(sr.Base, c, first) for c in data[:50]] == limbs(inputs[k])
        assert [ctl_ref.eval_column(sr.Base, c, last) for c in data[50:]] == limbs(exp[k])
        # where the filter is 1 the "input" columns show the state entering round 23 — the output of row 24 k + 22 —, not the
        # permutation's input: the lookup as the reference has it
        before = [int(v) for v in rows[24 * k + 22]]
        assert [ctl_ref.eval_column(sr.Base, c, last) for c in data[:50]] == [before[kr.reg_output_limb(i)] for i in range(50)] != limbs(inputs[k])


# ---------------------------------------------------------------- one whole proof
def test_the_reference_prover_proves_the_table_and_its_verifier_accepts():
    """32 rows (one permutation and a cut padding permutation), rate 2, 5 query rounds, 2 challenges: stark_ref proves the program and
    verifies with the program and with the closures. The one slow CPU test (hashes, trees and transforms in C; the algebra Python)."""
    from oracle import accel

    instrs, immediates = _program()
    stark = kr.KeccakTableStark(instrs, immediates)
    fp = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))
    trace = [[int(v) for v in col] for col in _rows(1, 32).T]
    hasher = gr.PoseidonHasher()
    with accel.c_backend():
        proof = sr.prove(hasher, stark, 2, fp, trace, [])
        assert sr.verify(hasher, stark, 2, fp, proof)
        assert sr.verify(hasher, stark, 2, fp, proof, evaluator="closure")
    assert len(proof["openings"]["local_values"]) == 2430 and len(proof["openings"]["quotient_polys"]) == 4 and proof["permutation_zs_cap"] is None
