"""The Poseidon table on the CPU: tests/poseidon_table_ref.py (the reference's permutation unit restated from the Rust) against
oracle/pyref.py's Poseidon and against its own constraints; plonky2_gpu_amd/poseidon_table.py (the constraints as a register
program, the columns, the CTL columns, the record helpers) and the native emitter gl_poseidon_table_program against the
restatement. Everything is exact; nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import poseidon_table_instances as pi  # noqa: E402
import poseidon_table_ref as pr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
from oracle import pyref  # noqa: E402

P = pr.P
EMITS = (sr.EMIT, sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW)
_cache = {}


def _program():
    from plonky2_gpu_amd import poseidon_table as pt

    if "program" not in _cache:
        _cache["program"] = pt.program()
    return _cache["program"]


def _trace(family="mixed", num_ops=20, degree_bits=5):
    key = (family, num_ops, degree_bits)
    if key not in _cache:
        _cache[key] = pr.trace_of_words(pi.FAMILIES[family](num_ops), degree_bits)
        _cache[key].setflags(write=False)
    return _cache[key]


def _emitted(local):
    instrs, immediates = _program()
    consumer = sr.Consumer(sr.Base, [3], 1, 1, 1)
    sr.run_program(sr.Base, instrs, immediates, local, local, [], consumer)
    return consumer.emitted


# ---------------------------------------------------------------- the columns
def test_the_column_map_equals_the_formulas():
    from plonky2_gpu_amd import poseidon_table as pt

    assert pt.NUM_COLUMNS == 249 == pr.NUM_COLUMNS and pt.IS_REAL == 248 == pr.IS_REAL
    assert (pt.INPUT, pt.START_FULL_FIRST, pt.START_PARTIAL, pt.START_FULL_SECOND, pt.OUTPUT) == (0, 12, 108, 152, 236)
    seen = []
    for i in range(12):
        assert pt.col_input(i) == pr.col_input(i) == i
        assert pt.col_output(i) == pr.col_output(i) == 236 + i
        seen.append(pt.col_input(i))
    for r in range(4):
        for i in range(12):
            assert pt.col_full_first_mid_sbox(r, i) == pr.col_full_first_mid_sbox(r, i) == 12 + 24 * r + i
            assert pt.col_full_first_after_mds(r, i) == pr.col_full_first_after_mds(r, i) == 24 + 24 * r + i
            assert pt.col_full_second_mid_sbox(r, i) == pr.col_full_second_mid_sbox(r, i) == 152 + 24 * r + i
            assert pt.col_full_second_after_mds(r, i) == pr.col_full_second_after_mds(r, i) == 164 + 24 * r + i
            seen += [12 + 24 * r + i, 24 + 24 * r + i, 152 + 24 * r + i, 164 + 24 * r + i]
    for r in range(22):
        assert pt.col_partial_mid_sbox(r) == pr.col_partial_mid_sbox(r) == 108 + 2 * r
        assert pt.col_partial_after_sbox(r) == pr.col_partial_after_sbox(r) == 109 + 2 * r
        seen += [108 + 2 * r, 109 + 2 * r]
    assert sorted(seen + [pt.IS_REAL]) == list(range(249))  # every column has exactly one meaning
    assert (pt.OP_WORDS, pt.KIND_START, pt.SPONGE_RATE, pt.SPONGE_WIDTH) == (13, 0, 8, 12)


def test_the_families_are_what_they_say():
    assert not pi.starts(50)[:, 0].any() and not pi.pairs(50)[:, 0].any() and not pi.pairs(50)[:, 9:].any()
    kinds = pi.leaves135(40)[:, 0].tolist()
    assert kinds == ([0] + [8] * 15 + [7]) * 2 + [0] + [8] * 5
    kinds = pi.mixed(2049)[:, 0].tolist()
    assert set(kinds) == set(range(9)) == set(pi.mixed(20)[:, 0].tolist()) and kinds[0] == 0
    lengths = np.diff([k for k, kind in enumerate(kinds) if kind == 0])
    assert 1 <= lengths.min() and lengths.max() <= 40 and len(set(lengths.tolist())) > 20
    assert (pi.mixed(300)[:, 0] == pi.mixed(2049)[:300, 0]).all()  # a shorter list has a prefix's shape
    kinds = pi.one_run(100)[:, 0].tolist()
    assert kinds == [0] + [8] * 99
    w = pi.noncanonical(257)
    for kind, positions in ((0, 12), (8, 8)):
        for word in pi.NONCANONICAL:
            rows = w[w[:, 0] == kind]
            assert all((rows[:, 1 + p] == np.uint64(word)).any() for p in range(positions)), (kind, hex(word))


# ---------------------------------------------------------------- the trace
@pytest.mark.parametrize("family", sorted(pi.FAMILIES))
def test_rows_chain_and_outputs_are_the_permutation(family):
    """every real row's OUTPUT is pyref.poseidon of its INPUT (asserted where the row is written); an ABSORB's INPUT is the OUTPUT
    of the row before it with its elements overwritten; the rows behind the records are the permutation of zero with IS_REAL 0"""
    w = pi.FAMILIES[family](21)
    cols = pr.trace_of_words(w)
    assert cols.shape == (249, 32) and (cols < np.uint64(P)).all()
    assert cols[248].tolist() == [1] * 21 + [0] * 11
    zero_out = pyref.poseidon([0] * 12)
    for r in range(21, 32):
        assert not cols[:12, r].any() and cols[236:248, r].tolist() == zero_out
    for r, rec in enumerate(w):
        kind = int(rec[0])
        if kind == 0:
            assert cols[:12, r].tolist() == [int(x) % P for x in rec[1:]]
        else:
            assert cols[:kind, r].tolist() == [int(x) % P for x in rec[1 : 1 + kind]]
            assert cols[kind:12, r].tolist() == cols[236 + kind : 248, r - 1].tolist()


def test_a_prefix_of_a_list_has_the_list_s_rows():
    """cutting a list only shortens its last run: the rows of the records that stay are unchanged, padding takes the others' place"""
    whole = _trace()
    for cut in (19, 10, 9, 1, 0):
        cols = pr.trace_of_words(pi.mixed(20)[:cut], 5)
        assert (cols[:, :cut] == whole[:, :cut]).all() and (cols[:, cut:] == whole[:, 31:32]).all()


@pytest.mark.parametrize("length", [1, 7, 8, 9, 16, 135])
def test_hash_no_pad_ops(length):
    from plonky2_gpu_amd import poseidon_table as pt

    message = [int(v) for v in np.random.default_rng([9, length]).integers(0, P, size=length, dtype=np.uint64)]
    ops = pt.hash_no_pad_ops(message)
    assert len(ops) == -(-length // 8) and ops[0][0] == pt.KIND_START and list(ops[0][1][8:]) == [0] * 4
    assert [op[0] for op in ops[1:]] == [8] * (len(ops) - 2) + ([length - 8 * (len(ops) - 1)] if len(ops) > 1 else [])
    cols = pr.trace_of_words(pt.ops_to_words(ops))
    assert cols[236:240, len(ops) - 1].tolist() == pyref.hash_no_pad(message)
    with pytest.raises(ValueError):
        pt.hash_no_pad_ops([])


def test_two_to_one_ops():
    from plonky2_gpu_amd import poseidon_table as pt

    rng = np.random.default_rng(21)
    left, right = ([int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64)] for _ in range(2))
    ops = pt.two_to_one_ops(left, right)
    assert len(ops) == 1
    cols = pr.trace_of_words(pt.ops_to_words(ops))
    assert cols[236:240, 0].tolist() == pyref.two_to_one(left, right)
    states = [[int(v) for v in rng.integers(0, P, size=12, dtype=np.uint64)] for _ in range(3)]
    cols = pr.trace_of_words(pt.ops_to_words(pt.permute_ops(states)))
    assert [cols[236:248, r].tolist() for r in range(3)] == [pyref.poseidon(s) for s in states]
    with pytest.raises(ValueError):
        pt.two_to_one_ops(left[:3], right)


def test_ops_to_words_and_its_refusals():
    from plonky2_gpu_amd import poseidon_table as pt

    ones = (1 << 64) - 1
    w = pt.ops_to_words([(0, list(range(1, 13))), (3, [7, ones, P]), (8, [5] * 8)])
    assert w.dtype == np.uint64 and w.shape == (3, 13)
    assert w.tolist() == [[0] + list(range(1, 13)), [3, 7, ones, P] + [0] * 9, [8] + [5] * 8 + [0] * 4]
    assert pr.inputs_of_words(w)[1][:3] == [7, ones - P, 0]
    assert pt.ops_to_words([]).shape == (0, 13)
    with pytest.raises(ValueError, match="kind of record 1 "):
        pt.ops_to_words([(0, [0] * 12), (9, [0] * 9)])
    with pytest.raises(ValueError, match="kind"):
        pt.ops_to_words([(-1, [])])
    with pytest.raises(ValueError, match="12 elements"):
        pt.ops_to_words([(0, [0] * 11)])
    with pytest.raises(ValueError, match="takes 3 elements"):
        pt.ops_to_words([(0, [0] * 12), (3, [1, 2, 3, 4])])
    with pytest.raises(ValueError, match="no record starts"):
        pt.ops_to_words([(2, [1, 2])])
    with pytest.raises(ValueError, match="64 bits"):
        pt.ops_to_words([(0, [1 << 64] + [0] * 11)])


# ---------------------------------------------------------------- the constraints on the trace
def test_every_constraint_holds_on_every_row():
    """all 237 on mixed at 2^5 rows, through the program's interpreter and through the closures, padding rows included"""
    cols = _trace()
    assert cols.shape == (249, 32) and set(cols[248].tolist()) == {0, 1}
    for r in range(32):
        local = [int(v) for v in cols[:, r]]
        assert _emitted(local) == [0] * 237 == pr.eval_constraints(local)


def test_one_changed_cell_breaks_a_constraint_for_each_column_in_turn():
    """row 7 of mixed(20) is a real row; the program and the closures name the same constraints"""
    cols = _trace()
    assert cols[248, 7] == 1
    for column in range(249):
        local = [int(v) for v in cols[:, 7]]
        local[column] = 2 if column == 248 else local[column] ^ 1  # IS_REAL: 0 is a boolean as well
        emitted = _emitted(local)
        assert any(emitted), column
        assert emitted == pr.eval_constraints(local)
    local = [int(v) for v in cols[:, 30]]  # a padding row: its INPUT is constrained like any other
    local[3] = 1
    assert any(_emitted(local))


# ---------------------------------------------------------------- the program
def test_program_and_closures_agree_on_random_rows():
    instrs, immediates = _program()
    rng = np.random.default_rng(249)
    for _ in range(4):
        local, nxt = ([int(v) % P for v in rng.integers(0, 1 << 64, size=pr.NUM_COLUMNS, dtype=np.uint64)] for _ in range(2))
        consumer = sr.Consumer(sr.Base, [3], 5, 7, 11)
        sr.run_program(sr.Base, instrs, immediates, local, nxt, [], consumer)
        exp = pr.eval_constraints(local)
        assert len(consumer.emitted) == len(exp) == 237 and all(exp)
        assert consumer.emitted == exp


def test_program_validates_and_the_native_emitter_gives_the_same_words():
    from plonky2_gpu_amd import poseidon_table as pt

    instrs, immediates = _program()
    sr.validate_program(instrs, immediates, pt.NUM_COLUMNS, 0)  # registers below 64, accumulators below 4, the ACC contract
    assert instrs.dtype == np.uint16
    n_instrs, n_immediates, num_constraints = pt.native_program()
    assert n_instrs.shape == instrs.shape and (n_instrs == instrs).all()
    assert n_immediates == list(immediates)
    assert num_constraints == 237 == pt.NUM_CONSTRAINTS == pr.NUM_CONSTRAINTS == sum(int(op) in EMITS for op in instrs[:, 0])
    assert all(int(op) == sr.EMIT for op in instrs[:, 0] if int(op) in EMITS)
    assert max(int(row[1]) for row in instrs if int(row[0]) not in EMITS + (sr.ACC,)) < 64
    accs = [int(row[1]) for row in instrs if int(row[0]) == sr.ACC]
    assert accs and max(accs) < 4
    assert set(pyref.ROUND_CONSTANTS) <= set(immediates)
    desc = pt.stark_desc(5, 2, si.fri_params(rate_bits=1))
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.quotient_degree_factor) == (249, 0, 3, 2)
    assert desc.pairs == pr.PoseidonTableStark.pairs == [] and desc.num_zs == 0


def test_the_library_takes_the_description():
    """the checks gl_stark_create makes on a program need no device: gl_stark_split_program runs them"""
    from plonky2_gpu_amd import poseidon_table as pt
    from plonky2_gpu_amd import stark as pstark

    desc = pt.stark_desc(5, 2, si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,)))
    units = pstark.split_program(desc, 0)
    assert len(units) >= 1 and units[0][1][0] == 0 and units[-1][1][1] == 237
    assert all(units[k][1][1] == units[k + 1][1][0] for k in range(len(units) - 1))  # every constraint in exactly one unit, in order


def test_ctl_columns_are_input_output_and_the_filter():
    from plonky2_gpu_amd import poseidon_table as pt

    data, flt = pt.ctl_data(), pt.ctl_filter()
    assert [c.terms for c in data] == [[(i, 1)] for i in range(12)] + [[(236 + i, 1)] for i in range(12)]
    assert flt.terms == [(248, 1)] and all(c.constant == 0 for c in data + [flt])
    cols = _trace()
    rows = [[int(v) for v in cols[:, r]] for r in range(32)]
    looked = [tuple(ctl_ref.eval_column(sr.Base, c, row) for c in data) for row in rows if ctl_ref.eval_column(sr.Base, flt, row)]
    assert len(looked) == 20 and all(list(pair[12:]) == pyref.poseidon(list(pair[:12])) for pair in looked)


# ---------------------------------------------------------------- whole proofs
@pytest.mark.parametrize("hasher,num_challenges", [("poseidon", 2), ("keccak", 1)])
def test_the_reference_prover_proves_the_table_and_refuses_a_changed_cell(hasher, num_challenges):
    """32 rows, rate 2, degree 3: stark_ref proves the program and verifies with the program and with the closures; the proof of the
    trace with one changed cell is refused at zeta. Keccak with 2 challenges would have quotient leaves of 4 elements, which
    KeccakHash<25> cannot hash: 1 there."""
    from oracle import accel

    instrs, immediates = _program()
    stark = pr.PoseidonTableStark(instrs, immediates)
    assert stark.constraint_degree == 3
    fp = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))
    trace = [[int(v) for v in col] for col in _trace()]
    h = {"poseidon": gr.PoseidonHasher, "keccak": gr.KeccakHasher}[hasher]()
    with accel.c_backend():
        proof = sr.prove(h, stark, num_challenges, fp, trace, [])
        assert sr.verify(h, stark, num_challenges, fp, proof)
        assert sr.verify(h, stark, num_challenges, fp, proof, evaluator="closure")
        assert len(proof["openings"]["local_values"]) == 249 and len(proof["openings"]["quotient_polys"]) == 2 * num_challenges
        trace[pr.col_partial_after_sbox(11)][7] ^= 1
        changed = sr.prove(h, stark, num_challenges, fp, trace, [])
        with pytest.raises(AssertionError, match="Mismatch between evaluation and opening"):
            sr.verify(h, stark, num_challenges, fp, changed)
