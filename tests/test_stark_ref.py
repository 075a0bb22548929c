"""tests/stark_ref.py pinned the way the reference pins its own STARK prover (starky/src/fibonacci_stark.rs tests: prove -> verify),
plus what a restatement needs on top: tampered proofs are rejected, the program interpreter and the hand-written closures of
tests/stark_instances.py agree constraint by constraint, the wire format round-trips through plonky2_gpu_amd.stark's parser, and the
program validator refuses what gl_stark_create refuses. Pure Python: degree_bits 3..5."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generic_prove_ref as gr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = sr.P
HASHERS = {"poseidon": gr.PoseidonHasher(), "keccak": gr.KeccakHasher()}
# name, degree_bits, num_challenges, fri parameters, hasher. A has 4 columns: KeccakHash<25> cannot hash its leaves.
CASES = [
    ("A", 4, 2, dict(rate_bits=1, cap_height=1, arity_bits=(1, 2)), "poseidon"),
    ("B", 3, 3, dict(rate_bits=1, cap_height=0, arity_bits=(1,)), "poseidon"),
    ("B", 4, 1, dict(rate_bits=2, cap_height=2, arity_bits=(3,)), "keccak"),
    ("C", 3, 2, dict(rate_bits=2, cap_height=0, arity_bits=()), "poseidon"),
    ("C", 5, 1, dict(rate_bits=2, cap_height=1, arity_bits=(2, 2)), "keccak"),
]
_proofs = {}


def _case(i):
    """(stark, num_challenges, fri_params, hasher, proof): proved once, never changed (the tests copy what they tamper with)"""
    if i not in _proofs:
        name, degree_bits, nch, fp, hasher = CASES[i]
        stark, fp = si.STARKS[name], si.fri_params(**fp)
        trace, pis = stark.make_trace(degree_bits, seed=i)
        _proofs[i] = (stark, nch, fp, HASHERS[hasher], sr.prove(HASHERS[hasher], stark, nch, fp, trace, pis))
    return _proofs[i]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_prove_then_verify(i):
    stark, nch, fp, hasher, proof = _case(i)
    assert sr.verify(hasher, stark, nch, fp, proof)
    assert sr.verify(hasher, stark, nch, fp, proof, evaluator="closure")
    assert (proof["permutation_zs_cap"] is None) == (not stark.pairs)
    assert len(proof["openings"]["quotient_polys"]) == nch * sr.quotient_degree_factor(stark)


def _bump_hash(h):
    return [(h[0] + 1) % P] + list(h[1:]) if isinstance(h, list) else bytes([h[0] ^ 1]) + bytes(h[1:])


@pytest.mark.parametrize("i", [0, 2, 3])
def test_tampered_proofs_are_rejected(i):
    stark, nch, fp, hasher, proof = _case(i)

    def rejected(change):
        p = copy.deepcopy(proof)
        change(p)
        with pytest.raises(AssertionError):
            sr.verify(hasher, stark, nch, fp, p)

    def opening(p):
        a, b = p["openings"]["local_values"][1]
        p["openings"]["local_values"][1] = ((a + 1) % P, b)

    def next_opening(p):
        a, b = p["openings"]["next_values"][0]
        p["openings"]["next_values"][0] = (a, (b + 1) % P)

    def quotient_opening(p):
        a, b = p["openings"]["quotient_polys"][-1]
        p["openings"]["quotient_polys"][-1] = ((a + 1) % P, b)

    def cap_word(p):
        p["trace_cap"][0] = _bump_hash(p["trace_cap"][0])

    def quotient_cap_word(p):
        p["quotient_polys_cap"][-1] = _bump_hash(p["quotient_polys_cap"][-1])

    def public_input(p):
        p["public_inputs"][0] = (p["public_inputs"][0] + 1) % P

    def fri_leaf(p):
        evals, sib = p["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"][0]
        evals[0] = (evals[0] + 1) % P

    for change in (opening, next_opening, quotient_opening, cap_word, quotient_cap_word, public_input, fri_leaf):
        rejected(change)
    if stark.pairs:
        def z_opening(p):
            a, b = p["openings"]["permutation_zs_next"][0]
            p["openings"]["permutation_zs_next"][0] = ((a + 1) % P, b)

        rejected(z_opening)


def test_this_starky_does_not_bind_unused_public_inputs():
    """the transcript observes neither the public inputs nor a digest (prover.rs:72-74): a public input only the constraints read
    is checked through them — every public input of A, B and C is (test above) — so nothing more is claimed here than that the
    proof bytes end in the public inputs"""
    stark, nch, fp, hasher, proof = _case(0)
    data = sr.proof_bytes(hasher, proof)
    assert data[-8 * stark.num_public_inputs :] == np.array(proof["public_inputs"], dtype="<u8").tobytes()


@pytest.mark.parametrize("name", sorted(si.STARKS))
def test_interpreter_and_closures_agree_on_random_rows(name):
    """over the base field and over the extension, constraint by constraint and in the accumulators; random rows satisfy nothing,
    so every constraint is non-zero and a swapped operand or a wrong emit kind shows"""
    stark = si.STARKS[name]
    rng = np.random.default_rng(5)
    rand = lambda k: [int(x) for x in rng.integers(0, P, size=k, dtype=np.uint64)]  # noqa: E731
    for F in (sr.Base, sr.Ext):
        elem = (lambda k: rand(k)) if F is sr.Base else (lambda k: list(zip(rand(k), rand(k))))
        for _ in range(4):
            local, nxt, pis = elem(stark.num_columns), elem(stark.num_columns), [F.lift(x) for x in rand(stark.num_public_inputs)]
            z_last, l_first, l_last = elem(3)
            alphas = rand(3)
            a, b = sr.Consumer(F, alphas, z_last, l_first, l_last), sr.Consumer(F, alphas, z_last, l_first, l_last)
            sr.eval_constraints(F, stark, local, nxt, pis, a, "program")
            sr.eval_constraints(F, stark, local, nxt, pis, b, "closure")
            assert a.emitted == b.emitted and a.accs == b.accs and len(a.emitted) >= (3 if name.startswith("D") else 5)  # D: 3 or 4
            assert all(c != F.zero for c in a.emitted)


def test_the_consumer_gives_the_first_constraint_the_highest_power():
    c = sr.Consumer(sr.Base, [3, 5], 1, 1, 1)
    for v in (2, 7, 11):
        c.constraint(v)
    assert c.accs == [2 * 9 + 7 * 3 + 11, 2 * 25 + 7 * 5 + 11]


def test_every_opcode_is_used_by_b():
    ops = {int(op) for op in si.B.instrs[:, 0]}
    assert ops == set(range(15)) - {sr.LOAD_CONST}
    assert any(v >= 1 << 32 for v in si.B.immediates)


@pytest.mark.parametrize("degree_bits", [3, 5])
def test_the_third_public_input_of_a_is_the_fibonacci_number(degree_bits):
    trace, pis = si.A.make_trace(degree_bits, seed=0)  # x0 = 0, x1 = 1
    fib = [0, 1]
    while len(fib) <= 1 << degree_bits:
        fib.append(fib[-1] + fib[-2])
    assert pis == [0, 1, fib[1 << degree_bits] % P]
    assert sorted(trace[2]) == sorted(trace[3])


def test_traces_satisfy_the_constraints_row_by_row():
    """on the subgroup itself: z_last vanishes on the last row, the Lagrange selectors are 1 on their row and 0 elsewhere"""
    for stark in si.STARKS.values():
        n = 8
        trace, pis = stark.make_trace(3, seed=3)
        for r in range(n):
            c = sr.Consumer(sr.Base, [1], int(r != n - 1), int(r == 0), int(r == n - 1))
            sr.eval_constraints(sr.Base, stark, [col[r] for col in trace], [col[(r + 1) % n] for col in trace], pis, c, "program")
            assert all(v == 0 for v in c.emitted), (stark.name, r)


def test_permutation_batches_and_zs():
    """B with 3 challenges: 9 instances in batches of 2, the last short; instance i of a batch uses challenge set i; Z is the
    exclusive prefix product and closes: the product of all quotients is 1"""
    sets = [[(10 * s + c, 100 * s + c) for c in range(3)] for s in range(2)]
    batches = sr.get_permutation_batches(si.B.pairs, sets, 3, 2)
    assert [len(b) for b in batches] == [2, 2, 2, 2, 1] and sr.num_zs(si.B, 3) == 5
    assert batches[0] == [(si.B.pairs[0], sets[0][0]), (si.B.pairs[0], sets[1][1])]
    assert batches[4] == [(si.B.pairs[2], sets[0][2])]
    trace, _ = si.B.make_trace(4, seed=1)
    rng = np.random.default_rng(1)
    sets = [[(int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64))) for _ in range(3)] for _ in range(2)]
    zs = sr.compute_permutation_z_polys(si.B, 3, trace, sets)
    assert len(zs) == 5 and all(z[0] == 1 for z in zs)
    # the last quotient closes the product: recompute it through the permutation check on the wrapped last row
    for i, z in enumerate(zs):
        c = sr.Consumer(sr.Base, [1], 0, 0, 0)
        sr.eval_permutation_checks(sr.Base, si.B, 3, [col[15] for col in trace], [zz[15] for zz in zs], [zz[0] for zz in zs], sets, c)
        assert c.emitted[len(zs) + i] == 0


@pytest.mark.parametrize("i", range(len(CASES)))
def test_wire_format_round_trip(i):
    from plonky2_gpu_amd import stark as pstark

    stark, nch, fp, hasher, proof = _case(i)
    desc = stark.desc(CASES[i][1], nch, fp)
    data = sr.proof_bytes(hasher, proof)
    parsed = pstark.proof_from_bytes(data, desc, hasher.name)
    assert pstark.proof_to_bytes(parsed, desc, hasher.name) == data
    assert sr.proof_bytes(hasher, parsed) == data
    assert sr.verify(hasher, stark, nch, fp, parsed)
    with pytest.raises((EOFError, ValueError)):
        pstark.proof_from_bytes(data[:-1], desc, hasher.name)
    with pytest.raises(ValueError):
        pstark.proof_from_bytes(data + b"\0", desc, hasher.name)


def test_the_validator_refuses():
    ok = si.B
    sr.validate_program(ok.instrs, ok.immediates, ok.num_columns, ok.num_public_inputs)

    def refused(instrs, imms=(), cols=4, pis=1):
        with pytest.raises(ValueError):
            sr.validate_program(np.array(instrs, dtype=np.uint16).reshape(-1, 4), list(imms), cols, pis)

    load, emit = [sr.LOAD_WIRE, 0, 0, 0], [sr.EMIT, 0, 0, 0]
    sr.validate_program(np.array([load, emit]), [], 4, 1)
    refused([[sr.LOAD_CONST, 0, 0, 0], emit])
    refused([load, [15, 1, 0, 0], emit])
    refused([[sr.LOAD_WIRE, 0, 4, 0], emit])  # column 4 of 4
    refused([[sr.LOAD_NEXT, 0, 4, 0], emit])
    refused([[sr.LOAD_PI, 0, 1, 0], emit])  # public input 1 of 1
    refused([[sr.LOAD_IMM, 0, 0, 0], emit])  # no immediates
    refused([load, [sr.ADD, 1, 0, 2], emit])  # register 2 never written
    refused([load, [sr.MULK, 1, 0, 64], emit])
    refused([load])  # no EMIT
    refused([load, [sr.ACC, 0, 0, 0], [sr.ACCR, 1, 0, 0], emit], imms=[1 << 32])  # weight not below 2^32
    refused([load, [sr.ACC, 4, 0, 0], emit], imms=[1])  # accumulator 4
    refused([load, [sr.ACCR, 1, 0, 0], emit], imms=[1])  # nothing accumulated
    many = [load] + [[sr.ACC, 0, 0, 0]] * 3 + [[sr.ACCR, 1, 0, 0], emit]
    refused(many, imms=[0xFFFFFFFF])  # (2^32 - 1)^2 per term: the halves could wrap
    sr.validate_program(np.array([load] + [[sr.ACC, 0, 0, 0]] * 3 + [[sr.ACCR, 1, 0, 0], emit]), [0x7FFFFFFF // 3], 4, 1)
    # the product's builder refuses the same things where it can
    from plonky2_gpu_amd.stark import StarkAsm

    a = StarkAsm()
    with pytest.raises(ValueError):
        a.const(0)
    with pytest.raises(ValueError):
        a.acc(a.local(0), 1 << 32)
    r = a.local(0)
    a.acc(r, 1 << 30)
    a.acc(r, 1 << 30)
    with pytest.raises(ValueError):
        a.acc(r, 1 << 30)  # 3 * 2^30 * (2^32 - 1) > 2^63


def test_gate_programs_do_not_know_the_stark_opcodes():
    """gate_programs_validate's restatement in the package's own gate-program checker: opcodes above ACCR are unknown there"""
    from plonky2_gpu_amd import gate_program as gp
    from plonky2_gpu_amd import stark as pstark

    assert gp.ACCR == 10 and pstark.LOAD_NEXT == 11 and pstark.EMIT_LAST_ROW == 14
    assert not hasattr(gp, "LOAD_NEXT")
