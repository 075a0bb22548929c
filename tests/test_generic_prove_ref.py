"""The pins of tests/generic_prove_ref.py, the prover and verifier with the Merkle hasher as a parameter (CPU only):
with PoseidonHasher it IS oracle/prove_ref.py + serialize_ref.py (same dict, same bytes); with KeccakHasher its proofs are accepted
by its verifier and tampered ones are not; KeccakHasher.to_vec on vectors written out by hand."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generic_prove_ref as gr  # noqa: E402
from oracle import prove_ref, serialize_ref  # noqa: E402
from plonk_instance import make_circuit  # noqa: E402

P = 0xFFFFFFFF00000001
POSEIDON, KECCAK = gr.PoseidonHasher(), gr.KeccakHasher()


def _salts(circuit, seed):
    fp = circuit["fri_params"]
    n_ext = 1 << (circuit["degree_bits"] + fp["rate_bits"])
    return np.random.default_rng(seed).integers(0, P, size=(3, 4, n_ext), dtype=np.uint64).tolist()


@pytest.mark.parametrize("two_groups", [False, True])
def test_with_the_poseidon_hasher_it_is_the_oracle(two_groups):
    circuit, wires, pis = make_circuit(4, seed=3, two_groups=two_groups)
    mine = gr.with_hasher(POSEIDON, circuit)
    assert mine["circuit_digest"] == circuit["circuit_digest"]
    assert mine["constants_sigmas"] == circuit["constants_sigmas"]
    exp = prove_ref.prove(circuit, wires, pis)
    got = gr.prove(POSEIDON, mine, wires, pis)
    assert got == exp
    assert gr.proof_bytes(POSEIDON, got) == serialize_ref.proof_bytes(exp)
    assert gr.verify(POSEIDON, mine, got) and prove_ref.verify(circuit, got)


def test_with_the_poseidon_hasher_it_is_the_oracle_on_a_hiding_circuit():
    circuit, wires, pis = make_circuit(4, seed=5)
    circuit = dict(circuit, fri_params=dict(circuit["fri_params"], hiding=True))
    salts = _salts(circuit, 7)
    exp = prove_ref.prove(circuit, wires, pis, salts=salts)
    got = gr.prove(POSEIDON, circuit, wires, pis, salts=salts)
    assert got == exp
    assert gr.proof_bytes(POSEIDON, got) == serialize_ref.proof_bytes(exp)
    assert gr.verify(POSEIDON, circuit, got)


# make_circuit's default shape (12 routed wires, quotient_degree_factor 8, 2 challenges) has one partial product per challenge:
# its Zs / partial products commitment has 2 * (1 + 1) = 4 columns, the leaf KeccakHash<25>::hash_or_noop panics on
# (plonk/config.rs:56-63). The Keccak circuits here therefore take 3 challenges (leaves of 6 and 24).
KECCAK_SHAPE = dict(seed=3, arity_bits=(2, 2), cap_height=1, num_challenges=3)


@pytest.fixture(scope="module")
def keccak_proof():
    circuit, wires, pis = make_circuit(4, **KECCAK_SHAPE)
    circuit = gr.with_hasher(KECCAK, circuit)
    return circuit, gr.prove(KECCAK, circuit, wires, pis)


def _flip(h, byte=3):
    b = bytearray(h)
    b[byte] ^= 0x10
    return bytes(b)


def test_a_keccak_proof_is_accepted_and_tampered_ones_are_not(keccak_proof):
    circuit, proof = keccak_proof
    assert isinstance(circuit["circuit_digest"], bytes) and len(circuit["circuit_digest"]) == 25
    assert all(isinstance(h, bytes) and len(h) == 25 for h in proof["wires_cap"])
    assert gr.verify(KECCAK, circuit, proof)
    # a flipped byte in a sibling: of an initial tree's opening and of a FRI layer's
    bad = copy.deepcopy(proof)
    evals, sib = bad["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"][1]
    bad["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"][1] = (evals, [_flip(sib[0])] + sib[1:])
    with pytest.raises(AssertionError, match="initial Merkle proof"):
        gr.verify(KECCAK, circuit, bad)
    bad = copy.deepcopy(proof)
    step = bad["opening_proof"]["query_round_proofs"][1]["steps"][0]
    step["merkle_proof"][-1] = _flip(step["merkle_proof"][-1], 24)
    with pytest.raises(AssertionError):
        gr.verify(KECCAK, circuit, bad)
    # a flipped byte in a cap: the transcript changes with it (observe_cap), so does every challenge
    for key in ("wires_cap", "quotient_polys_cap"):
        bad = copy.deepcopy(proof)
        bad[key][0] = _flip(bad[key][0], 24)
        with pytest.raises(AssertionError):
            gr.verify(KECCAK, circuit, bad)
    bad = copy.deepcopy(proof)
    bad["opening_proof"]["commit_phase_merkle_caps"][1][1] = _flip(bad["opening_proof"]["commit_phase_merkle_caps"][1][1], 0)
    with pytest.raises(AssertionError):
        gr.verify(KECCAK, circuit, bad)
    # one changed opening
    bad = copy.deepcopy(proof)
    a, b = bad["openings"]["wires"][2]
    bad["openings"]["wires"][2] = ((a + 1) % P, b)
    with pytest.raises(AssertionError):
        gr.verify(KECCAK, circuit, bad)
    # and the circuit digest is part of the transcript
    with pytest.raises(AssertionError):
        gr.verify(KECCAK, dict(circuit, circuit_digest=_flip(circuit["circuit_digest"], 24)), proof)


def test_the_keccak_wire_format_carries_25_bytes_per_hash(keccak_proof):
    circuit, proof = keccak_proof
    plain, wires, pis = make_circuit(4, **KECCAK_SHAPE)
    poseidon_proof = gr.prove(POSEIDON, plain, wires, pis)
    assert gr.count_hashes(proof) == gr.count_hashes(poseidon_proof)
    assert len(gr.proof_bytes(POSEIDON, poseidon_proof)) - len(gr.proof_bytes(KECCAK, proof)) == 7 * gr.count_hashes(proof)


def test_keccak_to_vec_on_hand_written_vectors():
    assert KECCAK.to_vec(b"\xff" * 25) == [2**56 - 1, 2**56 - 1, 2**56 - 1, 2**32 - 1]
    assert KECCAK.to_vec(bytes(range(25))) == [0x06050403020100, 0x0D0C0B0A090807, 0x14131211100F0E, 0x18171615]
    assert KECCAK.to_vec(bytes(25)) == [0, 0, 0, 0]
    one_per_chunk = bytearray(25)
    one_per_chunk[6], one_per_chunk[7], one_per_chunk[20], one_per_chunk[21], one_per_chunk[24] = 0x80, 0x01, 0x02, 0x03, 0x04
    assert KECCAK.to_vec(bytes(one_per_chunk)) == [0x80 << 48, 0x01, 0x02 << 48, 0x03 | (0x04 << 24)]
    assert all(v < P for v in KECCAK.to_vec(b"\xff" * 25))


def test_a_four_element_leaf_panics_like_the_reference():
    with pytest.raises(ValueError):
        KECCAK.hash_or_noop([1, 2, 3, 4])
    assert KECCAK.hash_or_noop([1, 2, 3]) == (1).to_bytes(8, "little") + (2).to_bytes(8, "little") + (3).to_bytes(8, "little") + b"\0"
    # arity_bits (2, 1): the second reduction's leaves are 2 extension elements
    circuit, wires, pis = make_circuit(4, seed=3, num_challenges=3)
    with pytest.raises(ValueError):
        gr.prove(KECCAK, gr.with_hasher(KECCAK, circuit), wires, pis)
    # 2 challenges x (Z + one partial product): a 4-column commitment
    circuit, wires, pis = make_circuit(4, seed=3, arity_bits=(2, 2))
    with pytest.raises(ValueError):
        gr.prove(KECCAK, gr.with_hasher(KECCAK, circuit), wires, pis)
