"""Whole proofs with KeccakGoldilocksConfig (plonky2/src/plonk/config.rs:120-128): gl_circuit_create_h(GL_HASHER_KECCAK25) + gl_prove /
gl_prove_zk / gl_prove_many against tests/generic_prove_ref.py with KeccakHasher, byte for byte.

The Keccak circuit dicts are tests/plonk_instance.py's with the preprocessed commitment and the circuit digest recomputed by the
generic reference (gr.with_hasher). make_circuit's default shape — 12 routed wires, quotient_degree_factor 8, 2 challenges — has a
Zs / partial products commitment of 2 * (1 + 1) = 4 columns, the leaf width KeccakHash<25>::hash_or_noop panics on (plonk/config.rs:
56-63; the library refuses such a circuit, see the refusals below), so the provable cases take 3 challenges (leaves of 6 and 24
elements) or 1 (leaves of 2, which are their own hash, and 8)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generic_prove_ref as gr  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401
from plonk_instance import make_circuit, make_full_circuit  # noqa: E402

P = 0xFFFFFFFF00000001
KECCAK_HASHER, POSEIDON_HASHER = gr.KeccakHasher(), gr.PoseidonHasher()


def _check(gpu, plain, wires, pis, compile_gates=True, salts=None, give_digest=False, verify=True):
    """prove `plain` (a plonk_instance circuit) as a Keccak circuit on the device and with the reference; returns (circuit, bytes).
    `verify`: the reference's verifier runs on the parsed bytes (hash by hash in numpy: seconds at 28 queries, so the one larger
    circuit, whose bytes equal the reference prover's like the others', leaves it out)"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import serialization

    circuit = gr.with_hasher(KECCAK_HASHER, plain)
    exp = gr.proof_bytes(KECCAK_HASHER, gr.prove(KECCAK_HASHER, circuit, wires, pis, salts=None if salts is None else salts.tolist()))
    nc = pg.NativeCircuit(gpu, circuit if give_digest else dict(circuit, circuit_digest=None), compile_gates=compile_gates, hasher="keccak")
    try:
        assert nc.circuit_digest == circuit["circuit_digest"]  # derived on the device = the reference's (or the one given)
        assert nc.constants_sigmas_cap == circuit["constants_sigmas"]["cap"]
        data = nc.prove_bytes(wires, pis, salts=salts)
        assert data == exp
        assert nc.prove_bytes(wires, pis, salts=salts) == exp  # recycled buffers
    finally:
        nc.close()
    parsed = serialization.proof_from_bytes(data, circuit, hasher=serialization.KECCAK)
    assert serialization.proof_to_bytes(parsed, hasher=serialization.KECCAK) == data
    assert not verify or gr.verify(KECCAK_HASHER, circuit, parsed)
    return circuit, data


# degree_bits, arity_bits, cap_height (caps of 4, 8 and 16 observed elements: a partial block, exactly one block, two blocks), then
# two_groups, num_challenges, compile_gates
SMALL = [(4, (2,), 0, False, 3, True), (4, (2, 2), 1, True, 3, True), (5, (3,), 2, False, 1, False), (3, (), 0, True, 3, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits,arity_bits,cap_height,two_groups,num_challenges,compile_gates", SMALL)
def test_small_keccak_proofs_equal_the_reference(gpu, degree_bits, arity_bits, cap_height, two_groups, num_challenges, compile_gates):
    plain, wires, pis = make_circuit(degree_bits, seed=2 + degree_bits, two_groups=two_groups, arity_bits=arity_bits, cap_height=cap_height,
                                     num_challenges=num_challenges)
    _check(gpu, plain, wires, pis, compile_gates=compile_gates, give_digest=degree_bits == 3)


@pytest.mark.gpu
def test_full_gate_list_keccak_proof_equals_the_reference(gpu):
    """135 wires, 80 routed, every gate kind of the ed25519 list"""
    from oracle import accel

    with accel.c_backend():  # the reference's Poseidon side (public-inputs hash, transcript) and its transforms in C
        plain, wires, pis = make_full_circuit(4, arity_bits=(2, 2))
        _check(gpu, plain, wires, pis)


@pytest.mark.gpu
def test_a_2e10_row_keccak_proof_equals_the_reference(gpu):
    """multi-wave trees, the two-pass LDE, 28 query openings, caps of 16 hashes"""
    from oracle import accel

    with accel.c_backend():
        plain, wires, pis = make_circuit(10, arity_bits=(4, 4), cap_height=4, num_queries=28, pow_bits=8, num_challenges=3)
        _check(gpu, plain, wires, pis, verify=False)


@pytest.mark.gpu
def test_hiding_keccak_proof_equals_the_reference(gpu):
    """gl_prove_zk on a Keccak handle: the salt columns are hashed with the leaf (2 challenges: 4 + 4 salt elements per leaf)"""
    plain, wires, pis = make_circuit(4, seed=6, arity_bits=(2, 2))
    plain = dict(plain, fri_params=dict(plain["fri_params"], hiding=True))
    n_ext = 1 << (4 + plain["fri_params"]["rate_bits"])
    salts = np.random.default_rng(606).integers(0, P, size=(3, 4, n_ext), dtype=np.uint64)
    _check(gpu, plain, wires, pis, salts=salts)


@pytest.mark.gpu
def test_prove_many_on_a_keccak_handle_and_the_size_of_a_keccak_proof(gpu):
    """three proofs, two in flight, each the one gl_prove makes alone; and a Keccak proof is smaller than the Poseidon proof of the
    same circuit by exactly 7 bytes per hash it carries (32 - 25; caps and Merkle siblings, counted from the parsed proof)"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import serialization

    plain, wires, pis = make_circuit(4, seed=8, arity_bits=(2, 2), num_challenges=3)
    circuit = gr.with_hasher(KECCAK_HASHER, plain)
    nc = pg.NativeCircuit(gpu, dict(circuit, circuit_digest=None), hasher="keccak")
    other = pg.Context(0)
    try:
        bufs = [pg.DeviceBuffer.from_host(gpu, np.ascontiguousarray(np.array(wires, dtype=np.uint64).reshape(-1))) for _ in range(3)]
        alone = [nc.prove_bytes(b, pis) for b in bufs]
        assert alone[0] == gr.proof_bytes(KECCAK_HASHER, gr.prove(KECCAK_HASHER, circuit, wires, pis))
        assert nc.prove_many(bufs, [pis] * 3, [gpu, other]) == alone
        nc.trim()
        assert nc.prove_bytes(bufs[0], pis) == alone[0]
        for b in bufs:
            b.free()
    finally:
        nc.close()
        other.close()
    pc = pg.NativeCircuit(gpu, dict(plain, circuit_digest=None))
    try:
        poseidon = pc.prove_bytes(wires, pis)
    finally:
        pc.close()
    parsed = serialization.proof_from_bytes(alone[0], circuit, hasher=serialization.KECCAK)
    hashes = gr.count_hashes(parsed)
    assert hashes == gr.count_hashes(serialization.proof_from_bytes(poseidon, plain)) and hashes > 0
    assert len(poseidon) - len(alone[0]) == 7 * hashes


def _create_h(gpu, hasher, circuit):
    """gl_circuit_create_h through NativeCircuit's own marshalling; returns the error (None if a handle came back)"""
    import plonky2_gpu_amd as pg

    try:
        nc = pg.NativeCircuit(gpu, dict(circuit, circuit_digest=None), hasher=hasher)
    except pg.Plonky2HipError as e:
        return e
    nc.close()
    return None


@pytest.mark.gpu
def test_refusals(gpu):
    """an unknown hasher, and the circuits that would build a Merkle leaf of 4 elements: GL_E_INVALID with the cause named, no handle,
    and the library goes on working"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    good, wires, pis = make_circuit(4, seed=9, arity_bits=(2, 2), num_challenges=3)
    e = _create_h(gpu, 7, good)
    assert e is not None and e.code == _lib.GL_E_INVALID and "hasher" in str(e)
    # *circuit is not written
    h = ctypes.c_void_p(0x1234)
    desc = _lib.GlCircuitDesc()
    with pytest.raises(pg.Plonky2HipError):
        _lib.call("gl_circuit_create_h", 7, ctypes.byref(desc), ctypes.byref(h), gpu.ptr)
    assert h.value == 0x1234
    cases = [(make_circuit(4, seed=9, arity_bits=(2, 1), num_challenges=3)[0], "arity_bits = 1"),
             (make_circuit(4, seed=9, arity_bits=(1, 2), num_challenges=3)[0], "arity_bits = 1"),
             (make_circuit(4, seed=9, two_groups=True, arity_bits=(2, 2), num_challenges=1, quotient_degree_factor=4)[0], "quotient"),
             (make_circuit(4, seed=9, arity_bits=(2, 2))[0], "partial products")]
    for circuit, word in cases:
        e = _create_h(gpu, "keccak", circuit)
        assert e is not None and e.code == _lib.GL_E_INVALID and word in str(e), (word, str(e))
        if word == "quotient":
            assert _create_h(gpu, "poseidon", circuit) is None  # a Poseidon circuit of that shape is fine
    _check(gpu, good, wires, pis)


@pytest.mark.gpu
def test_poseidon_through_gl_circuit_create_h_is_gl_circuit_create(gpu, monkeypatch):
    """GL_HASHER_POSEIDON forwards: the handle proves to the bytes of a gl_circuit_create handle (NativeCircuit goes through
    gl_circuit_create_h; the second circuit is made with its call redirected to the un-suffixed entry point) and of the oracle"""
    import plonky2_gpu_amd as pg
    from oracle import prove_ref, serialize_ref
    from plonky2_gpu_amd import _lib

    circuit, wires, pis = make_circuit(4, seed=1)
    called = []
    real_call = _lib.call

    def unsuffixed(name, *args):
        called.append(name)
        return real_call("gl_circuit_create", *args[1:]) if name == "gl_circuit_create_h" else real_call(name, *args)

    data = []
    for redirect in (False, True):
        if redirect:
            monkeypatch.setattr(_lib, "call", unsuffixed)
        nc = pg.NativeCircuit(gpu, dict(circuit, circuit_digest=None), hasher="poseidon")
        try:
            assert nc.circuit_digest == circuit["circuit_digest"] and nc.constants_sigmas_cap == circuit["constants_sigmas"]["cap"]
            data.append(nc.prove_bytes(wires, pis))
        finally:
            nc.close()
    assert "gl_circuit_create_h" in called
    assert data[0] == data[1] == serialize_ref.proof_bytes(prove_ref.prove(circuit, wires, pis))
