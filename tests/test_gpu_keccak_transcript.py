"""gl_challenger_step with Keccak digest sources (GlObserveSrc.planar_len == GL_OBSERVE_KECCAK_DIGESTS): how the transcript of a
KeccakGoldilocksConfig proof observes a hash — BytesHash<25>::to_vec (hash/hash_types.rs:179-189), four field elements per digest,
its 25 bytes in chunks of 7, 7, 7 and 4 — read from the 32-byte digest slots the Keccak tree kernels write. Held against
oracle/fri_ref.Challenger fed the to_vec elements of tests/generic_prove_ref.KeccakHasher: the challenges and the whole 32-word
state, bit for bit. Goes through plonky2_gpu_amd.challenger.DeviceChallenger, the Python wrapper of the device transcript."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generic_prove_ref as gr  # noqa: E402
import keccak_ref as kr  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401
from oracle import fri_ref, pyref  # noqa: E402

P = pyref.P
KECCAK = gr.KeccakHasher()


def _slots(hashes, garbage=None):
    """the device layout of `hashes` (bytes of length 25 each); `garbage`: a numpy Generator that fills bytes 25..31 of every slot"""
    s = kr.slots(np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 25))
    if garbage is not None:
        s[:, 3] |= garbage.integers(1, 1 << 56, size=s.shape[0], dtype=np.uint64) << np.uint64(8)
    return np.ascontiguousarray(s)


def _hashes(rng, count, kind):
    if kind == "ff":
        return [b"\xff" * 25] * count
    return [rng.integers(0, 256, size=25, dtype=np.uint8).tobytes() for _ in range(count)]


def _state_matches(ch, ref):
    T = ch.state.download()
    assert [int(v) for v in T[:12]] == ref.sponge_state
    assert int(T[28]) == len(ref.input_buffer) and int(T[29]) == len(ref.output_buffer)
    assert [int(v) for v in T[12 : 12 + len(ref.input_buffer)]] == ref.input_buffer


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "ff"])
@pytest.mark.parametrize("buffered", [0, 3, 7])
@pytest.mark.parametrize("n_digests", [1, 2, 3, 5])
def test_digests_are_observed_as_to_vec(gpu, n_digests, buffered, kind):
    """1, 2, 3 and 5 digests (two fill exactly one rate-8 block, three and five leave a remainder) after 0, 3 and 7 buffered plain
    elements, so that the chunks of a digest land on both sides of a duplexing; bytes 25..31 of every slot hold garbage, which
    must not reach the transcript: the result is that of clean slots and of the reference, which never sees a slot."""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd.challenger import DeviceChallenger

    rng = np.random.default_rng(1000 * n_digests + 10 * buffered + (kind == "ff"))
    hashes = _hashes(rng, n_digests, kind)
    plain = [int(v) for v in rng.integers(0, P, size=buffered, dtype=np.uint64)]
    ref = fri_ref.Challenger()
    ref.observe_elements(plain)
    for h in hashes:
        gr.observe_hash(KECCAK, ref, h)
    exp = ref.get_n_challenges(5)
    d_plain = pg.DeviceBuffer.from_host(gpu, np.array(plain or [0], dtype=np.uint64))
    results = []
    for garbage in (rng, None):
        d_slots = pg.DeviceBuffer.from_host(gpu, _slots(hashes, garbage))
        ch = DeviceChallenger(gpu)
        if buffered:  # in a step of their own: they wait in the input buffer
            assert ch.step([(d_plain, buffered)]) == []
        got = ch.step([DeviceChallenger.keccak_digests(d_slots, n_digests)], 5)
        assert got == exp
        _state_matches(ch, ref)
        results.append(ch.state.download().tolist())
    assert results[0] == results[1]


@pytest.mark.gpu
def test_digests_mixed_with_plain_and_planar_sources_in_one_call(gpu):
    """one launch over a plain source, two digests, a planar extension vector, three digests out of the middle of a buffer and a
    plain tail, then a second step on the same transcript: the circuit digest, the public-inputs hash and a cap, as prove() starts"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd.challenger import DeviceChallenger

    rng = np.random.default_rng(5)
    hashes = _hashes(rng, 6, "random")
    hashes[4] = b"\xff" * 25
    head = [int(v) for v in rng.integers(0, 1 << 64, size=5, dtype=np.uint64)]  # any representative: observed mod p
    planes = [int(v) for v in rng.integers(0, P, size=6, dtype=np.uint64)]
    tail = [int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)]
    d_slots = pg.DeviceBuffer.from_host(gpu, _slots(hashes, rng))
    bufs = [pg.DeviceBuffer.from_host(gpu, np.array(v, dtype=np.uint64)) for v in (head, planes, tail)]
    ch = DeviceChallenger(gpu)
    got = ch.step([(bufs[0], 5), DeviceChallenger.keccak_digests(d_slots, 2), (bufs[1], 6, 3), DeviceChallenger.keccak_digests(d_slots, 3, first=3),
                   (bufs[2], 2)], 4)
    ref = fri_ref.Challenger()
    ref.observe_elements(head)
    gr.observe_cap(KECCAK, ref, hashes[0:2])
    ref.observe_extension_elements([(planes[i], planes[3 + i]) for i in range(3)])
    gr.observe_cap(KECCAK, ref, hashes[3:6])
    ref.observe_elements(tail)
    assert got == ref.get_n_challenges(4)
    _state_matches(ch, ref)
    pih = [int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64)]
    d_pih = pg.DeviceBuffer.from_host(gpu, np.array(pih, dtype=np.uint64))
    got = ch.step([DeviceChallenger.keccak_digests(d_slots, 1, first=2), (d_pih, 4), DeviceChallenger.keccak_digests(d_slots, 4, first=1)], 6)
    gr.observe_hash(KECCAK, ref, hashes[2])
    ref.observe_elements(pih)
    gr.observe_cap(KECCAK, ref, hashes[1:5])
    assert got == ref.get_n_challenges(6)
    _state_matches(ch, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n_digests", [1, 2, 3, 5])
def test_hash_no_pad_over_a_digest_source(gpu, n_digests):
    """GL_CHALLENGER_HASH: hash_n_to_hash_no_pad of the to_vec elements (what the circuit digest's parts are made of)"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd.challenger import DeviceChallenger

    rng = np.random.default_rng(40 + n_digests)
    hashes = _hashes(rng, n_digests, "random")
    d_slots = pg.DeviceBuffer.from_host(gpu, _slots(hashes, rng))
    d_one = pg.DeviceBuffer.from_host(gpu, np.array([7], dtype=np.uint64))
    ch = DeviceChallenger(gpu)
    elems = [x for h in hashes for x in KECCAK.to_vec(h)]
    assert ch.step([DeviceChallenger.keccak_digests(d_slots, n_digests)], hash_out=True, reset=True) == pyref.hash_no_pad(elems)
    assert ch.step([DeviceChallenger.keccak_digests(d_slots, n_digests), (d_one, 1)], hash_out=True, reset=True) == pyref.hash_no_pad(elems + [7])


@pytest.mark.gpu
def test_a_count_that_is_no_multiple_of_four_is_refused(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    d_slots = pg.DeviceBuffer.from_host(gpu, _slots([b"\x01" * 25, b"\x02" * 25]))
    d_ch = pg.DeviceBuffer.from_host(gpu, np.arange(32, dtype=np.uint64))
    d_out = pg.DeviceBuffer(gpu, 4)
    for count in (1, 2, 3, 5, 7):
        src = (_lib.GlObserveSrc * 1)(_lib.GlObserveSrc(d_slots.ptr, count, _lib.GL_OBSERVE_KECCAK_DIGESTS))
        with pytest.raises(pg.Plonky2HipError, match="multiple of 4") as e:
            _lib.call("gl_challenger_step", d_ch.ptr, ctypes.addressof(src), 1, 2, d_out.ptr, 0, gpu.ptr)
        assert e.value.code == _lib.GL_E_INVALID
    assert d_ch.download().tolist() == list(range(32))  # no launch: the transcript is untouched
    # counts 0, 4 and 8 are fine, and the library goes on working
    for count in (0, 4, 8):
        src = (_lib.GlObserveSrc * 1)(_lib.GlObserveSrc(d_slots.ptr, count, _lib.GL_OBSERVE_KECCAK_DIGESTS))
        _lib.call("gl_challenger_step", d_ch.ptr, ctypes.addressof(src), 1, 2, d_out.ptr, 1, gpu.ptr)
    ref = fri_ref.Challenger()
    gr.observe_cap(KECCAK, ref, [b"\x01" * 25, b"\x02" * 25])
    assert [int(v) for v in d_out.download()[:2]] == ref.get_n_challenges(2)
