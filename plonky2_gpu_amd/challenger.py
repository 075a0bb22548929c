"""Host-side mirror of plonky2/src/iop/challenger.rs (Fiat-Shamir transcript). The sponge
permutation runs on the device (gl_poseidon_permute_batch on a 12-element buffer); the serial
glue — buffers, overwrite-mode duplexing — is host logic exactly like the reference's."""
import numpy as np

from . import _lib

SPONGE_RATE, SPONGE_WIDTH = 8, 12
P = 0xFFFFFFFF00000001


class Challenger:
    def __init__(self, ctx):
        self.ctx = ctx
        self.sponge_state = [0] * SPONGE_WIDTH
        self.input_buffer = []
        self.output_buffer = []

    def _absorb(self, state, blocks):
        """state after absorbing len(blocks)/8 full rate blocks (overwrite mode), one device call"""
        st = np.array(state, dtype=np.uint64)
        inp = np.array(blocks, dtype=np.uint64)
        _lib.call("gl_sponge_absorb", st, inp, inp.size // SPONGE_RATE, self.ctx.ptr)
        return [int(v) for v in st]

    def _permute(self, state):
        return self._absorb(state, state[:SPONGE_RATE])

    def observe_element(self, e):  # challenger.rs:43-53
        self.observe_elements([e])

    def observe_elements(self, es):
        """observe_element for each e (challenger.rs:43-59). Every time the input buffer fills the
        reference duplexes; the outputs of all but the last of those duplexings are discarded by the
        next observe, so all full blocks are absorbed by a single device call."""
        es = [int(e) % P for e in es]
        if not es:
            return
        buf = self.input_buffer + es
        full = len(buf) // SPONGE_RATE * SPONGE_RATE
        self.output_buffer = []
        if full:
            self.sponge_state = self._absorb(self.sponge_state, buf[:full])
            if full == len(buf):  # the last observe triggered the duplexing: its output is live
                self.output_buffer = list(self.sponge_state[:SPONGE_RATE])
        self.input_buffer = buf[full:]

    def observe_extension_elements(self, es):
        self.observe_elements([x for e in es for x in e])

    def observe_hash(self, h):
        self.observe_elements(h)

    def observe_cap(self, cap):  # challenger.rs:81-85
        self.observe_elements([x for h in cap for x in h])

    def get_challenge(self):  # challenger.rs:87-97
        if self.input_buffer or not self.output_buffer:
            self.duplexing()
        return self.output_buffer.pop()

    def get_n_challenges(self, n):
        return [self.get_challenge() for _ in range(n)]

    def get_extension_challenge(self):
        a, b = self.get_n_challenges(2)
        return (a, b)

    def compact(self):  # challenger.rs:149-155
        if self.input_buffer:
            self.duplexing()
        self.output_buffer = []
        return list(self.sponge_state)

    def duplexing(self):  # challenger.rs:131-149
        for i, x in enumerate(self.input_buffer):
            self.sponge_state[i] = x
        self.input_buffer = []
        self.sponge_state = self._permute(self.sponge_state)
        self.output_buffer = list(self.sponge_state[:SPONGE_RATE])


class DeviceChallenger:
    """The transcript in device memory (gl_challenger_step): 32 words the object owns; one `step` = one launch that observes up to
    eight device sources in order and then draws challenges. A source is (DeviceBuffer or address, count) for plain field
    elements, (.., count, planar_len) for an extension vector kept as two planes, or `keccak_digests(buf, n)` for n Keccak digest
    slots, observed as Challenger::observe_hash::<KeccakHash<25>> / observe_cap do: four elements per digest, its 25 bytes in
    chunks of 7, 7, 7 and 4 (hash/hash_types.rs:179-189)."""

    RESET, HASH, COMPACT = 1, 2, 4

    def __init__(self, ctx):
        from .device import DeviceBuffer

        self.ctx = ctx
        # all 32 words defined from the start: the kernel writes the sponge state, the input buffer and the two lengths (words 0..19,
        # 28, 29) and never touches the rest, which would otherwise be whatever the allocation held
        self.state = DeviceBuffer.from_host(ctx, np.zeros(32, dtype=np.uint64))
        self._out = DeviceBuffer(ctx, 64)
        self._fresh = True

    @staticmethod
    def keccak_digests(buf, n_digests, first=0):
        """the source of `n_digests` digest slots starting at slot `first` of `buf`"""
        ptr = buf if isinstance(buf, int) else buf.ptr
        return (ptr + 32 * first, 4 * n_digests, _lib.GL_OBSERVE_KECCAK_DIGESTS)

    def step(self, srcs=(), n_challenges=0, hash_out=False, reset=False, compact=False):
        """observe `srcs`, then get_n_challenges(n_challenges) -> list of ints; hash_out: the 4 words of hash_n_to_hash_no_pad of
        everything observed since the reset instead (use with reset=True); compact: Challenger::compact() before observing"""
        import ctypes

        if n_challenges > 64:
            raise ValueError("at most 64 challenges per step")
        arr = (_lib.GlObserveSrc * max(1, len(srcs)))()
        for i, s in enumerate(srcs):
            p, count, planar = (tuple(s) + (0,))[:3]
            arr[i] = _lib.GlObserveSrc(p if isinstance(p, int) else p.ptr, count, planar)
        flags = (self.RESET if reset or self._fresh else 0) | (self.HASH if hash_out else 0) | (self.COMPACT if compact else 0)
        words = 4 if hash_out else n_challenges
        _lib.call("gl_challenger_step", self.state.ptr, ctypes.addressof(arr), len(srcs), n_challenges, self._out.ptr if words else None,
                  flags, self.ctx.ptr)
        self._fresh = False
        return [int(v) for v in self._out.download(0, words)] if words else []


def hash_no_pad(ctx, inputs):
    """hash_n_to_hash_no_pad (plonky2/src/hash/hashing.rs:81-108) of a short host vector (public
    inputs, circuit digest parts); the permutation runs on the device."""
    c = Challenger(ctx)
    state = [0] * SPONGE_WIDTH
    inputs = [int(x) % P for x in inputs]
    full = len(inputs) // SPONGE_RATE * SPONGE_RATE
    if full:
        state = c._absorb(state, inputs[:full])
    if full < len(inputs):  # a short last chunk leaves the old lanes in place
        state[: len(inputs) - full] = inputs[full:]
        state = c._permute(state)
    return state[:4]
