"""Matrices whose columns lie more than 2^32 words apart (tests/test_gpu_far_pitch.py): the counterpart of tests/strided.py for
pitches at which a product `column * stride` formed in 32 bits goes wrong.

A pitch is only an address step: a matrix of a few kilobytes at a pitch of 2^32 / (cols - 1) words has its last column beyond
2^32 words, its kernel does a few kilobytes of work and the references answer in milliseconds. One allocation per test module

    [ FRONT = 2^31 words | base ... REACH = 2^32 + 2^24 words ]

holds every such matrix: column c of a matrix in slot k starts at base + k * 2^16 + c * stride and is surrounded by guard words

    [guard 64 | column c | guard 64]

Everything else in the allocation is left as the allocator gave it. The base sits 2^31 words into the allocation, so a column
offset cut to 32 bits (of words or of bytes, zero- or sign-extended) still lands inside it: a defect shows as a wrong value or a
changed guard word, never as a fault. check_layout() is the assertion that a layout can tell a cut offset from a whole one; every
Far checks its layout when it is made, and the CPU test of tests/test_gpu_far_pitch.py checks every layout the module declares.

The tail is 2^24 words (not 2^20): the last column of three 2^22-point polynomials and of their 2^23-point LDE starts behind
2^32 words and has to end inside the allocation."""
import ctypes

import numpy as np

from strided import filler

FRONT = 1 << 31                  # words in front of the base
REACH = (1 << 32) + (1 << 24)    # words from the base on
WORDS = FRONT + REACH            # 48 GiB + 128 MiB
GUARD = 64
SLOT = 1 << 16
THRESHOLDS = (1 << 29, 1 << 31, 1 << 32)   # the byte offset reaches 2^32; a signed word offset breaks; the word offset reaches 2^32
MIN_DEVICE_BYTES = 96 << 30


def far_pitch(cols, multiple_of=1):
    """the smallest even pitch S (the smallest even multiple of `multiple_of`) with (cols - 1) * S >= 2^32 + 2: the last column
    starts behind 2^32 words, and cut to 32 bits its offset is not column 0's"""
    assert cols >= 2
    step = multiple_of if multiple_of % 2 == 0 else 2 * multiple_of
    per = -(-((1 << 32) + 2) // (cols - 1))
    return -(-per // step) * step


def _sign(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


# what a kernel computes in place of the word offset c * stride when it forms it, or the byte offset, in 32 bits
TRUNCATIONS = {
    "u32 words": lambda w: w & 0xFFFFFFFF,
    "i32 words": lambda w: _sign(w, 32),
    "u32 bytes": lambda w: ((8 * w) & 0xFFFFFFFF) // 8,
    "i32 bytes": lambda w: _sign(8 * w, 32) // 8,
}


class Layout:
    """`cols` columns of `width` words at far_pitch(cols, multiple_of), column 0 at base + slot * 2^16. `pitch_of`: the number of
    columns of the widest matrix of a call that takes several matrices at ONE pitch; the narrower ones follow its pitch."""

    def __init__(self, cols, width, slot=0, multiple_of=1, pitch_of=None):
        self.cols, self.width, self.slot = int(cols), int(width), int(slot)
        self.pitch_of = self.cols if pitch_of is None else int(pitch_of)
        assert self.pitch_of >= self.cols
        self.stride = far_pitch(self.pitch_of, multiple_of)
        self.offset = self.slot * SLOT

    def start(self, c):
        """of column c, in words from the base"""
        return self.offset + c * self.stride

    def key(self):
        return (self.cols, self.width, self.slot, self.stride)

    def __repr__(self):
        return "Layout(cols=%d, width=%d, slot=%d, stride=%d)" % self.key()


def check_layout(lay):
    """every column with its guards lies inside the allocation, and so does what each truncation makes of the column; for each
    truncation some column's cut window is disjoint from its true one; some column starts at or behind each threshold. A matrix
    that follows a wider one's pitch (pitch_of) only has to stay inside: the wider one is what tells."""
    span = lay.width + 2 * GUARD
    assert lay.stride % 2 == 0 and lay.stride >= span, lay
    for c in range(lay.cols):
        assert -FRONT <= lay.start(c) - GUARD and lay.start(c) + lay.width + GUARD <= REACH, (lay, "column outside the allocation", c)
    for name, cut in TRUNCATIONS.items():
        for c in range(lay.cols):
            got = lay.offset + cut(c * lay.stride)
            assert -FRONT <= got and got + lay.width <= REACH, (lay, name, "leaves the allocation at column", c)
    if lay.pitch_of != lay.cols:
        return lay
    assert (lay.cols - 1) * lay.stride >= (1 << 32) + 2, lay
    for t in THRESHOLDS:
        assert any(c * lay.stride >= t for c in range(lay.cols)), (lay, "no column at or behind", t)
    for name, cut in TRUNCATIONS.items():
        told = sum(abs(cut(c * lay.stride) - c * lay.stride) >= span for c in range(lay.cols))
        assert told, (lay, name, "no column whose cut window is disjoint from its true one")
    return lay


DECLARED = {}
_frozen = False


def declare(cols, width, slot=0, multiple_of=1, pitch_of=None):
    """the layout of a matrix of the test module: declared while the module is imported (so that the CPU test sees every one),
    looked up by the tests afterwards"""
    lay = Layout(cols, width, slot, multiple_of, pitch_of)
    if lay.key() not in DECLARED:
        assert not _frozen, ("a layout the module did not declare", lay)
        DECLARED[lay.key()] = lay
    return DECLARED[lay.key()]


def freeze():
    global _frozen
    _frozen = True


def disjoint(layouts):
    """the windows of matrices that share the allocation in one call do not touch"""
    spans = []
    for lay in layouts:
        starts = lay.offset + lay.stride * np.arange(lay.cols, dtype=np.int64) - GUARD
        spans += [(int(s), int(s) + lay.width + 2 * GUARD) for s in starts]
    spans.sort()
    return all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def device_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return total.value


class FarAllocation:
    """the one allocation of a test module; .live: the layouts of the matrices in it"""

    def __init__(self, ctx):
        import plonky2_gpu_amd as pg

        self.ctx = ctx
        self.buf = pg.DeviceBuffer(ctx, WORDS)   # a refusal on a device of 96 GiB and more is a failure
        self.live = []

    def at(self, words_from_base):
        return self.buf.at(FRONT + words_from_base)

    def free(self):
        self.buf.free()


class Far:
    """A matrix [cols][width] in the far allocation. .ptr is the address of column 0, .stride the pitch; .read() downloads the
    columns and checks every guard word; .unchanged() is .read() compared with what was uploaded. free() gives the windows back."""

    def __init__(self, alloc, layout, data):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        assert data.shape == (layout.cols, layout.width), (data.shape, layout)
        assert DECLARED.get(layout.key()) is layout, ("a layout the module did not declare", layout)
        check_layout(layout)
        assert disjoint(alloc.live + [layout]), ("windows of two matrices overlap", alloc.live, layout)
        alloc.live.append(layout)
        self.alloc, self.layout, self.data = alloc, layout, data
        self.cols, self.width, self.stride = layout.cols, layout.width, layout.stride
        self.ptr = alloc.at(layout.offset)
        assert self.ptr % 16 == 0
        image = np.empty(self.width + 2 * GUARD, dtype=np.uint64)
        for c in range(self.cols):
            image[:GUARD], image[-GUARD:] = self._guards(c)
            image[GUARD:-GUARD] = data[c]
            alloc.buf.upload(image, FRONT + layout.start(c) - GUARD)

    @classmethod
    def filled(cls, alloc, layout, start=0):
        """an output: every word the filler, which is no canonical field element"""
        return cls(alloc, layout, np.broadcast_to(filler(layout.width, start), (layout.cols, layout.width)))

    def _guards(self, c):
        return filler(GUARD, 131 * c), filler(GUARD, 131 * c + 77)

    def read(self, what=""):
        out = np.empty((self.cols, self.width), dtype=np.uint64)
        for c in range(self.cols):
            got = self.alloc.buf.download(FRONT + self.layout.start(c) - GUARD, self.width + 2 * GUARD)
            front, back = self._guards(c)
            assert (got[:GUARD] == front).all(), ("the guard in front of a column was written", c, what)
            assert (got[-GUARD:] == back).all(), ("the guard behind a column was written", c, what)
            out[c] = got[GUARD:-GUARD]
        return out

    def unchanged(self, what=""):
        bad = np.argwhere(self.read(what) != self.data)
        assert bad.size == 0, ("a read-only input was written, first (column, word)", bad[0].tolist(), len(bad), what)

    def free(self):
        self.alloc.live.remove(self.layout)
