"""Strided device buffers for the stride tests (tests/test_gpu_strides.py, tests/ntt_variant_child.py): polynomials laid out as

    [guard | poly 0 | pad | poly 1 | pad | ... | poly k-1 | pad | guard]

with every guard and pad word a recognisable word that is no canonical field element. A kernel that rounds a tile up and stores
past a column, or past the batch, changes one of them."""
import numpy as np

P = 0xFFFFFFFF00000001
GUARD = 66   # words: the first polynomial starts 16-byte aligned (528 bytes into the allocation) but not 64-byte aligned
TAIL = 64


def filler(count, start=0):
    """0xFFFFFFFFDEADxxxx with xxxx = the word's position mod 2^16: every word >= p, and a block moved elsewhere does not fit"""
    return np.uint64(0xFFFFFFFFDEAD0000) + ((np.arange(count, dtype=np.uint64) + np.uint64(start)) & np.uint64(0xFFFF))


class Strided:
    """k polynomials of `width` words at distance `stride` in one device buffer, guards and pads as above.
    .ptr is the address of polynomial 0, .polys() downloads, checks every guard and pad word and returns the polynomials."""

    def __init__(self, ctx, polys, stride):
        import plonky2_gpu_amd as pg

        polys = np.asarray(polys, dtype=np.uint64)
        self.k, self.width = polys.shape
        self.stride = int(stride)
        assert self.stride >= self.width
        self.total = GUARD + self.k * self.stride + TAIL
        host = filler(self.total)
        host[GUARD : GUARD + self.k * self.stride].reshape(self.k, self.stride)[:, : self.width] = polys
        self.buf = pg.DeviceBuffer.from_host(ctx, host)
        self.ptr = self.buf.at(GUARD)
        assert self.ptr % 16 == 0 and self.ptr % 64 != 0

    def polys(self, what=""):
        out = self.buf.download()
        fill = filler(self.total)
        assert (out[:GUARD] == fill[:GUARD]).all(), ("the guard in front of the batch was written", what)
        assert (out[-TAIL:] == fill[-TAIL:]).all(), ("the guard behind the batch was written", what)
        body = out[GUARD:-TAIL].reshape(self.k, self.stride)
        if self.stride > self.width:
            pads = fill[GUARD:-TAIL].reshape(self.k, self.stride)[:, self.width :]
            bad = np.argwhere(body[:, self.width :] != pads)
            assert bad.size == 0, ("pad words behind a polynomial were written, first (polynomial, word)", bad[0].tolist(), len(bad), what)
        return body[:, : self.width]

    def free(self):
        self.buf.free()


def bitrev_perm(bits):
    idx = np.arange(1 << bits, dtype=np.uint64)
    out = np.zeros_like(idx)
    for b in range(bits):
        out |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
    return out.astype(np.int64)


def lift_some(x, column, seed):
    """give half of the liftable words (x < 2^32 - 1) of one column their second representative x + p; so that there are some,
    a quarter of that column is made small first. Returns the number lifted."""
    rng = np.random.default_rng(seed)
    col = x[column]
    small = rng.random(col.size) < 0.25
    col[small] = rng.integers(0, (1 << 32) - 1, size=int(small.sum()), dtype=np.uint64)
    pick = small & (rng.random(col.size) < 0.5)
    col[pick] += np.uint64(P)
    if col.size > 1:
        col[-1] = np.uint64(2**64 - 1)
    return int(pick.sum())


# gl_ntt_batch: (log_n, number of polynomials). At the one-pass sizes (log_n <= 12) a tile holds 2^(13 - log_n) polynomials and the
# count leaves the last tile ragged; three polynomials at the multi-pass sizes.
NTT_SHAPES = [(1, 4099), (5, 259), (12, 5), (13, 3), (16, 3), (18, 3), (19, 3), (20, 3), (21, 3), (22, 3), (23, 3), (24, 3)]


def ntt_strides(log_n, order):
    """the padded strides: forward and bit-reversed n + 2 (the smallest legal pad: no alignment above 16 bytes survives), n + 48
    (a pitch that is no power of two) and 2n; inverse (stride % n == 0) 2n and 3n (offset bits above log_n that are not a single
    bit). Every size takes all of them, 2^24 included."""
    n = 1 << log_n
    return [2 * n, 3 * n] if order == "inverse" else [n + 2, n + 48, 2 * n]


def ntt_case(oracle, log_n, n_polys, threads=4):
    """(input with non-canonical words in column 1, forward transform, inverse transform, bit reversal permutation): the
    oracle's answers for one size, computed once and used for every stride and order"""
    n = 1 << log_n
    x = oracle.random_field((n_polys, n), seed=8800 + log_n)
    x[0, :] = np.uint64(P - 1)
    lift_some(x, 1, 8900 + log_n)
    xc = oracle.canon(x)  # the oracle gets the canonical representatives of the same field elements
    return x, oracle.canon(oracle.fft_batch(xc, threads=threads)), oracle.canon(oracle.fft_batch(xc, inverse=True, threads=threads)), bitrev_perm(log_n)


def run_ntt(ctx, x, stride, order):
    """gl_ntt_batch on a guarded, padded copy of x; the transformed polynomials (guards and pads checked)"""
    from plonky2_gpu_amd import _lib

    s = Strided(ctx, x, stride)
    _lib.call("gl_ntt_batch", s.ptr, x.shape[0], x.shape[1].bit_length() - 1, stride, int(order == "inverse"), int(order == "bit_reversed"), ctx.ptr)
    out = s.polys((order, stride))
    s.free()
    return out


def check_ntt(ctx, case, order, strides):
    x, exp_f, exp_i, perm = case
    exp = {"forward": exp_f, "inverse": exp_i}[order] if order != "bit_reversed" else exp_f[:, perm]
    for stride in strides:
        got = run_ntt(ctx, x, stride, order)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, (order, "stride", stride, "polynomials that differ from the oracle", bad[:8].tolist())
