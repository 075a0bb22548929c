"""Transforms, column hashing, openings and the quotient at PADDED column strides, in every pass plan of the planner
(csrc/ntt.hip ntt_batch / coset_lde_batch), and the stride and alignment rules of include/plonky2_hip.h.

Every comparison is equality with the C oracle (oracle/oracle.py) or with Python integers; the buffers are guarded and padded
(tests/strided.py): a store past a column or past the batch fails the case that made it.

Planner branch (product build)                                                    -> test id
  ntt_batch   one pass, log_n <= 12, ragged last tile                              test_ntt_padded_strides[1|5|12-*]
              two passes, natural order through the workspace (13, 16, 20)         test_ntt_padded_strides[13|16|20-forward|inverse]
              two passes, bit-reversed in place (13 .. 21)                         test_ntt_padded_strides[13..21-bit_reversed]
              2^18 = 256 x 1024 and 2^19 = 512 x 1024 (direct kernels both passes) test_ntt_padded_strides[18|19-*]
              2^21 = 2048 x 1024, split 2048-point columns                         test_ntt_padded_strides[21-*]
              2^22 natural forward, transposed through the workspace               test_ntt_padded_strides[22-forward]
              2^22 inverse on the index-reversed input                             test_ntt_padded_strides[22-inverse]
              2^22 bit-reversed, two waves per 2048-point row                      test_ntt_padded_strides[22-bit_reversed]
              three passes (2^23, 2^24), every order                               test_ntt_padded_strides[23|24-*]
              workspace chunk boundary crossed, each of the three chunk loops      test_ntt_batch_crossing_a_workspace_chunk[13 .. 24]
              the 65535-polynomial step (grid.y) crossed, in place                 test_ntt_and_lde_batches_of_more_than_65535_polynomials
  coset_lde   log_n <= 12, one batched transform (dst_stride == n_ext)             test_coset_lde_padded_strides[3-3|12-3] (dst n_ext)
              log_n <= 12, one transform per polynomial (padded dst_stride)        test_coset_lde_padded_strides[3-3|12-3] (dst padded)
              two passes (13 .. 21; 18 / 19 with 1024-point rows; 21 split)        test_coset_lde_padded_strides[13-3 .. 21-1]
              three passes (22, 23), contiguous and one call per polynomial        test_coset_lde_padded_strides[22-1|23-0]
              the 65535-polynomial step crossed                                    test_ntt_and_lde_batches_of_more_than_65535_polynomials
  the diagnostic build's kernel selections at a padded stride                      test_gpu_ntt.py::test_alternative_kernel_selections
  every entry point that takes a pitch, the last column behind 2^32 words           test_gpu_far_pitch.py (layout: tests/far.py)

NOT reachable: the 65535-polynomial step of the plans from 2^22 up (bit-reversed in place; the three-pass LDE): 65536 polynomials
of 2^22 points are 2.2 TB. The step is crossed at 2^13 only. log_n = 0 moves single words and has no plan. The bit-reversed
inverse is refused by the API. Every size, 2^24 included, runs the whole stride list (tests/strided.py ntt_strides)."""
import ctypes

import numpy as np
import pytest

import strided
from gpu_util import P, gpu  # noqa: F401
from strided import Strided, bitrev_perm, filler

pytestmark = pytest.mark.gpu


def _L():
    from plonky2_gpu_amd import _lib

    return _lib


def _pg():
    import plonky2_gpu_amd as pg

    return pg


def _dev(gpu, a):
    return _pg().DeviceBuffer.from_host(gpu, np.ascontiguousarray(a, dtype=np.uint64).reshape(-1))


def _zeros(gpu, n):
    b = _pg().DeviceBuffer(gpu, max(int(n), 1))
    _L().call("gl_memset_zero", b.ptr, 8 * max(int(n), 1), gpu.ptr)
    return b


def _invalid(name, *args):
    with pytest.raises(_pg().Plonky2HipError) as e:
        _L().call(name, *args)
    assert e.value.code == _pg().GL_E_INVALID, (name, e.value)


# ---- 1. gl_ntt_batch: every plan x every order x padded strides ----------------------------------------------------------------

_ntt_case = {}


def _case(oracle, log_n, n_polys):
    """the oracle's answers, once per size (the parametrisation runs a size's three orders one after the other)"""
    if log_n not in _ntt_case:
        _ntt_case.clear()
        _ntt_case[log_n] = strided.ntt_case(oracle, log_n, n_polys)
    return _ntt_case[log_n]


@pytest.mark.parametrize("order", ["forward", "bit_reversed", "inverse"])
@pytest.mark.parametrize("log_n,n_polys", strided.NTT_SHAPES, ids=[str(s[0]) for s in strided.NTT_SHAPES])
def test_ntt_padded_strides(gpu, oracle, log_n, n_polys, order):
    """gl_ntt_batch in place on [guard | poly | pad | ... | guard] at strides n + 2, n + 48, 2n (inverse: 2n, 3n): every polynomial
    equals the oracle's transform, no guard or pad word changes. Column 0 is all p - 1, column 1 carries non-canonical words."""
    case = _case(oracle, log_n, n_polys)
    strided.check_ntt(gpu, case, order, strided.ntt_strides(log_n, order))
    if order == "inverse" and log_n >= 23:
        _ntt_case.clear()


# ---- 2. gl_ntt_batch: the batch splits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n", [13, 16, 20, 21, 22, 23, 24])
def test_ntt_batch_crossing_a_workspace_chunk(gpu, oracle, log_n):
    """The natural-order plans take gl_workspace_bytes() / 8 >> log_n polynomials at a time through the workspace: chunk + 3
    polynomials cross into a second chunk. Forward at strides n and n + 2, inverse at n and 2n; polynomials 0, chunk - 1, chunk,
    chunk + 2 against the oracle, all of them through ifft(fft(x)) == canon(x). 13, 16, 20: the generic two-pass plan (2^20 forward
    with 67 columns is the benchmark's shape); 2^21 = 2048 x 1024 on split columns goes through the same loop; 2^22 (the transposed
    two-pass plan and its inverse on the index-reversed input) and 2^23, 2^24 (three passes) have chunk loops of their own."""
    L = _L()
    n = 1 << log_n
    chunk = (L.load().gl_workspace_bytes() // 8) >> log_n
    assert chunk >= 1
    k = chunk + 3
    x = oracle.random_field((k, n), seed=9300 + log_n)
    strided.lift_some(x, chunk, 9400 + log_n)
    watch = [0, chunk - 1, chunk, chunk + 2]
    xc = oracle.canon(x)
    exp_f = oracle.canon(oracle.fft_batch(xc[watch].copy(), threads=4))

    # stride n: forward, then the inverse of that in the same buffer
    s = Strided(gpu, x, n)
    L.call("gl_ntt_batch", s.ptr, k, log_n, n, 0, 0, gpu.ptr)
    f = s.polys("forward, stride n").copy()
    assert (f[watch] == exp_f).all(), np.flatnonzero((f[watch] != exp_f).any(axis=1))
    L.call("gl_ntt_batch", s.ptr, k, log_n, n, 1, 0, gpu.ptr)
    back = s.polys("inverse, stride n")
    bad = np.flatnonzero((back != xc).any(axis=1))
    assert bad.size == 0, ("ifft(fft(x)) != x at stride n, polynomials", bad[:8].tolist())
    s.free()
    exp_i = oracle.canon(oracle.fft_batch(f[watch].copy(), inverse=True, threads=4))
    assert (exp_i == xc[watch]).all()  # the oracle's inverse of the watched transforms: what the round trip was compared with

    # forward at n + 2: the watched ones against the oracle, all of them against the (round-trip verified) transform above
    got = strided.run_ntt(gpu, x, n + 2, "forward")
    assert (got[watch] == exp_f).all(), np.flatnonzero((got[watch] != exp_f).any(axis=1))
    bad = np.flatnonzero((got != f).any(axis=1))
    assert bad.size == 0, ("forward at stride n + 2, polynomials", bad[:8].tolist())
    del got
    if log_n == 22:  # the bit-reversed 2^22 plan (two waves per row) reads its rows from the workspace: the same chunks
        perm = bitrev_perm(log_n)
        got = strided.run_ntt(gpu, x, n + 2, "bit_reversed")
        assert (got[watch] == exp_f[:, perm]).all(), np.flatnonzero((got[watch] != exp_f[:, perm]).any(axis=1))
        bad = np.flatnonzero((got != f[:, perm]).any(axis=1))
        assert bad.size == 0, ("bit-reversed at stride n + 2, polynomials", bad[:8].tolist())
        del got

    # inverse at 2n of the transforms
    back = strided.run_ntt(gpu, f, 2 * n, "inverse")
    bad = np.flatnonzero((back != xc).any(axis=1))
    assert bad.size == 0, ("ifft(fft(x)) != x at stride 2n, polynomials", bad[:8].tolist())


def _replicate(gpu, buf, block_words, n_words):
    """fill buf[0 : n_words] with copies of its first block_words words, on the device"""
    done = block_words
    while done < n_words:
        step = min(done, n_words - done)
        _L().call("gl_memcpy_d2d", buf.at(done), buf.ptr, 8 * step, gpu.ptr)
        done += step


def _replicas_equal_the_first(gpu, buf, block_words, n_blocks, what):
    """every block of buf equals block 0: spans of `span` blocks are subtracted from the first span on the device (gl_debug_field_op
    1 = sub: zero exactly when the two canonical words are equal), and inside the first span block j from block 0 the same way"""
    L = _L()
    span = 256
    diff = _pg().DeviceBuffer(gpu, span * block_words)
    size = 1
    while size < min(span, n_blocks):  # blocks [size, 2 size) against [0, size)
        cnt = min(size, n_blocks - size)
        L.call("gl_debug_field_op", 1, buf.ptr, buf.at(size * block_words), diff.ptr, cnt * block_words, gpu.ptr)
        assert not diff.download(0, cnt * block_words).any(), (what, "blocks from", size)
        size *= 2
    for first in range(span, n_blocks, span):
        cnt = min(span, n_blocks - first)
        L.call("gl_debug_field_op", 1, buf.ptr, buf.at(first * block_words), diff.ptr, cnt * block_words, gpu.ptr)
        assert not diff.download(0, cnt * block_words).any(), (what, "blocks from", first)
    diff.free()


def test_ntt_and_lde_batches_of_more_than_65535_polynomials(gpu, oracle):
    """The in-place plans and the coset LDE walk the batch in steps of 65535 polynomials (grid.y): 65535 + 4 polynomials of 2^13
    points (4.3 GB), copies of eight distinct columns made on the device. Bit-reversed in place, then the same count through
    gl_coset_lde_batch at rate_bits = 1 (8.6 GB out): polynomials 0, 65534, 65535 and 65538 against the oracle, every block of
    eight against the first one on the device, the words behind the batch untouched."""
    L, pg = _L(), _pg()
    log_n, distinct, k = 13, 8, 65535 + 4
    n = 1 << log_n
    watch = (0, 65534, 65535, 65538)
    x = oracle.random_field((distinct, n), seed=9500)
    strided.lift_some(x, 2, 9501)
    tail = filler(strided.TAIL)

    src = pg.DeviceBuffer(gpu, k * n + strided.TAIL)
    src.upload(x, 0)
    _replicate(gpu, src, distinct * n, k * n)
    src.upload(tail, k * n)
    for c in watch:
        assert (src.download(c * n, n) == x[c % distinct]).all(), c

    # the coset LDE first: it reads src, which the transform below overwrites
    n_ext = 2 * n
    out = pg.DeviceBuffer(gpu, k * n_ext + strided.TAIL)
    out.upload(tail, k * n_ext)
    L.call("gl_coset_lde_batch", src.ptr, out.ptr, k, log_n, 1, 7, n, n_ext, gpu.ptr)
    gpu.synchronize()
    exp = oracle.canon(oracle.coset_lde_batch(oracle.canon(x), 1, threads=4))[:, bitrev_perm(log_n + 1)]
    for c in watch:
        assert (out.download(c * n_ext, n_ext) == exp[c % distinct]).all(), ("lde", c)
    assert (out.download(k * n_ext, strided.TAIL) == tail).all(), "the coset LDE wrote behind its last polynomial"
    _replicas_equal_the_first(gpu, out, distinct * n_ext, k // distinct, "lde")
    for c in range(k - k % distinct, k):  # the last, partial block
        assert (out.download(c * n_ext, n_ext) == exp[c % distinct]).all(), ("lde", c)
    out.free()
    for c in watch:
        assert (src.download(c * n, n) == x[c % distinct]).all(), ("the coset LDE changed its source", c)

    L.call("gl_ntt_batch", src.ptr, k, log_n, n, 0, 1, gpu.ptr)
    gpu.synchronize()
    exp = oracle.canon(oracle.fft_batch(oracle.canon(x), threads=4))[:, bitrev_perm(log_n)]
    for c in list(watch) + list(range(k - k % distinct, k)):
        assert (src.download(c * n, n) == exp[c % distinct]).all(), ("ntt", c)
    assert (src.download(k * n, strided.TAIL) == tail).all(), "the transform wrote behind its last polynomial"
    _replicas_equal_the_first(gpu, src, distinct * n, k // distinct, "ntt")
    src.free()


# ---- 3. gl_coset_lde_batch: source and destination strides -------------------------------------------------------------------

@pytest.mark.parametrize("log_n,rate_bits", [(3, 3), (12, 3), (13, 3), (16, 3), (18, 1), (19, 1), (20, 3), (21, 1), (22, 1), (23, 0)])
def test_coset_lde_padded_strides(gpu, oracle, log_n, rate_bits):
    """src_stride in {n + 2, 2n} x dst_stride in {n_ext, n_ext + 2, n_ext + 48}: every polynomial equals the oracle's coset LDE in
    bit-reversed order, the destination's guards and pads and the whole source buffer are unchanged. At log_n >= 22 a padded
    dst_stride runs one call per polynomial (csrc/ntt.hip), as it does at log_n <= 12."""
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    k = 3 if log_n + rate_bits <= 21 else 2
    c = oracle.random_field((k, n), seed=9600 + 10 * log_n + rate_bits)
    strided.lift_some(c, 1, 9700 + log_n)
    exp = oracle.canon(oracle.coset_lde_batch(oracle.canon(c), rate_bits, threads=4))[:, bitrev_perm(log_n + rate_bits)]
    for src_stride in (n + 2, 2 * n):
        src = Strided(gpu, c, src_stride)
        for dst_stride in (n_ext, n_ext + 2, n_ext + 48):
            dst = Strided(gpu, np.broadcast_to(filler(n_ext, 7), (k, n_ext)), dst_stride)
            _L().call("gl_coset_lde_batch", src.ptr, dst.ptr, k, log_n, rate_bits, 7, src_stride, dst_stride, gpu.ptr)
            got = dst.polys(("lde", src_stride, dst_stride))
            bad = np.flatnonzero((got != exp).any(axis=1))
            assert bad.size == 0, ("src_stride", src_stride, "dst_stride", dst_stride, "polynomials", bad.tolist())
            dst.free()
        assert (src.polys("the source of the LDE") == c).all(), "the coset LDE changed its source"
        src.free()


# ---- 4. a commitment at a padded pitch, end to end ----------------------------------------------------------------------------

def _open_and_verify(gpu, oracle, d_cols, pitch, leaf_len, n_leaves, cap_height, d_dig, leaves, cap, seed):
    """gl_merkle_open_batch and gl_merkle_open_batch_device reading the columns in place, (row_stride, elem_stride) = (1, pitch)"""
    L = _L()
    rng = np.random.default_rng(seed)
    log_leaves = n_leaves.bit_length() - 1
    layers = log_leaves - cap_height
    canon = oracle.canon(leaves)  # the opened leaves are the caller's words; the paths are checked with the field elements
    idx = np.concatenate([np.array([0, n_leaves - 1, 1, n_leaves // 2], dtype=np.uint64), rng.integers(0, n_leaves, size=12, dtype=np.uint64)])
    h_l = np.zeros(idx.size * leaf_len, dtype=np.uint64)
    h_s = np.zeros(max(idx.size * layers * 4, 1), dtype=np.uint64)
    L.call("gl_merkle_open_batch", d_cols, 1, pitch, leaf_len, n_leaves, cap_height, d_dig.ptr, idx, idx.size, h_l, h_s, gpu.ptr)
    assert (h_l.reshape(idx.size, leaf_len) == leaves[idx.astype(np.int64)]).all()
    sib = h_s[: idx.size * layers * 4].reshape(idx.size, layers, 4)
    for q, i in enumerate(idx):
        assert oracle.merkle_verify(canon[int(i)], int(i), cap, sib[q]), ("host indices", int(i))
    # raw 64-bit challenges and an index shift: leaf = (raw mod (n_leaves << shift)) >> shift
    shift = 3
    raw = rng.integers(0, 2**64, size=16, dtype=np.uint64)
    raw[0] = 0                                        # leaf 0
    raw[1] = np.uint64((n_leaves << shift) - 1)        # the last leaf
    raw[2] = np.uint64(2**64 - 1)
    want = np.array([(int(r) % (n_leaves << shift)) >> shift for r in raw], dtype=np.int64)
    assert want[0] == 0 and want[1] == n_leaves - 1
    d_raw, d_ol, d_os = _dev(gpu, raw), _zeros(gpu, raw.size * leaf_len), _zeros(gpu, raw.size * layers * 4)
    L.call("gl_merkle_open_batch_device", d_cols, 1, pitch, leaf_len, n_leaves, cap_height, d_dig.ptr, d_raw.ptr, raw.size, shift,
           d_ol.ptr, d_os.ptr, gpu.ptr)
    gpu.synchronize()
    assert (d_ol.download().reshape(raw.size, leaf_len) == leaves[want]).all()
    sib = d_os.download()[: raw.size * layers * 4].reshape(raw.size, layers, 4)
    for q, i in enumerate(want):
        assert oracle.merkle_verify(canon[int(i)], int(i), cap, sib[q]), ("raw challenges", int(i))
    for b in (d_raw, d_ol, d_os):
        b.free()


@pytest.mark.parametrize("polys,log_n,rate_bits,cap_height", [(135, 10, 3, 4), (20, 16, 3, 4), (9, 20, 3, 4)])
def test_commitment_at_a_padded_pitch(gpu, oracle, polys, log_n, rate_bits, cap_height):
    """The LDE buffer with a column pitch of n_ext + 2 and n_ext + 48 through everything that reads it: gl_coset_lde_batch writes
    it, gl_merkle_tree_from_columns hashes it (digests and cap = oracle.commit_from_coeffs), gl_transpose copies it leaf-major
    (= the oracle's leaves), gl_merkle_open_batch{,_device} open it in place (paths verified by the oracle), gl_pack_leaf_ranges
    packs it for 2 and 4 ranks (the header's formula); afterwards the pads and guards of the buffer are as they were."""
    L = _L()
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    coeffs = oracle.random_field((polys, n), seed=9800 + log_n)
    strided.lift_some(coeffs, polys - 1, 9801 + log_n)
    exp = oracle.commit_from_coeffs(oracle.canon(coeffs), rate_bits, cap_height, threads=4)
    leaves, dig, cap = oracle.canon(exp["leaves"]), oracle.canon(exp["digests"]).reshape(-1), oracle.canon(exp["cap"])
    cols = np.ascontiguousarray(leaves.T)
    d_coeffs = _dev(gpu, coeffs)
    for pitch in (n_ext + 2, n_ext + 48):
        lde = Strided(gpu, np.broadcast_to(filler(n_ext, 3), (polys, n_ext)), pitch)
        L.call("gl_coset_lde_batch", d_coeffs.ptr, lde.ptr, polys, log_n, rate_bits, 7, n, pitch, gpu.ptr)
        assert (lde.polys(("lde", pitch)) == cols).all()
        d_dig, d_cap = _zeros(gpu, dig.size), _zeros(gpu, cap.size)
        L.call("gl_merkle_tree_from_columns", lde.ptr, polys, n_ext, pitch, cap_height, d_dig.ptr, d_cap.ptr, gpu.ptr)
        gpu.synchronize()
        assert (d_cap.download().reshape(-1, 4) == cap).all(), pitch
        assert (d_dig.download() == dig).all(), pitch
        d_rows = Strided(gpu, np.broadcast_to(filler(polys, 5), (n_ext, polys)), polys)
        L.call("gl_transpose", lde.ptr, d_rows.ptr, polys, n_ext, pitch, gpu.ptr)
        assert (d_rows.polys(("transpose", pitch)) == leaves).all(), pitch
        d_rows.free()
        _open_and_verify(gpu, oracle, lde.ptr, pitch, polys, n_ext, cap_height, d_dig, leaves, cap, 9900 + log_n)
        for world in (2, 4):
            per = n_ext // world
            packed = Strided(gpu, np.broadcast_to(filler(per, 9), (world * polys, per)), per)
            L.call("gl_pack_leaf_ranges", lde.ptr, pitch, polys, per, world, packed.ptr, gpu.ptr)
            got = packed.polys(("pack", pitch, world)).reshape(world, polys, per)
            for q in range(world):  # d_out[(q * n_cols + c) * per + i] = d_lde[c * col_stride + q * per + i]
                assert (got[q] == cols[:, q * per : (q + 1) * per]).all(), (pitch, world, q)
            packed.free()
        assert (lde.polys(("after the readers", pitch)) == cols).all()
        for b in (lde, d_dig, d_cap):
            b.free()
    d_coeffs.free()


@pytest.mark.parametrize("log_leaves", [0, 1, 8, 13])
@pytest.mark.parametrize("leaf_len", [3, 4, 7, 8, 9, 135])
def test_merkle_tree_from_columns_at_an_odd_column_stride(gpu, oracle, leaf_len, log_leaves):
    """col_stride = n_leaves + 1: columns that are 8-byte aligned only (nothing in the header forbids it). Leaves of 3 and 4 words
    are their own digests (hash_or_noop), 7 / 8 / 9 sit around one rate block, 135 is the wires' width; trees of 1, 2, 256 and 2^13
    leaves with cap height 0 and the largest one; transposed and opened at the same stride."""
    L = _L()
    n = 1 << log_leaves
    leaves = oracle.random_field((n, leaf_len), seed=10000 + 200 * log_leaves + leaf_len)
    strided.lift_some(leaves.reshape(1, -1), 0, 10001 + leaf_len)
    canon = oracle.canon(leaves)
    stride = n + 1
    cols = Strided(gpu, leaves.T, stride)
    for h in sorted({0, log_leaves}):
        dig, cap = oracle.merkle_tree(canon, h, threads=4)
        dig, cap = oracle.canon(dig).reshape(-1), oracle.canon(cap)
        d_dig, d_cap = _zeros(gpu, dig.size), _zeros(gpu, cap.size)
        L.call("gl_merkle_tree_from_columns", cols.ptr, leaf_len, n, stride, h, d_dig.ptr, d_cap.ptr, gpu.ptr)
        gpu.synchronize()
        assert (d_cap.download().reshape(-1, 4) == cap).all(), h
        assert dig.size == 0 or (d_dig.download() == dig).all(), h
        if log_leaves >= 8:
            _open_and_verify(gpu, oracle, cols.ptr, stride, leaf_len, n, h, d_dig, leaves, cap, 10100 + leaf_len)
        d_dig.free()
        d_cap.free()
    d_rows = Strided(gpu, np.broadcast_to(filler(leaf_len, 5), (n, leaf_len)), leaf_len)
    L.call("gl_transpose", cols.ptr, d_rows.ptr, leaf_len, n, stride, gpu.ptr)
    assert (d_rows.polys("transpose") == leaves).all()   # pure data movement: the caller's words
    d_rows.free()
    assert (cols.polys("after the readers") == leaves.T).all()
    cols.free()


# ---- the contract of include/plonky2_hip.h -----------------------------------------------------------------------------------

def test_transform_stride_and_alignment_rules(gpu, oracle):
    """Even strides and 16-byte aligned buffers for gl_ntt_batch, gl_coset_lde_batch and gl_coset_ntt_batch: each violation is
    GL_E_INVALID and leaves the buffer alone; one polynomial may have any stride."""
    L = _L()
    log_n, k = 6, 3
    n = 1 << log_n
    x = oracle.random_field((k, n + 8), seed=10200)
    buf = _dev(gpu, x)
    out = _zeros(gpu, 4 * k * (n + 8))
    for inverse, bit_reversed in ((0, 0), (0, 1)):
        _invalid("gl_ntt_batch", buf.ptr, k, log_n, n + 1, inverse, bit_reversed, gpu.ptr)          # odd stride
        _invalid("gl_ntt_batch", buf.at(1), 1, log_n, n, inverse, bit_reversed, gpu.ptr)            # 8-byte aligned only
    _invalid("gl_ntt_batch", buf.at(1), 1, log_n, n, 1, 0, gpu.ptr)
    _invalid("gl_ntt_batch", buf.ptr, 2, log_n, n + 2, 1, 0, gpu.ptr)                               # inverse: stride % n != 0
    for shift_inverse in (0, 1):
        _invalid("gl_coset_ntt_batch", buf.ptr, k, log_n, n + 1, 7, shift_inverse, gpu.ptr)
        _invalid("gl_coset_ntt_batch", buf.at(1), 1, log_n, n, 7, shift_inverse, gpu.ptr)
        _invalid("gl_coset_ntt_batch", buf.ptr, 1, log_n, n // 2, 7, shift_inverse, gpu.ptr)        # stride < n
    _invalid("gl_coset_ntt_batch", buf.ptr, 2, log_n, n + 2, 7, 1, gpu.ptr)
    _invalid("gl_coset_lde_batch", buf.ptr, out.ptr, k, log_n, 1, 7, n + 1, 2 * n, gpu.ptr)         # odd source stride
    _invalid("gl_coset_lde_batch", buf.ptr, out.ptr, k, log_n, 1, 7, n, 2 * n + 1, gpu.ptr)         # odd destination stride
    _invalid("gl_coset_lde_batch", buf.at(1), out.ptr, 1, log_n, 1, 7, n, 2 * n, gpu.ptr)           # source 8-byte aligned only
    _invalid("gl_coset_lde_batch", buf.ptr, out.at(1), 1, log_n, 1, 7, n, 2 * n, gpu.ptr)           # destination 8-byte aligned only
    _invalid("gl_coset_lde_batch", buf.ptr, out.ptr, k, log_n, 1, 7, n, 2 * n - 2, gpu.ptr)         # destination stride < n_ext
    gpu.synchronize()
    assert (buf.download() == x.reshape(-1)).all(), "a refused call changed the buffer"
    assert not out.download().any(), "a refused call wrote its destination"
    # one polynomial: the stride is not used, an odd one is accepted
    L.call("gl_ntt_batch", buf.ptr, 1, log_n, n + 1, 0, 0, gpu.ptr)
    got = buf.download()
    assert (got[:n] == oracle.canon(oracle.fft(x[0, :n]))).all() and (got[n:] == x.reshape(-1)[n:]).all()
    buf.upload(x)
    L.call("gl_coset_ntt_batch", buf.ptr, 1, log_n, n + 1, 7, 0, gpu.ptr)
    got = buf.download()
    assert (got[:n] == oracle.canon(oracle.coset_fft(x[0, :n], 7))).all() and (got[n:] == x.reshape(-1)[n:]).all()
    buf.free()
    out.free()


def test_overlapping_columns_are_refused(gpu, oracle):
    """col_stride < n_leaves (gl_merkle_tree_from_columns) and col_stride < n_rows (gl_transpose) would read overlapping columns:
    GL_E_INVALID. A single column has no stride: any value is accepted. gl_compute_quotient_polys refuses a column_stride below
    the column length the same way."""
    L = _L()
    n, leaf_len, h = 64, 5, 2
    leaves = oracle.random_field((n, leaf_len), seed=10300)
    cols = _dev(gpu, leaves.T)
    nd = 2 * (n - (1 << h))
    d_dig, d_cap, d_rows = _zeros(gpu, 4 * nd), _zeros(gpu, 4 << h), _zeros(gpu, n * leaf_len)
    for stride in (0, 1, n - 2, n - 1):
        _invalid("gl_merkle_tree_from_columns", cols.ptr, leaf_len, n, stride, h, d_dig.ptr, d_cap.ptr, gpu.ptr)
        _invalid("gl_transpose", cols.ptr, d_rows.ptr, leaf_len, n, stride, gpu.ptr)
    gpu.synchronize()
    assert not d_dig.download().any() and not d_cap.download().any() and not d_rows.download().any()
    one = np.ascontiguousarray(leaves[:, :1])
    dig, cap = oracle.merkle_tree(one, h)
    for stride in (0, n - 1, n):
        L.call("gl_merkle_tree_from_columns", cols.ptr, 1, n, stride, h, d_dig.ptr, d_cap.ptr, gpu.ptr)
        L.call("gl_transpose", cols.ptr, d_rows.ptr, 1, n, stride, gpu.ptr)
        gpu.synchronize()
        assert (d_cap.download().reshape(-1, 4) == oracle.canon(cap)).all() and (d_dig.download().reshape(-1, 4) == oracle.canon(dig)).all()
        assert (d_rows.download(0, n) == one.reshape(-1)).all()
    # the quotient: column-major leaves with a stride below n_ext
    degree_bits, rate_bits, qdf = 4, 3, 8
    n_ext = 1 << (degree_bits + rate_bits)
    d_any = _zeros(gpu, 64 * n_ext)
    h3 = np.array([1, 2, 3], dtype=np.uint64)
    args = L.GlQuotientArgs(d_any.ptr, d_any.ptr, d_any.ptr, 12, 14, 3, d_any.ptr, None, h3.ctypes.data, h3.ctypes.data, h3.ctypes.data,
                            2, 12, 1, 0, degree_bits, rate_bits, qdf, 7, None, n_ext - 2, None, None, None)
    _invalid("gl_compute_quotient_polys", ctypes.byref(args), d_any.ptr, gpu.ptr)
    for b in (cols, d_dig, d_cap, d_rows, d_any):
        b.free()
