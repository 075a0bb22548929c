"""Every entry point of include/plonky2_hip.h that takes a pitch, at a pitch that puts the last column more than 2^32 words behind
the first (tests/far.py): a product `column * stride` formed in 32 bits, in words or in bytes, signed or not, gives a wrong value
or a changed guard word here and passes every other test. The matrices are tiny, so a case costs what its reference costs.

Every comparison is equality with what the tests of the same entry point at small pitches compare with — the C oracle, Python
integers or the tests/*_ref.py restatements — computed at the tight pitch; read-only inputs are read back and compared, and every
column stands between guard words that are checked when it is read.

entry point                                   -> test
  gl_ntt_batch (forward, bit-reversed, inverse)  test_ntt[5|13|20|22-*]         one pass, two passes, 2^20, 2^22; three passes:
                                                                                 test_gpu_ntt.py::test_ntt_batch_with_more_than_2e32_elements
  gl_coset_ntt_batch                             test_coset_ntt[5|13-*]
  gl_coset_lde_batch                             test_coset_lde[3-3 .. 22-1-both|dst]
  gl_merkle_tree_from_columns, _h                test_merkle_tree_from_columns[poseidon|keccak-3|9|135-256|8192]
  gl_merkle_open_batch, _device                  test_merkle_openings_in_place[columns|rows]
  gl_transpose                                   test_transpose[3|135|200]
  gl_pack_leaf_ranges                            test_pack_leaf_ranges
  gl_keccak_hash_no_pad_batch                    test_keccak_hash_no_pad_batch[7|25]
  gl_permutation_partial_products                test_permutation_partial_products
  gl_eval_polys_ext2                             test_eval_polys_ext2[3|135-3|13]
  gl_compute_quotient_polys                      test_compute_quotient_polys (interpreted gate_program, then gl_gate_kernel_build)
  gl_stark_permutation_zs                        test_stark_permutation_zs
  gl_stark_quotient_polys                        test_stark_quotient_polys (interpreted, then compiled in units)
  gl_stark_tables_ctl_zs                         test_stark_tables_ctl_zs
  gl_stark_tables_quotient_polys                 test_stark_tables_quotient_polys
  gl_stark_fill_lookups                          test_stark_fill_lookups
  gl_keccak_table_trace                          test_keccak_table_trace
  gl_memory_table_trace                          test_memory_table_trace
  gl_logic_table_trace                           test_logic_table_trace
  gl_keccak_sponge_table_trace, _ops             test_keccak_sponge_table_trace_and_ops
  gl_arithmetic_table_trace                      test_arithmetic_table_trace

The library-owned LDEs of gl_prove / gl_stark_prove / gl_commit_* have no pitch a caller can set and reach 2^32 words only at real
sizes: not here. gl_merkle_open_batch takes trees of 2^k leaves: the leaf-major rows at a far row_stride are 16, of which 9 are
opened."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import far  # noqa: E402
import strided  # noqa: E402
from far import Far  # noqa: E402
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from strided import bitrev_perm, filler  # noqa: E402

P = 0xFFFFFFFF00000001
ONES = (1 << 64) - 1


def _L():
    from plonky2_gpu_amd import _lib

    return _lib


def _pg():
    import plonky2_gpu_amd as pg

    return pg


def _dev(gpu, a):
    return _pg().DeviceBuffer.from_host(gpu, np.ascontiguousarray(a, dtype=np.uint64).reshape(-1))


def _sentinels(gpu, n, start=0):
    """a tight output buffer of filler words with 64 more behind it: (buffer, .download()[:n] with the tail checked)"""
    buf = _pg().DeviceBuffer.from_host(gpu, filler(n + 64, start))

    def read():
        out = buf.download()
        assert (out[n:] == filler(n + 64, start)[n:]).all(), "the words behind a tight output were written"
        return out[:n]

    return buf, read


def _first_difference(got, exp):
    bad = np.argwhere(got != exp)
    return None if bad.size == 0 else ("first (column, word) that differs", bad[0].tolist(), len(bad), hex(int(got[tuple(bad[0])])), hex(int(exp[tuple(bad[0])])))


def _any_words(rng, *shape):
    """uniform words below p, one in eight moved into [p, 2^64): what tests/test_gpu_ctl.py plants"""
    w = rng.integers(0, P, size=shape, dtype=np.uint64)
    high = rng.integers(P, 1 << 64, size=shape, dtype=np.uint64)
    return np.where(rng.random(shape) < 0.125, high, w)


@pytest.fixture(scope="module")
def room(gpu):
    """the module's one far allocation (48 GiB + 128 MiB); only a device too small for it anyway skips"""
    if far.device_bytes() < far.MIN_DEVICE_BYTES:
        pytest.skip("the device has less than 96 GiB")
    alloc = far.FarAllocation(gpu)
    yield alloc
    assert not alloc.live, "a test left a matrix in the far allocation"
    alloc.free()


# ---- the layouts, and the CPU test that they can tell a cut offset from a whole one -----------------------------------------------

NTT_LOG_N = [5, 13, 20, 22]
COSET_NTT_LOG_N = [5, 13]
LDE_SHAPES = [(3, 3), (12, 3), (13, 3), (18, 1), (22, 1)]
MERKLE_LEAF_LENS, MERKLE_LEAVES = [3, 9, 135], [256, 1 << 13]
TRANSPOSE_COLS, TRANSPOSE_ROWS = [3, 135, 200], (64 << 10) + 5
EVAL_SHAPES = [(3, 3), (3, 13), (135, 3), (135, 13)]


def _ntt_layout(log_n, order):
    return far.declare(3, 1 << log_n, multiple_of=(1 << log_n) if order == "inverse" else 1)


def _lde_layouts(log_n, rate_bits):
    """the source in slot 0, the destination in the first slot behind it"""
    n = 1 << log_n
    return far.declare(3, n), far.declare(3, n << rate_bits, slot=(n + 2 * far.GUARD) // far.SLOT + 1), far.declare(3, n << rate_bits)


def _declare_all():
    for log_n in NTT_LOG_N:
        for order in ("forward", "inverse"):
            _ntt_layout(log_n, order)
    for shape in LDE_SHAPES:
        _lde_layouts(*shape)
    for k in MERKLE_LEAF_LENS:
        for n in MERKLE_LEAVES:
            far.declare(k, n)
    far.declare(16, 7)                                   # leaf-major rows at a far row_stride
    for c in TRANSPOSE_COLS:
        far.declare(c, TRANSPOSE_ROWS)
    far.declare(9, 1 << 10)                              # gl_pack_leaf_ranges
    for length in (7, 25):
        far.declare(9, length)                           # gl_keccak_hash_no_pad_batch
    far.declare(83, 64), far.declare(80, 64, slot=1)     # wires and sigmas of 80 routed wires
    for k, log_n in EVAL_SHAPES:
        far.declare(k, 1 << log_n)
    far.declare(12, 128, pitch_of=16), far.declare(16, 128, slot=1), far.declare(4, 128, slot=2, pitch_of=16)   # the plonk quotient
    far.declare(5, 32)                                   # B's trace, the CTL table's trace
    far.declare(5, 64), far.declare(5, 64, slot=1)       # B's LDE and the LDE of its five Zs
    far.declare(8, 1000)                                 # gl_stark_fill_lookups
    for cols, n in ((2430, 128), (26, 128), (523, 128), (414, 32), (92, 128)):
        far.declare(cols, n)                             # the five tables


_declare_all()


def _tables_quotient_case():
    import test_gpu_ctl as tgc

    rs = tgc._random_system(7)   # 3 CTL Zs, one permutation Z, qdf 3, 2^4 rows
    desc = rs.desc()
    return rs, desc, 1 << (rs.degree_bits + rs.rate_bits)


def _tables_quotient_layouts():
    rs, desc, n_ext = _tables_quotient_case()
    cols, zs = rs.tables[0].num_columns, desc.num_zs(0)
    wide = max(cols, zs)
    return far.declare(cols, n_ext, pitch_of=wide), far.declare(zs, n_ext, slot=1, pitch_of=wide)


_tables_quotient_layouts()
far.freeze()


@pytest.mark.parametrize("key", sorted(far.DECLARED))
def test_the_layout_tells_a_cut_offset_from_a_whole_one(key):
    """no GPU: for each of the four truncations (u32 / i32 of the word offset, u32 / i32 of the byte offset) some column's cut window
    is disjoint from its true one, every cut window lies inside the allocation, and some column starts at or behind each of 2^29,
    2^31 and 2^32 words. A matrix that follows the pitch of a wider one of its call stays inside the allocation."""
    lay = far.DECLARED[key]
    far.check_layout(lay)
    if lay.pitch_of == lay.cols:
        assert lay.stride == far.far_pitch(lay.cols, 1) or lay.stride % lay.width == 0
        for name, cut in far.TRUNCATIONS.items():
            last = (lay.cols - 1) * lay.stride
            assert cut(last) != last, name


def test_the_pitches_cross_the_thresholds_where_the_issue_says():
    """no GPU: the first column at or behind 2^29, 2^31 and 2^32 words for the widths the product has"""
    exp = {3: (1, 1, 2), 9: (1, 4, 8), 26: (4, 13, 25), 80: (10, 40, 79), 92: (12, 46, 91), 135: (17, 67, 134), 414: (52, 207, 413),
           523: (66, 261, 522), 2430: (304, 1215, 2429)}
    for cols, firsts in exp.items():
        s = far.far_pitch(cols)
        assert s % 2 == 0 and (cols - 1) * s >= (1 << 32) + 2 > (cols - 1) * (s - 2)
        assert tuple(next(c for c in range(cols) if c * s >= t) for t in far.THRESHOLDS) == firsts
    assert far.far_pitch(3, 1 << 13) % (1 << 13) == 0 and far.WORDS * 8 == (48 << 30) + (128 << 20)


# ---- transforms ---------------------------------------------------------------------------------------------------------------

_ntt_cases = {}


def _ntt_case(oracle, log_n):
    if log_n not in _ntt_cases:
        _ntt_cases.clear()
        _ntt_cases[log_n] = strided.ntt_case(oracle, log_n, 3)
    return _ntt_cases[log_n]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["forward", "bit_reversed", "inverse"])
@pytest.mark.parametrize("log_n", NTT_LOG_N)
def test_ntt(gpu, oracle, room, log_n, order):
    """three polynomials, the third behind 2^32 words; the inverse at the smallest such pitch that is a multiple of n"""
    x, exp_f, exp_i, perm = _ntt_case(oracle, log_n)
    exp = {"forward": exp_f, "inverse": exp_i}[order] if order != "bit_reversed" else exp_f[:, perm]
    f = Far(room, _ntt_layout(log_n, order), x)
    try:
        assert order != "inverse" or f.stride % (1 << log_n) == 0
        _L().call("gl_ntt_batch", f.ptr, 3, log_n, f.stride, int(order == "inverse"), int(order == "bit_reversed"), gpu.ptr)
        got = f.read((log_n, order))
    finally:
        f.free()
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, (order, "stride", f.stride, "polynomials that differ from the oracle", bad.tolist())
    if order == "inverse" and log_n == NTT_LOG_N[-1]:
        _ntt_cases.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("log_n", COSET_NTT_LOG_N)
def test_coset_ntt(gpu, oracle, room, log_n, inverse):
    x = oracle.random_field((3, 1 << log_n), seed=11000 + log_n)
    strided.lift_some(x, 1, 11001 + log_n)
    exp = np.array([oracle.canon((oracle.coset_ifft if inverse else oracle.coset_fft)(c, 7)) for c in oracle.canon(x)])
    f = Far(room, _ntt_layout(log_n, "inverse" if inverse else "forward"), x)
    try:
        _L().call("gl_coset_ntt_batch", f.ptr, 3, log_n, f.stride, 7, inverse, gpu.ptr)
        got = f.read((log_n, inverse))
    finally:
        f.free()
    assert _first_difference(got, exp) is None, _first_difference(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["both", "dst"])
@pytest.mark.parametrize("log_n,rate_bits", LDE_SHAPES)
def test_coset_lde(gpu, oracle, room, log_n, rate_bits, where):
    """source and destination both far in the one allocation, then the destination alone (the source tight in a buffer of its own)"""
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    c = oracle.random_field((3, n), seed=11100 + 10 * log_n + rate_bits)
    strided.lift_some(c, 1, 11200 + log_n)
    exp = oracle.canon(oracle.coset_lde_batch(oracle.canon(c), rate_bits, threads=4))[:, bitrev_perm(log_n + rate_bits)]
    l_src, l_dst_shared, l_dst = _lde_layouts(log_n, rate_bits)
    src = Far(room, l_src, c) if where == "both" else strided.Strided(gpu, c, n)
    dst = Far.filled(room, l_dst_shared if where == "both" else l_dst, 7)
    try:
        _L().call("gl_coset_lde_batch", src.ptr, dst.ptr, 3, log_n, rate_bits, 7, src.stride, dst.stride, gpu.ptr)
        got = dst.read(("lde", log_n, rate_bits, where))
        if where == "both":
            src.unchanged("the source of the LDE")
        else:
            assert (src.polys("the source of the LDE") == c).all()
    finally:
        dst.free()
        src.free()
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, (where, "polynomials that differ from the oracle", bad.tolist())


# ---- hashing, trees, openings -------------------------------------------------------------------------------------------------

def _leaves(oracle, n, k, seed):
    leaves = oracle.random_field((n, k), seed=seed)
    strided.lift_some(leaves.reshape(1, -1), 0, seed + 1)
    return leaves


def _tree(oracle, hasher, leaves, h):
    """(digest words, cap words [2^h][4]) of the reference"""
    if hasher == "poseidon":
        dig, cap = oracle.merkle_tree(oracle.canon(leaves), h, threads=4)
        return oracle.canon(dig).reshape(-1), oracle.canon(cap)
    import keccak_ref as kr

    dig, cap = kr.merkle_tree(leaves, h)
    return kr.slots(dig).reshape(-1), kr.slots(cap)


@pytest.mark.gpu
@pytest.mark.parametrize("n", MERKLE_LEAVES)
@pytest.mark.parametrize("leaf_len", MERKLE_LEAF_LENS)
@pytest.mark.parametrize("hasher", ["poseidon", "keccak"])
def test_merkle_tree_from_columns(gpu, oracle, room, hasher, leaf_len, n):
    """leaves of 3 words (their own digest under Poseidon), of 9 (more than one rate block) and of 135; cap heights 0 and 4; Poseidon
    through both entry points"""
    L = _L()
    leaves = _leaves(oracle, n, leaf_len, 11300 + 7 * leaf_len + n)
    cols = Far(room, far.declare(leaf_len, n), leaves.T)
    try:
        for h in (0, 4):
            dig, cap = _tree(oracle, hasher, leaves, h)
            calls = [("gl_merkle_tree_from_columns_h", (L.HASHERS[hasher],))] + ([("gl_merkle_tree_from_columns", ())] if hasher == "poseidon" else [])
            for name, head in calls:
                (d_dig, read_dig), (d_cap, read_cap) = _sentinels(gpu, dig.size, 1), _sentinels(gpu, cap.size, 2)
                L.call(name, *head, cols.ptr, leaf_len, n, cols.stride, h, d_dig.ptr, d_cap.ptr, gpu.ptr)
                gpu.synchronize()
                assert (read_cap().reshape(-1, 4) == cap).all(), (name, h)
                assert (read_dig() == dig).all(), (name, h)
                d_dig.free(), d_cap.free()
        cols.unchanged("the leaves")
    finally:
        cols.free()


def _open_both_ways(gpu, oracle, d_leaves, row_stride, elem_stride, leaves, h, d_dig, cap):
    """gl_merkle_open_batch and gl_merkle_open_batch_device: leaf 0, the last leaf, one leaf twice and others; the opened leaves are
    the caller's words and every path verifies to the cap"""
    L = _L()
    n, leaf_len = leaves.shape
    layers = n.bit_length() - 1 - h
    canon = oracle.canon(leaves)
    idx = np.array([0, n - 1, 5, 5, n // 2, 1, n - 2, 7, 3], dtype=np.uint64)
    h_l, h_s = np.zeros(idx.size * leaf_len, dtype=np.uint64), np.zeros(max(idx.size * layers * 4, 1), dtype=np.uint64)
    L.call("gl_merkle_open_batch", d_leaves, row_stride, elem_stride, leaf_len, n, h, d_dig.ptr, idx, idx.size, h_l, h_s, gpu.ptr)
    assert (h_l.reshape(idx.size, leaf_len) == leaves[idx.astype(np.int64)]).all()
    sib = h_s[: idx.size * layers * 4].reshape(idx.size, layers, 4)
    for q, i in enumerate(idx):
        assert oracle.merkle_verify(canon[int(i)], int(i), cap, sib[q]), ("host indices", int(i))
    shift = 3
    want = idx.astype(np.int64)
    raw = (idx << np.uint64(shift)) + np.uint64(5) + np.arange(idx.size, dtype=np.uint64) * np.uint64(n << shift)   # leaf = (raw mod (n << shift)) >> shift
    (d_ol, read_l), (d_os, read_s) = _sentinels(gpu, raw.size * leaf_len, 3), _sentinels(gpu, raw.size * layers * 4, 4)
    d_raw = _dev(gpu, raw)
    L.call("gl_merkle_open_batch_device", d_leaves, row_stride, elem_stride, leaf_len, n, h, d_dig.ptr, d_raw.ptr, raw.size, shift,
           d_ol.ptr, d_os.ptr, gpu.ptr)
    gpu.synchronize()
    assert (read_l().reshape(raw.size, leaf_len) == leaves[want]).all()
    sib = read_s().reshape(raw.size, layers, 4)
    for q, i in enumerate(want):
        assert oracle.merkle_verify(canon[int(i)], int(i), cap, sib[q]), ("raw challenges", int(i))
    for b in (d_raw, d_ol, d_os):
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["columns", "rows"])
def test_merkle_openings_in_place(gpu, oracle, room, layout):
    """columns: the LDE's layout (row_stride, elem_stride) = (1, S) with 9 columns of 256 leaves; rows: 16 leaf-major rows of 7 words
    at a far row_stride, elem_stride 1"""
    n, leaf_len = (256, 9) if layout == "columns" else (16, 7)
    leaves = _leaves(oracle, n, leaf_len, 11400 + n)
    f = Far(room, far.declare(leaf_len, n), leaves.T) if layout == "columns" else Far(room, far.declare(n, leaf_len), leaves)
    try:
        for h in (0, 2):
            dig, cap = _tree(oracle, "poseidon", leaves, h)
            d_dig = _dev(gpu, dig)
            strides = (1, f.stride) if layout == "columns" else (f.stride, 1)
            _open_both_ways(gpu, oracle, f.ptr, *strides, leaves, h, d_dig, cap)
            d_dig.free()
        f.unchanged("the leaves")
    finally:
        f.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n_cols", TRANSPOSE_COLS)
def test_transpose(gpu, oracle, room, n_cols):
    """64 k + 5 rows: more than one tile in both directions, both ragged; and back through the tight call"""
    L = _L()
    rows = TRANSPOSE_ROWS
    m = oracle.random_field((n_cols, rows), seed=11500 + n_cols)
    m[n_cols - 1, -1] = np.uint64(ONES)
    f = Far(room, far.declare(n_cols, rows), m)
    try:
        d_rows, read = _sentinels(gpu, n_cols * rows, 5)
        L.call("gl_transpose", f.ptr, d_rows.ptr, n_cols, rows, f.stride, gpu.ptr)
        gpu.synchronize()
        got = read().reshape(rows, n_cols)
        bad = np.argwhere(got != m.T)
        assert bad.size == 0, ("first (row, column) that differs", bad[0].tolist(), len(bad), hex(int(got[tuple(bad[0])])), hex(int(m.T[tuple(bad[0])])))
        f.unchanged("the columns")
        d_back, read_back = _sentinels(gpu, n_cols * rows, 6)
        L.call("gl_transpose", d_rows.ptr, d_back.ptr, rows, n_cols, n_cols, gpu.ptr)   # the rows as `rows` columns of n_cols words
        gpu.synchronize()
        assert (read_back().reshape(n_cols, rows) == m).all()
        d_rows.free(), d_back.free()
    finally:
        f.free()


@pytest.mark.gpu
def test_pack_leaf_ranges(gpu, oracle, room):
    """d_out[(q * n_cols + c) * per + i] = d_lde[c * col_stride + q * per + i] for 2 and for 4 ranks"""
    n_cols, n = 9, 1 << 10
    m = oracle.random_field((n_cols, n), seed=11600)
    f = Far(room, far.declare(n_cols, n), m)
    try:
        for world in (2, 4):
            per = n // world
            d_out, read = _sentinels(gpu, n_cols * n, 7)
            _L().call("gl_pack_leaf_ranges", f.ptr, f.stride, n_cols, per, world, d_out.ptr, gpu.ptr)
            gpu.synchronize()
            got = read().reshape(world, n_cols, per)
            for q in range(world):
                assert (got[q] == m[:, q * per : (q + 1) * per]).all(), (world, q)
            d_out.free()
        f.unchanged("the LDE")
    finally:
        f.free()


@pytest.mark.gpu
@pytest.mark.parametrize("length", [7, 25])
def test_keccak_hash_no_pad_batch(gpu, room, length):
    import keccak_ref as kr

    count = 9
    data = _any_words(np.random.default_rng(11700 + length), count, length)
    f = Far(room, far.declare(count, length), data)
    try:
        d_out, read = _sentinels(gpu, 4 * count, 8)
        _L().call("gl_keccak_hash_no_pad_batch", f.ptr, length, f.stride, count, d_out.ptr, gpu.ptr)
        gpu.synchronize()
        assert (read().reshape(count, 4) == kr.slots(kr.hash_no_pad(data))).all()
        f.unchanged("the inputs")
        d_out.free()
    finally:
        f.free()


# ---- plonk --------------------------------------------------------------------------------------------------------------------

def _cols(a):
    return np.array(a, dtype=np.uint64)


@pytest.mark.gpu
def test_permutation_partial_products(gpu, room):
    """80 routed wires of 83, 2^6 rows: wires and sigmas both far, each at the pitch of its own width"""
    from oracle import plonk_ref
    from plonk_instance import make_instance
    from plonky2_gpu_amd.prover import num_partial_products

    num_routed, degree_bits, qdf = 80, 6, 8
    inst = make_instance(degree_bits=degree_bits, num_wires=num_routed + 3, num_routed=num_routed, num_challenges=2, seed=num_routed * 7 + degree_bits)
    n = inst["n"]
    exp = _cols(plonk_ref.zs_partial_products(inst["wires"], inst["sigmas"], inst["k_is"], inst["betas"], inst["gammas"], qdf, inst["subgroup"]))
    w, s = Far(room, far.declare(83, n), _cols(inst["wires"])), Far(room, far.declare(80, n, slot=1), _cols(inst["sigmas"]))
    try:
        d_k = _dev(gpu, _cols(inst["k_is"]))
        n_cols = 2 * (1 + num_partial_products(num_routed, qdf))
        assert exp.shape == (n_cols, n)
        d_out, read = _sentinels(gpu, n_cols * n, 9)
        _L().call("gl_permutation_partial_products", w.ptr, w.stride, s.ptr, s.stride, d_k.ptr, _cols(inst["betas"]), _cols(inst["gammas"]), 2,
                  num_routed, qdf, degree_bits, d_out.ptr, gpu.ptr)
        gpu.synchronize()
        got = read().reshape(n_cols, n)
        assert _first_difference(got, exp) is None, _first_difference(got, exp)
        w.unchanged("the wires"), s.unchanged("the sigmas")
        d_k.free(), d_out.free()
    finally:
        w.free(), s.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n_polys,log_n", EVAL_SHAPES)
def test_eval_polys_ext2(gpu, oracle, room, n_polys, log_n):
    """two points of the quadratic extension; at 2^13 coefficients the polynomials compared with Python integers are the first, the
    last and the first at or behind each threshold"""
    import random

    from oracle import plonk_ref, pyref

    n = 1 << log_n
    coeffs = oracle.random_field((n_polys, n), seed=n_polys * 31 + log_n)
    rng = random.Random(log_n)
    zeta = (rng.randrange(P), rng.randrange(P))
    pts = [zeta, plonk_ref.ext2_mul((pyref.root_of_unity(log_n), 0), zeta)]
    f = Far(room, far.declare(n_polys, n), coeffs)
    try:
        d_out, read = _sentinels(gpu, len(pts) * n_polys * 2, 10)
        _L().call("gl_eval_polys_ext2", f.ptr, n_polys, log_n, f.stride, _cols(pts).reshape(-1), len(pts), d_out.ptr, gpu.ptr)
        gpu.synchronize()
        got = read().reshape(len(pts), n_polys, 2)
        f.unchanged("the coefficients")
        d_out.free()
    finally:
        f.free()
    firsts = {next(c for c in range(n_polys) if c * f.stride >= t) for t in far.THRESHOLDS}
    sample = range(n_polys) if n <= 4096 else sorted({0, n_polys - 1} | firsts)
    for q, z in enumerate(pts):
        for i in sample:
            assert tuple(int(v) for v in got[q, i]) == plonk_ref.eval_ext2([int(c) for c in coeffs[i]], z), (q, i)


@functools.lru_cache(maxsize=None)
def _plonk_quotient_case():
    """the small circuit of tests/test_gpu_plonk.py::test_quotient_with_table_driven_gates: (instance, the three column-major LDEs,
    the reference's quotient)"""
    from oracle import plonk_ref, pyref
    from plonk_instance import lde_leaves, make_circuit_instance

    degree_bits, rate_bits, qdf = 4, 3, 8
    inst = make_circuit_instance(degree_bits=degree_bits, seed=22, two_groups=True)
    n, nc = inst["n"], inst["num_constants"]
    zpp = plonk_ref.zs_partial_products(inst["wires"], inst["sigmas"], inst["k_is"], inst["betas"], inst["gammas"], qdf, inst["subgroup"])
    w_l, cs_l, z_l = (lde_leaves(c, rate_bits)[1] for c in (inst["wires"], inst["constants"] + inst["sigmas"], zpp))
    bits = degree_bits + rate_bits
    gate_terms = [plonk_ref.evaluate_gate_constraints(inst["gates"], inst["selector_indices"], inst["groups"], 4,
                                                      cs_l[pyref.reverse_bits(i, bits)][:nc], w_l[pyref.reverse_bits(i, bits)], inst["pih"]) for i in range(n * 8)]
    exp = _cols(plonk_ref.compute_quotient_polys(w_l, cs_l, z_l, nc, inst["k_is"], inst["betas"], inst["gammas"], inst["alphas"], degree_bits, rate_bits,
                                                 qdf, gate_terms))
    ldes = tuple(np.ascontiguousarray(_cols(leaves).T) for leaves in (w_l, cs_l, z_l))
    assert [a.shape for a in ldes] == [(12, 128), (16, 128), (4, 128)]
    return inst, ldes, exp


@pytest.mark.gpu
def test_compute_quotient_polys(gpu, room):
    """the three LDEs in the one allocation at ONE far column_stride (that of the widest, constants and sigmas: 16 columns); the gate
    constraints once through the interpreted gate_program and once through a gl_gate_kernel_build kernel"""
    pg, L = _pg(), _L()
    from plonky2_gpu_amd import gate_program as gp

    inst, ldes, exp = _plonk_quotient_case()
    degree_bits, rate_bits, qdf, num_ch = 4, 3, 8, 2
    lays = (far.declare(12, 128, pitch_of=16), far.declare(16, 128, slot=1), far.declare(4, 128, slot=2, pitch_of=16))
    fs = [Far(room, lay, a) for lay, a in zip(lays, ldes)]
    try:
        stride = fs[1].stride
        assert all(f.stride == stride for f in fs)
        d_k = _dev(gpu, _cols(inst["k_is"]))
        prog = pg.GateProgram(gpu, [gp.noop_gate(), gp.constant_gate(2), gp.public_input_gate(), gp.arithmetic_gate(3)], inst["selector_indices"],
                              inst["groups"], inst["pih"])
        b, g, a, pih = (_cols(inst[k]) for k in ("betas", "gammas", "alphas", "pih"))
        size = num_ch << (degree_bits + (qdf - 1).bit_length())
        for compiled in (False, True):
            if compiled:
                prog.compile(inst["num_gate_constraints"], num_ch)
            work = pg.DeviceBuffer(gpu, size) if compiled else None
            args = L.GlQuotientArgs(fs[0].ptr, fs[1].ptr, fs[2].ptr, 12, 16, 4, d_k.ptr, None, b.ctypes.data, g.ctypes.data, a.ctypes.data,
                                    inst["num_constants"], 12, num_ch, inst["num_gate_constraints"], degree_bits, rate_bits, qdf, 7,
                                    None if compiled else ctypes.pointer(prog.struct), stride, prog.kernel if compiled else None,
                                    pih.ctypes.data if compiled else None, work.ptr if compiled else None)
            d_q, read = _sentinels(gpu, size, 11)
            L.call("gl_compute_quotient_polys", ctypes.byref(args), d_q.ptr, gpu.ptr)
            gpu.synchronize()
            got = read().reshape(num_ch, -1)
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("compiled gates" if compiled else "interpreted gates", "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad))
            d_q.free()
            if work:
                work.free()
        for f, what in zip(fs, ("wires", "constants and sigmas", "zs and partial products")):
            f.unchanged(what)
        d_k.free()
    finally:
        for f in fs:
            f.free()


# ---- STARK --------------------------------------------------------------------------------------------------------------------

def _sets(rng, qdf, num_challenges, words=None):
    draw = words or (lambda r, *s: r.integers(0, P, size=s, dtype=np.uint64))
    return [[tuple(int(x) for x in draw(rng, 2)) for _ in range(num_challenges)] for _ in range(qdf)]


@pytest.mark.gpu
def test_stark_permutation_zs(gpu, room):
    """B (three permutation pairs, 3 challenges: 5 Zs in batches of two, the last one short) on 2^5 rows of random words with
    non-canonical ones among them; the reference gets the words reduced"""
    import stark_instances as si
    import stark_ref as sr
    from plonky2_gpu_amd.stark import _challenge_words

    stark, degree_bits, num_ch = si.B, 5, 3
    n = 1 << degree_bits
    rng = np.random.default_rng(11800)
    trace = _any_words(rng, stark.num_columns, n)
    sets = _sets(rng, sr.quotient_degree_factor(stark), num_ch)
    exp = _cols(sr.compute_permutation_z_polys(stark, num_ch, (trace % np.uint64(P)).tolist(), sets))
    ns = _pg().NativeStark(gpu, stark.desc(degree_bits, num_ch, si.fri_params(rate_bits=2)))
    t = Far(room, far.declare(stark.num_columns, n), trace)
    try:
        assert exp.shape == (ns.desc.num_zs, n) and exp.all()
        d_z, read = _sentinels(gpu, exp.size, 12)
        _L().call("gl_stark_permutation_zs", ns.ptr, t.ptr, t.stride, _challenge_words(sets), d_z.ptr, gpu.ptr)
        gpu.synchronize()
        got = read().reshape(exp.shape)
        assert _first_difference(got, exp) is None, _first_difference(got, exp)
        t.unchanged("the trace")
        d_z.free()
    finally:
        t.free()
        ns.close()


@pytest.mark.gpu
def test_stark_quotient_polys(gpu, room):
    """B on 2^4 rows at rate_bits 2: random words with non-canonical ones in place of the LDEs of the trace and of the five Zs, both
    in the one allocation at one far column_stride; interpreted, then compiled in units of at most 6 instructions"""
    import stark_instances as si
    import stark_ref as sr

    stark, degree_bits, rate_bits, num_ch = si.B, 4, 2, 3
    n_ext = 1 << (degree_bits + rate_bits)
    rng = np.random.default_rng(11900)
    ns = _pg().NativeStark(gpu, stark.desc(degree_bits, num_ch, si.fri_params(rate_bits=rate_bits)))
    lde, zs = _any_words(rng, stark.num_columns, n_ext), _any_words(rng, ns.desc.num_zs, n_ext)
    assert (lde >= np.uint64(P)).any() and (zs >= np.uint64(P)).any() and zs.shape[0] == 5
    sets = _sets(rng, sr.quotient_degree_factor(stark), num_ch)
    alphas = [int(x) for x in rng.integers(0, P, size=num_ch, dtype=np.uint64)]
    pis = [int(x) for x in rng.integers(0, P, size=stark.num_public_inputs, dtype=np.uint64)]
    leaves = lambda a: (a % np.uint64(P)).T.tolist()  # noqa: E731
    exp = _cols(sr.compute_quotient_polys(stark, num_ch, degree_bits, rate_bits, leaves(lde), leaves(zs), sets, pis, alphas))
    assert exp.all()
    t, z = Far(room, far.declare(5, n_ext), lde), Far(room, far.declare(5, n_ext, slot=1), zs)
    try:
        assert t.stride == z.stride
        for units in (None, 6):
            if units:
                ns.compile(unit_instrs=units)
                assert ns.is_compiled and ns.num_units > 1
            got = ns.quotient_polys(t.ptr, z.ptr, t.stride, alphas, sets, pis)
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("units", units, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad))
        t.unchanged("the trace LDE"), z.unchanged("the Zs LDE")
    finally:
        t.free(), z.free()
        ns.close()


@pytest.mark.gpu
def test_stark_tables_ctl_zs(gpu, room):
    """the two-table description of tests/test_gpu_ctl.py (filters, a combination with a large coefficient, a constant column) on 2^5
    rows with non-canonical filter words and values"""
    import ctl_ref as cr
    import test_gpu_ctl as tgc

    degree_bits, num_ch = 5, 2
    n = 1 << degree_bits
    desc = tgc._zs_desc(degree_bits, num_ch)
    trace = tgc._zs_trace(degree_bits, "mixed", 12000)
    challenges = tgc._pairs(np.random.default_rng(12001), num_ch)
    exp = _cols(cr.ctl_z_polys(desc.lookups, num_ch, 0, trace.tolist(), challenges))
    assert exp.shape == (3 * num_ch, n)
    nt = _pg().NativeStarkTables(gpu, desc)
    t = Far(room, far.declare(5, n), trace)
    try:
        d_z, read = _sentinels(gpu, exp.size, 13)
        _L().call("gl_stark_tables_ctl_zs", nt.ptr, 0, t.ptr, t.stride, _cols([w for bg in challenges for w in bg]), d_z.ptr, gpu.ptr)
        gpu.synchronize()
        got = read().reshape(exp.shape)
        assert _first_difference(got, exp) is None, _first_difference(got, exp)
        t.unchanged("the trace")
        d_z.free()
    finally:
        t.free()
        nt.close()


@pytest.mark.gpu
def test_stark_tables_quotient_polys(gpu, room):
    """table 0 of a random description (three CTL Zs and a permutation Z, qdf 3, 2^4 rows) on any u64 in place of the two LDEs"""
    import ctl_ref as cr
    import stark_ref as sr
    import test_gpu_ctl as tgc
    from oracle import accel

    rs, desc, n_ext = _tables_quotient_case()
    num_ch, stark = rs.num_challenges, rs.tables[0]
    l_t, l_z = _tables_quotient_layouts()
    rng = np.random.default_rng(12100)
    words = tgc._any_words
    trace, zs = words(rng, l_t.cols, n_ext), words(rng, l_z.cols, n_ext)
    sets = [tgc._pairs(rng, num_ch, words) for _ in range(sr.quotient_degree_factor(stark))] if stark.pairs else None
    ctl_challenges, alphas = tgc._pairs(rng, num_ch, words), [int(x) for x in words(rng, num_ch)]
    reduced = lambda a: (a % np.uint64(P)).T.tolist()  # noqa: E731
    mod = lambda pairs: [(a % P, b % P) for a, b in pairs]  # noqa: E731
    with accel.c_backend():
        exp = _cols(cr.compute_quotient_polys(rs, 0, num_ch, rs.degree_bits, rs.rate_bits, reduced(trace), reduced(zs), sets and [mod(s) for s in sets],
                                              mod(ctl_challenges), [a % P for a in alphas]))
    nt = _pg().NativeStarkTables(gpu, desc)
    t, z = Far(room, l_t, trace), Far(room, l_z, zs)
    try:
        assert t.stride == z.stride
        got = nt.quotient_polys(0, t.ptr, z.ptr, t.stride, alphas, sets, ctl_challenges)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, ("first (challenge, coefficient) that differs", bad[0].tolist(), len(bad))
        t.unchanged("the trace LDE"), z.unchanged("the Zs LDE")
    finally:
        t.free(), z.free()
        nt.close()


@pytest.mark.gpu
def test_stark_fill_lookups(gpu, room):
    """the case of tests/test_gpu_lookup.py: two lookups that share their table column, 1000 rows; the permuted columns are written,
    every other column and every guard is as it was"""
    import lookup_ref as lr
    from plonky2_gpu_amd import lookup

    n, num_columns = 1000, 8
    rng = np.random.default_rng(12200)
    host = rng.integers(0, P, size=(num_columns, n), dtype=np.uint64)
    host[0], host[1], host[5] = np.arange(n), rng.integers(0, n, size=n), rng.integers(0, n + 20, size=n)
    lookups = [(1, 0, 2, 3), (5, 0, 7, 4)]
    exp = host.copy()
    for c_in, c_t, c_pi, c_pt in lookups:
        exp[c_pi], exp[c_pt] = lr.permuted_cols(host[c_in].tolist(), host[c_t].tolist())
    t = Far(room, far.declare(num_columns, n), host)
    try:
        lookup.fill_lookups(gpu, t.ptr, n, num_columns, lookups, trace_stride=t.stride)
        got = t.read("the trace")
    finally:
        t.free()
    assert _first_difference(got, exp) is None, _first_difference(got, exp)


# ---- the tables ---------------------------------------------------------------------------------------------------------------

def _table_trace(room, columns, n):
    return Far.filled(room, far.declare(columns, n), 21)


@pytest.mark.gpu
def test_keccak_table_trace(gpu, room):
    """3 inputs in 128 rows: a permutation across the wave boundary at row 64; 2430 columns"""
    import test_gpu_keccak_table as tkt

    count, n = 3, 128
    exp = tkt._reference_trace(count, n)
    d_in = _dev(gpu, tkt._pool()[:count])
    t = _table_trace(room, tkt.COLUMNS, n)
    try:
        _L().call("gl_keccak_table_trace", d_in.ptr, count, 7, t.ptr, t.stride, gpu.ptr)
        got = t.read("the trace")
    finally:
        t.free()
    assert (d_in.download().reshape(count, 25) == tkt._pool()[:count]).all()
    assert _first_difference(got, exp) is None, _first_difference(got, exp)


@pytest.mark.gpu
def test_memory_table_trace(gpu, room):
    """65 mixed operations with dummies of both kinds, from unsorted records; 26 columns"""
    import test_gpu_memory_table as tmt

    exp, exp_rows = tmt._reference("mixed", 65)
    n = exp.shape[1]
    assert n == 128
    d_ops, scratch = _dev(gpu, tmt._ops("mixed", 65)), tmt._scratch(gpu, 65, 7)
    t = _table_trace(room, tmt.COLUMNS, n)
    try:
        rows, err = tmt._call(gpu, d_ops.ptr, 65, 7, t.ptr, t.stride, scratch.ptr)
        assert err is None and rows == exp_rows
        got = t.read("the trace")
    finally:
        t.free()
    assert (d_ops.download().reshape(65, 14) == tmt._ops("mixed", 65)).all()
    assert _first_difference(got, exp) is None, _first_difference(got, exp)


@pytest.mark.gpu
def test_logic_table_trace(gpu, room):
    """65 operations (more than a wave) in 128 rows; 523 columns"""
    import test_gpu_logic_table as tlt

    exp = tlt._reference(65, 7)
    d_ops, scratch = _dev(gpu, tlt._ops(65)), _pg().DeviceBuffer(gpu, 2)
    t = _table_trace(room, tlt.COLUMNS, 128)
    try:
        assert tlt._call(gpu, d_ops.ptr, 65, 7, t.ptr, t.stride, scratch.ptr) is None
        got = t.read("the trace")
    finally:
        t.free()
    assert (d_ops.download().reshape(65, 17) == tlt._ops(65)).all()
    assert _first_difference(got, exp) is None, _first_difference(got, exp)


@pytest.mark.gpu
def test_keccak_sponge_table_trace_and_ops(gpu, room):
    """the mixed list at its own height (2^5 rows), 414 columns; then gl_keccak_sponge_table_ops reads that far trace back into the
    three derived lists, and the trace is as it was"""
    import test_gpu_keccak_sponge_table as tks
    from plonky2_gpu_amd import keccak_sponge_table as ks

    name = "mixed"
    words, data = tks._words(name)
    bits = tks._exact_bits(name)
    assert bits == 5
    exp = tks._reference(name, bits)
    d_ops = _dev(gpu, words)
    d_bytes, bytes_ptr = ks.upload_bytes(gpu, data, 0)
    scratch = tks._scratch(gpu, len(words), bits)
    t = _table_trace(room, tks.COLUMNS, 1 << bits)
    try:
        rows, err = tks._call(gpu, d_ops.ptr, len(words), bytes_ptr, bits, t.ptr, t.stride, scratch.ptr)
        assert err is None and rows == tks.kr.rows_needed(tks._ops(name))
        got = t.read("the trace")
        assert _first_difference(got, exp) is None, _first_difference(got, exp)
        log = tks._log(name)
        lists = tks._derive(gpu, t.ptr, bits, t.stride, rows, [e.shape for e in log], (0, 1, 2))
        for k, (g, e) in enumerate(zip(lists, log)):
            assert _first_difference(g, e) is None, (k, _first_difference(g, e))
        assert (t.read("the trace behind gl_keccak_sponge_table_ops") == got).all()
    finally:
        t.free()
    assert (d_ops.download().reshape(len(words), 5) == words).all()
    assert (d_bytes.download().view(np.uint8)[: data.size] == data).all()


@pytest.mark.gpu
def test_arithmetic_table_trace(gpu, room):
    """mixed(65): one- and two-row operators interleaved; 92 columns"""
    import test_gpu_arithmetic_table as tat

    w, exp = tat._ops("mixed", 65), tat._reference("mixed", 65)
    rows = tat.ar.num_rows(w)
    bits = tat._bits(rows)
    assert exp.shape == (tat.COLUMNS, 1 << bits) and bits == 7
    d_ops, scratch = _dev(gpu, w), tat._scratch(gpu, len(w), bits)
    t = _table_trace(room, tat.COLUMNS, 1 << bits)
    try:
        err, got_rows = tat._call(gpu, d_ops.ptr, len(w), bits, t.ptr, t.stride, scratch.ptr)
        assert err is None and got_rows == rows
        got = t.read("the trace")
    finally:
        t.free()
    assert (d_ops.download().reshape(-1, tat.W) == w).all()
    assert _first_difference(got, exp) is None, _first_difference(got, exp)
