"""Keccak Merkle trees and commits (plonky2's KeccakGoldilocksConfig: csrc/keccak.hip, the `_h` entry points of
include/plonky2_hip.h), bit-exact against tests/keccak_ref.py — the numpy Keccak that tests/test_keccak_ref.py pins against
hashlib and the published values. What does not depend on the hasher (d_lde, d_leaves, the coefficients) is held against the
existing Poseidon commit on the same input."""
import os
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import keccak_ref as kr  # noqa: E402
import representatives as rp  # noqa: E402
from test_keccak_ref import FIELD_ANSWERS, TWO_TO_ONE_ZEROS  # noqa: E402

pytestmark = pytest.mark.gpu
P = kr.P
POSEIDON, KECCAK = 0, 1


@pytest.fixture(scope="module")
def gpu():
    import plonky2_gpu_amd as pg

    ctx = pg.Context(0)
    yield ctx
    ctx.close()


def _buf(ctx, arr_or_size):
    """a device buffer of at least one word (a zero-sized allocation has no address)"""
    import plonky2_gpu_amd as pg

    if isinstance(arr_or_size, (int, np.integer)):
        return pg.DeviceBuffer(ctx, max(int(arr_or_size), 1))
    a = np.ascontiguousarray(arr_or_size, dtype=np.uint64)
    b = pg.DeviceBuffer(ctx, max(a.size, 1))
    b.upload(a)
    return b


def _hash_batch(ctx, inputs, length, stride, count):
    from plonky2_gpu_amd import _lib

    d_in, d_out = _buf(ctx, inputs), _buf(ctx, 4 * count)
    _lib.call("gl_keccak_hash_no_pad_batch", d_in.ptr, length, stride, count, d_out.ptr, ctx.ptr)
    out = d_out.download(0, 4 * count).reshape(count, 4)
    d_in.free()
    d_out.free()
    return out


def _mixed_words(rng, shape):
    """canonical data with edge values, about half of the liftable entries as their second representative x + p, and a few raw
    words from the top of the u64 range"""
    a, _ = rp.lift(rp.field_data(rng, shape), rng)
    if a.size:
        flat = a.reshape(-1)
        k = max(1, flat.size // 50)
        flat[rng.integers(0, flat.size, size=k)] = rng.integers(P, 2**64, size=k, dtype=np.uint64)
    return a


def _n_digest_slots(n, h):
    return 2 * (n - (1 << h))


# ---- gl_keccak_hash_no_pad_batch ------------------------------------------------------------------------------------------------

def test_hash_no_pad_known_answers(gpu):
    for x, answer in FIELD_ANSWERS:
        got = _hash_batch(gpu, np.array(x, dtype=np.uint64), len(x), len(x), 1)
        assert kr.hash_bytes(got)[0].tobytes().hex() == answer, x
    a = _hash_batch(gpu, np.array([P + 5, 2**64 - 1, P, 1, 2], dtype=np.uint64), 5, 5, 1)
    b = _hash_batch(gpu, np.array([5, 2**32 - 2, 0, 1, 2], dtype=np.uint64), 5, 5, 1)
    assert (a == b).all()


@pytest.mark.parametrize("length", list(range(41)) + [135, 136, 137, 272])
def test_hash_no_pad_every_length_random_and_non_canonical(gpu, length):
    rng = np.random.default_rng(7000 + length)
    count, stride = 65, length + 3  # a padded stride: the words between the inputs are not read
    for data in (rng.integers(0, P, size=(count, stride), dtype=np.uint64), _mixed_words(rng, (count, stride))):
        got = _hash_batch(gpu, data, length, stride, count)
        exp = kr.slots(kr.hash_no_pad(data[:, :length]))
        assert (got == exp).all()
        data2 = data.copy()
        data2[:, length:] ^= np.uint64(0x5555)  # the padding words do not matter
        assert (_hash_batch(gpu, data2, length, stride, count) == exp).all()


@pytest.mark.parametrize("count", [1, 63, 65, 4097])
def test_hash_no_pad_counts(gpu, count):
    rng = np.random.default_rng(7100 + count)
    for length in (5, 20, 34):
        data = _mixed_words(rng, (count, length))
        assert (_hash_batch(gpu, data, length, length, count) == kr.slots(kr.hash_no_pad(data))).all()


def test_hash_no_pad_refusals(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    d = _buf(gpu, np.arange(64, dtype=np.uint64))
    out = _buf(gpu, np.full(64, 0xABCD, dtype=np.uint64))
    for args in [(None, 5, 5, 2, out.ptr, gpu.ptr), (d.ptr, 5, 5, 2, None, gpu.ptr), (d.ptr, 5, 4, 2, out.ptr, gpu.ptr),
                 (d.ptr, 5, 5, 2, out.ptr, None)]:
        with pytest.raises(pg.Plonky2HipError) as e:
            _lib.call("gl_keccak_hash_no_pad_batch", *args)
        assert e.value.code == pg.GL_E_INVALID
    _lib.call("gl_keccak_hash_no_pad_batch", d.ptr, 5, 5, 0, out.ptr, gpu.ptr)  # nothing to do
    assert (out.download() == 0xABCD).all()
    _lib.call("gl_keccak_hash_no_pad_batch", None, 0, 0, 3, out.ptr, gpu.ptr)  # three hashes of the empty message
    assert (out.download(0, 12).reshape(3, 4) == kr.slots(kr.hash_no_pad(np.zeros((3, 0), dtype=np.uint64)))).all()


# ---- trees ---------------------------------------------------------------------------------------------------------------------

def _trees_both_ways(ctx, leaves, h, col_stride):
    """(digests, cap) as slot words from gl_merkle_tree_from_columns_h and from gl_merkle_tree_from_leaves_h"""
    from plonky2_gpu_amd import _lib

    n, k = leaves.shape
    nd = _n_digest_slots(n, h)
    cols = np.full((k, col_stride), 0xDEAD0000DEAD, dtype=np.uint64)
    cols[:, :n] = leaves.T
    res = []
    for from_columns in (True, False):
        d_in = _buf(ctx, cols if from_columns else leaves)
        d_dig, d_cap = _buf(ctx, np.full(4 * nd + 4, 0x1111, dtype=np.uint64)), _buf(ctx, 4 << h)
        if from_columns:
            _lib.call("gl_merkle_tree_from_columns_h", KECCAK, d_in.ptr, k, n, col_stride, h, d_dig.ptr, d_cap.ptr, ctx.ptr)
        else:
            _lib.call("gl_merkle_tree_from_leaves_h", KECCAK, d_in.ptr, k, n, h, d_dig.ptr, d_cap.ptr, ctx.ptr)
        dig = d_dig.download()
        assert (dig[4 * nd:] == 0x1111).all(), "written past the digest array"
        res.append((dig[: 4 * nd].reshape(nd, 4), d_cap.download(0, 4 << h).reshape(-1, 4)))
        for b in (d_in, d_dig, d_cap):
            b.free()
    return res


def _check_tree(ctx, leaves, h, col_stride):
    exp_d, exp_c = kr.merkle_tree(leaves, h)
    (dig_c, cap_c), (dig_r, cap_r) = _trees_both_ways(ctx, leaves, h, col_stride)
    assert (dig_c == dig_r).all() and (cap_c == cap_r).all(), "the two entry points differ"
    # hash_bytes asserts that bytes 25..31 of every slot are zero
    assert (kr.hash_bytes(cap_c) == exp_c).all()
    assert dig_c.shape[0] == exp_d.shape[0] and (kr.hash_bytes(dig_c) == exp_d).all()
    assert (dig_c == kr.slots(exp_d)).all() and (cap_c == kr.slots(exp_c)).all()


def test_two_to_one_known_answer(gpu):
    """two empty leaves are two hashes of 25 zero bytes (hash_or_noop); their parent is the pinned two_to_one(0^25, 0^25)"""
    (dig, cap), _ = _trees_both_ways(gpu, np.zeros((2, 0), dtype=np.uint64), 0, 2)
    assert not dig.any() and kr.hash_bytes(cap)[0].tobytes().hex() == TWO_TO_ONE_ZEROS


# the (n, leaf_len, cap_height) list of tests/test_gpu_merkle.py::test_merkle_tree_matches_oracle; its leaf_len == 4 entry is a
# refusal case here (test_leaves_of_four_elements_and_unknown_hashers_are_refused)
MERKLE_SHAPES = [(256, 7, 1), (256, 7, 8), (256, 7, 0), (2, 5, 1), (1, 9, 0), (16, 4, 2), (16, 3, 0), (8, 1, 1), (64, 8, 3), (64, 9, 3),
                 (32, 16, 2), (128, 135, 4), (4096, 20, 4), (1024, 88, 10), (512, 17, 5)]


@pytest.mark.parametrize("n,k,h", [s for s in MERKLE_SHAPES if s[1] != 4])
def test_merkle_tree_matches_reference(gpu, n, k, h):
    rng = np.random.default_rng(n * 131 + k * 7 + h)
    leaves = _mixed_words(rng, (n, k))
    leaves[0, 0] = np.uint64(2**64 - 1)
    for col_stride in (n, n + 1, n + 6):
        _check_tree(gpu, leaves, h, col_stride)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 16, 17, 18, 34])
def test_merkle_tree_leaf_lengths_cap_heights_and_column_pitches(gpu, k):
    n = 16
    rng = np.random.default_rng(8000 + k)
    leaves = _mixed_words(rng, (n, k))
    for h in range(5):  # h = 4 = log2(n): the cap is the leaf hashes, the digest array is empty
        for col_stride in (n, n + 1, n + 6):
            _check_tree(gpu, leaves, h, col_stride)


@pytest.mark.parametrize("n,k,h", [s for s in MERKLE_SHAPES if s[1] == 4] + [(1, 4, 0), (64, 4, 6)])
def test_leaves_of_four_elements_and_unknown_hashers_are_refused(gpu, n, k, h):
    """KeccakHash<25>::hash_or_noop panics for 4 elements (plonk/config.rs:58-63): GL_E_INVALID and nothing written; the same
    for a hasher value the header does not define"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    rng = np.random.default_rng(n + h)
    nd = _n_digest_slots(n, h)
    for hasher, kk in ((KECCAK, k), (2, 5), (0xFFFFFFFF, 5)):
        leaves = rng.integers(0, P, size=(n, kk), dtype=np.uint64)
        d_in = _buf(gpu, leaves)
        pat_d, pat_c = np.full(4 * nd + 4, 0x7777, dtype=np.uint64), np.full(4 << h, 0x9999, dtype=np.uint64)
        d_dig, d_cap = _buf(gpu, pat_d), _buf(gpu, pat_c)
        for name, args in (("gl_merkle_tree_from_columns_h", (hasher, d_in.ptr, kk, n, n, h, d_dig.ptr, d_cap.ptr, gpu.ptr)),
                           ("gl_merkle_tree_from_leaves_h", (hasher, d_in.ptr, kk, n, h, d_dig.ptr, d_cap.ptr, gpu.ptr))):
            with pytest.raises(pg.Plonky2HipError) as e:
                _lib.call(name, *args)
            assert e.value.code == pg.GL_E_INVALID
        gpu.synchronize()
        assert (d_dig.download() == pat_d).all() and (d_cap.download() == pat_c).all()
        assert (d_in.download(0, leaves.size) == leaves.reshape(-1)).all()
        for b in (d_in, d_dig, d_cap):
            b.free()


def test_commits_refuse_four_element_leaves_unknown_hashers_and_bad_shapes(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    log_n, rate_bits, h = 5, 1, 2
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    rng = np.random.default_rng(99)
    # (hasher, poly_num, salt_size, cap_height)
    for hasher, polys, salt, cap_h in ((KECCAK, 4, 0, h), (KECCAK, 0, 4, h), (5, 3, 0, h), (KECCAK, 3, 0, log_n + rate_bits + 1)):
        vals = rng.integers(0, P, size=(max(polys, 1), n), dtype=np.uint64)
        pat = np.full((polys + salt) * n_ext, 0x4242, dtype=np.uint64)
        for name in ("gl_commit_from_values_h", "gl_commit_from_coeffs_h"):
            d_v, d_lde, d_lv = _buf(gpu, vals), _buf(gpu, pat), _buf(gpu, pat)
            d_dig, d_cap = _buf(gpu, np.full(8 * n_ext, 0x4242, dtype=np.uint64)), _buf(gpu, np.full(4 << min(cap_h, 7), 0x4242, dtype=np.uint64))
            with pytest.raises(pg.Plonky2HipError) as e:
                _lib.call(name, hasher, d_v.ptr, polys, log_n, rate_bits, cap_h, salt, 7, d_lde.ptr, d_lv.ptr, d_dig.ptr, d_cap.ptr, gpu.ptr)
            assert e.value.code == pg.GL_E_INVALID
            gpu.synchronize()
            assert (d_v.download(0, vals.size) == vals.reshape(-1)).all(), "a refused commit transformed its input"
            for b in (d_lde, d_lv, d_dig, d_cap):
                assert (b.download() == 0x4242).all()
                b.free()
            d_v.free()
    with pytest.raises(ValueError):
        pg.MerkleTree.new(gpu, np.zeros((4, 5), dtype=np.uint64), 0, hasher="blake")


NULL_POINTER = "null pointer"
UNKNOWN_HASHER = "unknown hasher"
CAP_TOO_HIGH = "cap_height should be at most log2(leaves.len())"
LOG_N_TOO_BIG = "log_n > 24 is not supported by this build"
KECCAK_LEAF_LEN_4 = "KeccakHash<25>::hash_or_noop is undefined for leaves of 4 elements (plonk/config.rs:58-63 panics)"


def _refused(name, args, message):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    with pytest.raises(pg.Plonky2HipError) as e:
        _lib.call(name, *args)
    assert e.value.code == pg.GL_E_INVALID
    assert str(e.value) == "plonky2_hip error %d: %s" % (pg.GL_E_INVALID, message), name


# (entry point, hasher); None: the un-suffixed entry point, which takes no hasher and commits with Poseidon
@pytest.mark.parametrize("name,hasher", [("gl_commit_from_coeffs", None), ("gl_commit_from_values", None)] +
                         [(n, h) for n in ("gl_commit_from_coeffs_h", "gl_commit_from_values_h") for h in (POSEIDON, KECCAK)])
def test_each_refusal_of_a_commit_has_its_message(gpu, name, hasher):
    """one broken rule per call, on the tiny shape of the test above: GL_E_INVALID with the message of that rule, the same for
    every entry point and hasher that has the rule. A null d_digests is what the hashers treat differently: Poseidon refuses it
    always, Keccak takes it exactly when the tree is all cap (cap_height == log_n + rate_bits)."""
    from plonky2_gpu_amd import _lib

    log_n, rate_bits, h, polys = 5, 1, 2, 3
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    vals = np.random.default_rng(7).integers(0, P, size=(polys, n), dtype=np.uint64)
    bufs = dict(d_in=_buf(gpu, vals), d_lde=_buf(gpu, polys * n_ext), d_lv=_buf(gpu, polys * n_ext), d_dig=_buf(gpu, 8 * n_ext),
                d_cap=_buf(gpu, 4 * n_ext))

    def args(hasher=hasher, polys=polys, log_n=log_n, cap_h=h, salt=0, **null):
        p = {k: (None if k in null else b.ptr) for k, b in bufs.items()}
        a = (p["d_in"], polys, log_n, rate_bits, cap_h, salt, 7, p["d_lde"], p["d_lv"], p["d_dig"], p["d_cap"], gpu.ptr)
        return a if name[-2:] != "_h" else (hasher,) + a

    _refused(name, args(d_lde=None), NULL_POINTER)
    _refused(name, args(d_cap=None), NULL_POINTER)
    _refused(name, args(d_dig=None), NULL_POINTER)
    if hasher == KECCAK:
        bufs["d_in"].upload(vals)
        _lib.call(name, *args(cap_h=log_n + rate_bits, d_dig=None))
        cap_without = bufs["d_cap"].download(0, 4 * n_ext)
        bufs["d_in"].upload(vals)
        _lib.call(name, *args(cap_h=log_n + rate_bits))
        assert (bufs["d_cap"].download(0, 4 * n_ext) == cap_without).all()
    else:
        _refused(name, args(cap_h=log_n + rate_bits, d_dig=None), NULL_POINTER)
    _refused(name, args(polys=0), "bad poly_num")
    _refused(name, args(log_n=25), LOG_N_TOO_BIG)
    _refused(name, args(cap_h=log_n + rate_bits + 1), CAP_TOO_HIGH)
    if name[-2:] == "_h":
        _refused(name, args(hasher=5), UNKNOWN_HASHER)
    if hasher == KECCAK:
        _refused(name, args(polys=0, salt=4), KECCAK_LEAF_LEN_4)
    gpu.synchronize()
    for b in bufs.values():
        b.free()


@pytest.mark.parametrize("name,hasher", [("gl_merkle_tree_from_columns", None), ("gl_merkle_tree_from_leaves", None)] +
                         [(n, h) for n in ("gl_merkle_tree_from_columns_h", "gl_merkle_tree_from_leaves_h") for h in (POSEIDON, KECCAK)])
def test_each_refusal_of_a_tree_has_its_message(gpu, name, hasher):
    """the same for the four tree entry points. Only Keccak checks d_digests (refused when a layer lies below the cap); a tree
    that is all cap takes a null d_digests with either hasher."""
    from plonky2_gpu_amd import _lib

    n, k, h = 16, 5, 2
    columns = "columns" in name
    leaves = np.random.default_rng(8).integers(0, P, size=(n, k), dtype=np.uint64)
    bufs = dict(d_in=_buf(gpu, leaves), d_dig=_buf(gpu, 4 * _n_digest_slots(n, h)), d_cap=_buf(gpu, 4 * n))

    def args(hasher=hasher, k=k, n=n, col_stride=n, cap_h=h, **null):
        p = {key: (None if key in null else b.ptr) for key, b in bufs.items()}
        a = (p["d_in"], k, n) + ((col_stride,) if columns else ()) + (cap_h, p["d_dig"], p["d_cap"], gpu.ptr)
        return a if name[-2:] != "_h" else (hasher,) + a

    _refused(name, args(d_in=None), NULL_POINTER)
    _refused(name, args(d_cap=None), NULL_POINTER)
    if hasher == KECCAK:
        _refused(name, args(d_dig=None), NULL_POINTER)
    _lib.call(name, *args(cap_h=4, d_dig=None))
    cap_without = bufs["d_cap"].download(0, 4 * n)
    _lib.call(name, *args(cap_h=4))
    assert (bufs["d_cap"].download(0, 4 * n) == cap_without).all()
    _refused(name, args(n=3, cap_h=1), "n_leaves must be a power of two")
    _refused(name, args(cap_h=5), CAP_TOO_HIGH)
    if columns:
        _refused(name, args(col_stride=n - 1), "col_stride smaller than n_leaves: the columns would overlap")
    if name[-2:] == "_h":
        _refused(name, args(hasher=5), UNKNOWN_HASHER)
    if hasher == KECCAK:
        _refused(name, args(k=4), KECCAK_LEAF_LEN_4)
    gpu.synchronize()
    for b in bufs.values():
        b.free()


# ---- openings ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_n,k,h,which", [(10, 7, 2, "all"), (16, 20, 4, "random")])
def test_openings_of_a_keccak_tree_verify_to_the_cap(gpu, log_n, k, h, which):
    """gl_merkle_open_batch on a Keccak tree (unchanged code: a digest is one slot whatever the hasher): every path recomputed to
    the cap with the reference (verify_merkle_proof_to_cap, hash/merkle_proofs.rs:57-86)"""
    import plonky2_gpu_amd as pg

    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    leaves = _mixed_words(rng, (n, k))
    tree = pg.MerkleTree.new(gpu, leaves, h, hasher="keccak")
    idx = np.arange(n) if which == "all" else rng.integers(0, n, size=256)
    got_leaves, sib = tree.open_batch(idx)
    assert (got_leaves == leaves[idx]).all()
    layers = log_n - h
    assert sib.shape == (idx.size, layers, 4)
    cap = tree.cap_bytes()
    assert cap.shape == (1 << h, 25) and tree.digest_bytes().shape == (_n_digest_slots(n, h), 25)
    ok = kr.merkle_verify_batch(leaves[idx], idx, cap, kr.hash_bytes(sib))
    assert ok.all()
    # prove() reads the same slots one by one; a flipped sibling does not verify
    for i in (0, 1, n - 1, int(idx[-1])):
        assert (tree.prove(i) == tree.open_batch([i])[1][0]).all()
        assert kr.merkle_verify(leaves[i], i, cap, kr.hash_bytes(tree.prove(i)))
    bad = kr.hash_bytes(sib[:1]).copy()
    bad[0, layers - 1, 24] ^= 0x80
    assert not kr.merkle_verify_batch(leaves[idx[:1]], idx[:1], cap, bad).any()
    if which == "all":
        exp_d, exp_c = kr.merkle_tree(leaves, h)
        assert (tree.digest_bytes() == exp_d).all() and (cap == exp_c).all()


# ---- commits -------------------------------------------------------------------------------------------------------------------

def _commit(ctx, name, hasher, vals, log_n, rate_bits, h, salt, leaves_mode):
    """one commit through `name` (`hasher` None: the un-suffixed entry point); returns the host copies of everything it wrote.
    leaves_mode: "null" | "separate" | "alias" (d_leaves = d_coeffs: one region of (P+S) * n_ext words, the input at its start)"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    polys = vals.shape[0]
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    salt_size = 0 if salt is None else salt.shape[0]
    cols = polys + salt_size
    nd = _n_digest_slots(n_ext, h)
    d_lde = pg.DeviceBuffer(ctx, cols * n_ext)
    if salt_size:
        d_lde.upload(salt, offset=polys * n_ext)
    if leaves_mode == "alias":
        d_in = pg.DeviceBuffer(ctx, cols * n_ext)
        d_in.upload(vals)
        d_leaves, leaves_ptr = d_in, d_in.ptr
    else:
        d_in = pg.DeviceBuffer.from_host(ctx, vals)
        d_leaves = pg.DeviceBuffer(ctx, cols * n_ext) if leaves_mode == "separate" else None
        leaves_ptr = d_leaves.ptr if d_leaves else None
    d_dig, d_cap = _buf(ctx, 4 * nd), _buf(ctx, 4 << h)
    args = (d_in.ptr, polys, log_n, rate_bits, h, salt_size, 7, d_lde.ptr, leaves_ptr, d_dig.ptr, d_cap.ptr, ctx.ptr)
    _lib.call(name, *(args if hasher is None else (hasher,) + args))
    ctx.synchronize()
    out = {"lde": d_lde.download().reshape(cols, n_ext), "digests": d_dig.download(0, 4 * nd).reshape(nd, 4),
           "cap": d_cap.download(0, 4 << h).reshape(-1, 4)}
    if leaves_mode != "alias":
        out["coeffs"] = d_in.download().reshape(polys, n)
    if leaves_mode != "null":
        out["leaves"] = d_leaves.download(0, cols * n_ext).reshape(n_ext, cols)
    for b in {id(b): b for b in (d_lde, d_in, d_leaves, d_dig, d_cap) if b is not None}.values():
        b.free()
    return out


# (log_n, columns, rate_bits, cap_height, salt_size, d_leaves, entry): rows 2^4 .. 2^14 each once or more, every column count, rate,
# cap height and salt size, every d_leaves mode with and without salt, both entry points; the largest (2^17 leaves of 135 columns)
# is still held against the whole numpy tree
COMMIT_CASES = [(4, 1, 1, 0, 0, "null", "values"), (5, 3, 2, 4, 4, "separate", "coeffs"), (6, 20, 3, 0, 0, "alias", "values"),
                (7, 135, 1, 4, 4, "alias", "coeffs"), (8, 1, 2, 4, 4, "null", "values"), (9, 3, 3, 0, 0, "separate", "values"),
                (10, 20, 1, 4, 4, "separate", "values"), (11, 135, 2, 0, 0, "null", "coeffs"), (12, 3, 3, 4, 0, "alias", "coeffs"),
                (13, 20, 2, 0, 4, "null", "coeffs"), (14, 135, 3, 4, 0, "separate", "values"), (14, 1, 1, 4, 4, "alias", "values")]


@pytest.mark.parametrize("log_n,polys,rate_bits,h,salt_size,leaves_mode,entry", COMMIT_CASES)
def test_commit_matches_the_poseidon_commit_and_the_reference_tree(gpu, log_n, polys, rate_bits, h, salt_size, leaves_mode, entry):
    rng = np.random.default_rng(log_n * 1000 + polys)
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    vals = _mixed_words(rng, (polys, n))
    salt = None
    if salt_size:
        salt, lifted = rp.lift(rp.field_data(rng, (salt_size, n_ext)), rng)
        assert lifted > 0
    name = "gl_commit_from_" + entry
    base = _commit(gpu, name, None, vals, log_n, rate_bits, h, salt, leaves_mode)
    got = _commit(gpu, name + "_h", KECCAK, vals, log_n, rate_bits, h, salt, leaves_mode)
    # hasher-independent outputs, word for word
    assert (got["lde"] == base["lde"]).all() and rp.all_canonical(got["lde"])
    if salt_size:
        assert (got["lde"][polys:] == kr.canon(salt)).all()
    if "coeffs" in base:
        assert (got["coeffs"] == base["coeffs"]).all()
    if "leaves" in base:
        assert (got["leaves"] == base["leaves"]).all() and (got["leaves"] == got["lde"].T).all()
    # the tree over that LDE
    t0 = time.perf_counter()
    exp_d, exp_c = kr.merkle_tree(np.ascontiguousarray(got["lde"].T), h)
    print("reference tree over %d leaves of %d: %.1f s" % (n_ext, polys + salt_size, time.perf_counter() - t0))
    assert (got["cap"] == kr.slots(exp_c)).all()
    assert (got["digests"] == kr.slots(exp_d)).all()
    # and the same commit through the operator mirror
    import plonky2_gpu_amd as pg

    ctor = pg.PolynomialBatch.from_values if entry == "values" else pg.PolynomialBatch.from_coeffs
    batch = ctor(gpu, vals, rate_bits, bool(salt_size), h, salt=salt, leaf_major=leaves_mode != "null", hasher="keccak")
    assert (batch.merkle_tree.cap_bytes() == exp_c).all()
    if log_n <= 10:
        assert (batch.merkle_tree.digest_bytes() == exp_d).all()
        assert (batch.get_lde_values(3) == got["lde"][:polys, int(f"{3:0{log_n + rate_bits}b}"[::-1], 2)]).all()


def test_poseidon_through_the_h_entry_points_is_the_unsuffixed_call(gpu):
    from plonky2_gpu_amd import _lib

    rng = np.random.default_rng(5)
    # trees
    n, k, h = 256, 7, 2
    leaves = _mixed_words(rng, (n, k))
    nd = _n_digest_slots(n, h)
    outs = []
    for suffix in (False, True):
        for from_columns in (True, False):
            d_in = _buf(gpu, np.ascontiguousarray(leaves.T) if from_columns else leaves)
            d_dig, d_cap = _buf(gpu, 4 * nd), _buf(gpu, 4 << h)
            name = "gl_merkle_tree_from_columns" if from_columns else "gl_merkle_tree_from_leaves"
            args = (d_in.ptr, k, n, n, h, d_dig.ptr, d_cap.ptr, gpu.ptr) if from_columns else (d_in.ptr, k, n, h, d_dig.ptr, d_cap.ptr, gpu.ptr)
            _lib.call(name + "_h" if suffix else name, *((POSEIDON,) + args if suffix else args))
            outs.append((d_dig.download(), d_cap.download()))
            for b in (d_in, d_dig, d_cap):
                b.free()
    for d, c in outs[1:]:
        assert (d == outs[0][0]).all() and (c == outs[0][1]).all()
    assert rp.all_canonical(outs[0][0])  # four field elements per digest: a Poseidon tree, not 25 bytes and zeros
    assert (outs[0][0].reshape(-1, 4)[:, 3] > 255).any()
    # commits: a small one and one that takes the pipelined path of the Poseidon commit
    for log_n, polys, rate_bits, ch, salt_size, mode in ((6, 5, 3, 2, 4, "separate"), (13, 50, 3, 4, 0, "alias"), (13, 50, 3, 4, 4, "null")):
        vals = _mixed_words(rng, (polys, 1 << log_n))
        salt = rp.lift(rp.field_data(rng, (salt_size, 1 << (log_n + rate_bits))), rng)[0] if salt_size else None
        for entry in ("values", "coeffs"):
            a = _commit(gpu, "gl_commit_from_" + entry, None, vals, log_n, rate_bits, ch, salt, mode)
            b = _commit(gpu, "gl_commit_from_" + entry + "_h", POSEIDON, vals, log_n, rate_bits, ch, salt, mode)
            assert a.keys() == b.keys()
            for key in a:
                assert (a[key] == b[key]).all(), key


def test_commit_at_the_size_users_run(gpu):
    """2^20 rows x 135 columns, rate 8 (rate_bits 3), cap height 4: 2^23 leaves — too many for the numpy tree. 256 random openings
    verified to the cap with the reference, the top 8 layers of the digest array (and the cap) recomputed from the layer below
    them, and ten columns of d_lde compared with the Poseidon commit's."""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    log_n, polys, rate_bits, h = 20, 135, 3, 4
    n, log_ext = 1 << log_n, log_n + rate_bits
    n_ext = 1 << log_ext
    rng = np.random.default_rng(2023)
    vals = rng.integers(0, P, size=(polys, n), dtype=np.uint64)
    nd = _n_digest_slots(n_ext, h)
    d_vals, d_work = pg.DeviceBuffer.from_host(gpu, vals), pg.DeviceBuffer(gpu, polys * n)
    d_lde, d_dig, d_cap = pg.DeviceBuffer(gpu, polys * n_ext), pg.DeviceBuffer(gpu, 4 * nd), pg.DeviceBuffer(gpu, 4 << h)
    del vals
    _lib.call("gl_memcpy_d2d", d_work.ptr, d_vals.ptr, polys * n * 8, gpu.ptr)
    _lib.call("gl_commit_from_values_h", KECCAK, d_work.ptr, polys, log_n, rate_bits, h, 0, 7, d_lde.ptr, None, d_dig.ptr, d_cap.ptr, gpu.ptr)
    gpu.synchronize()
    tree = pg.MerkleTree(gpu, n_ext, polys, h, d_dig, d_cap, None, d_lde, n_ext, hasher="keccak")
    cap = tree.cap_bytes()
    # openings from the column-major LDE
    idx = np.concatenate([[0, n_ext - 1], rng.integers(0, n_ext, size=254)])
    leaves, sib = tree.open_batch(idx)
    assert kr.merkle_verify_batch(leaves, idx, cap, kr.hash_bytes(sib)).all()
    # the upper layers: node i of layer L of subtree s sits at slot s * sub_slots + digest_slot(i, L)
    dig = tree.digest_bytes()
    log_sub = log_ext - h
    sub_slots = 2 * ((1 << log_sub) - 1)

    def layer(L):
        i = np.arange(1 << (log_sub - L))
        slot = 2 * (((i >> 1) << (L + 1)) + (1 << L) - 1) + (i & 1)
        return dig[(np.arange(1 << h)[:, None] * sub_slots + slot[None, :]).reshape(-1)]

    for L in range(log_sub - 8, log_sub):
        below = layer(L)
        above = cap if L + 1 == log_sub else layer(L + 1)
        assert (kr.two_to_one(below[0::2], below[1::2]) == above).all(), L
    # the first layer above the leaves on a sample: parents of the opened leaves
    l0 = layer(0)
    pairs = np.unique(idx >> 1)
    assert (kr.two_to_one(l0[2 * pairs], l0[2 * pairs + 1]) == layer(1)[pairs]).all()
    assert (l0[idx] == kr.hash_no_pad(leaves)).all()
    # d_lde does not depend on the hasher
    columns = sorted(set([0, polys - 1] + [int(c) for c in rng.choice(np.arange(1, polys - 1), size=8, replace=False)]))
    mine = [d_lde.download(c * n_ext, n_ext) for c in columns]
    _lib.call("gl_memcpy_d2d", d_work.ptr, d_vals.ptr, polys * n * 8, gpu.ptr)
    _lib.call("gl_commit_from_values", d_work.ptr, polys, log_n, rate_bits, h, 0, 7, d_lde.ptr, None, d_dig.ptr, d_cap.ptr, gpu.ptr)
    gpu.synchronize()
    for c, col in zip(columns, mine):
        assert (d_lde.download(c * n_ext, n_ext) == col).all(), c
    for b in (d_vals, d_work, d_lde, d_dig, d_cap):
        b.free()


def test_two_contexts_commit_with_different_hashers_at_once(gpu):
    """two host threads, each with its own context, one committing with Poseidon and one with Keccak: what each gives alone"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    log_n, polys, rate_bits, h = 14, 50, 3, 4
    n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
    nd = _n_digest_slots(n_ext, h)
    rng = np.random.default_rng(77)
    vals = rng.integers(0, P, size=(polys, n), dtype=np.uint64)
    other = pg.Context(0)
    try:
        bufs = {}
        for ctx in (gpu, other):
            bufs[ctx] = dict(vals=pg.DeviceBuffer.from_host(ctx, vals), work=pg.DeviceBuffer(ctx, polys * n), lde=pg.DeviceBuffer(ctx, polys * n_ext),
                             leaves=pg.DeviceBuffer(ctx, polys * n_ext), dig=pg.DeviceBuffer(ctx, 4 * nd), cap=pg.DeviceBuffer(ctx, 4 << h))

        def commit(ctx, hasher):
            b = bufs[ctx]
            _lib.call("gl_memcpy_d2d", b["work"].ptr, b["vals"].ptr, polys * n * 8, ctx.ptr)
            _lib.call("gl_commit_from_values_h", hasher, b["work"].ptr, polys, log_n, rate_bits, h, 0, 7, b["lde"].ptr, b["leaves"].ptr,
                      b["dig"].ptr, b["cap"].ptr, ctx.ptr)
            ctx.synchronize()
            return b["dig"].download().copy(), b["cap"].download().copy(), b["leaves"].download(0, 4096).copy()

        alone = {POSEIDON: commit(gpu, POSEIDON), KECCAK: commit(other, KECCAK)}
        assert (alone[POSEIDON][1] != alone[KECCAK][1]).any()
        assert (kr.slots(kr.hash_no_pad(bufs[other]["lde"].download().reshape(polys, n_ext)[:, :16].T))
                == alone[KECCAK][0].reshape(-1, 4)[[2 * ((q << 1)) + p for q in range(8) for p in range(2)]]).all()
        got = {gpu: [], other: []}
        errors = []

        def work(ctx, hasher):
            try:
                for _ in range(8):
                    got[ctx].append(commit(ctx, hasher))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(gpu, POSEIDON)), threading.Thread(target=work, args=(other, KECCAK))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for ctx, hasher in ((gpu, POSEIDON), (other, KECCAK)):
            assert len(got[ctx]) == 8
            for g in got[ctx]:
                assert all((x == y).all() for x, y in zip(g, alone[hasher]))
        for d in bufs.values():
            for b in d.values():
                b.free()
    finally:
        other.close()
