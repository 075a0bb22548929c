"""The Keccak sponge table on the device: gl_keccak_sponge_table_trace against tests/keccak_sponge_table_ref.py's restatement of
generate_trace_rows on all 414 columns, its count and its refusals; gl_keccak_sponge_table_ops against the restatement of
keccak_sponge_log; the derived lists through the three neighbouring trace calls; the table proved by gl_stark_prove and, with the
tables it ties together, by gl_stark_tables_prove from device-built traces against tests/stark_ref.py and tests/ctl_ref.py, byte for
byte: there is no tolerance anywhere.

The shapes cross the edges of the kernels as built: lengths around one, two and three blocks (135: both padding bits in one byte),
no operation, 1, 3 and 64 operations (a wave of the chain kernel), 300 operations in 550 rows (more than one 256-thread workgroup of
either kernel), the exact height and one above it, tight, even and odd padded pitches, input bytes at odd addresses."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref as cr  # noqa: E402
import keccak_sponge_table_instances as ki  # noqa: E402
import keccak_sponge_table_ref as kr  # noqa: E402
import keccak_table_ref  # noqa: E402
import logic_table_ref  # noqa: E402
import memory_table_ref  # noqa: E402
import stark_instances as si  # noqa: E402
import table_harness as th  # noqa: E402
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from strided import Strided, filler  # noqa: E402

ONES = (1 << 64) - 1
HASHERS = th.HASHERS
COLUMNS = 414
LISTS = {"mixed": ki.mixed, "system": ki.system_ops, "none": lambda: [], "many1": lambda: ki.many(1), "many3": lambda: ki.many(3),
         "many34": lambda: ki.many(34), "many64": lambda: ki.many(64), "many300": lambda: ki.many(300)}
LISTS.update({"single%d" % length: (lambda length=length: ki.single(length)) for length in ki.LENGTHS})


# ---------------------------------------------------------------- instances and reference traces
@functools.lru_cache(maxsize=None)
def _ops(name):
    return tuple(LISTS[name]())


@functools.lru_cache(maxsize=None)
def _words(name):
    words, data = kr.ops_to_words(_ops(name))
    words.setflags(write=False)
    data.setflags(write=False)
    return words, data


def _exact_bits(name):
    return max(1, (max(kr.rows_needed(_ops(name)), 1) - 1).bit_length())


@functools.lru_cache(maxsize=None)
def _reference(name, degree_bits):
    """[414][2^degree_bits] columns; never changed"""
    cols = kr.trace_of_ops(_ops(name), degree_bits)
    assert cols.shape == (COLUMNS, 1 << degree_bits)
    cols.setflags(write=False)
    return cols


def _scratch(gpu, num_ops, degree_bits):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    size = _lib.load().gl_keccak_sponge_table_scratch_bytes(num_ops, degree_bits)
    assert size and size % 16 == 0
    return pg.DeviceBuffer(gpu, size // 8)


def _call(gpu, d_ops, num_ops, d_bytes, degree_bits, d_trace, stride, d_scratch):
    """gl_keccak_sponge_table_trace -> (rows, None or the error)"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    rows = ctypes.c_uint64(ONES)
    try:
        _lib.call("gl_keccak_sponge_table_trace", d_ops, num_ops, d_bytes, degree_bits, d_trace, stride, d_scratch, ctypes.byref(rows), gpu.ptr)
    except pg.Plonky2HipError as e:
        return int(rows.value), e
    return int(rows.value), None


def _run(gpu, name, degree_bits, pad=0, byte_offset=0):
    """the trace of list `name` in a buffer pre-filled with 0xFF bytes — an unwritten word shows — whose guards and pitch gaps hold
    sentinels that must survive; the records and the bytes are left as they were"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import keccak_sponge_table as ks

    words, data = _words(name)
    num_ops, n = len(words), 1 << degree_bits
    buf = Strided(gpu, np.full((COLUMNS, n), ONES, dtype=np.uint64), n + pad)
    d_ops = pg.DeviceBuffer.from_host(gpu, words) if num_ops else None
    d_bytes, bytes_ptr = ks.upload_bytes(gpu, data, byte_offset) if data.size else (None, None)
    assert bytes_ptr is None or bytes_ptr % 8 == byte_offset
    scratch = _scratch(gpu, num_ops, degree_bits)
    rows, err = _call(gpu, d_ops.ptr if d_ops else None, num_ops, bytes_ptr, degree_bits, buf.ptr, n + pad, scratch.ptr)
    assert err is None, err
    assert rows == kr.rows_needed(_ops(name))
    got = buf.polys((name, degree_bits, pad, byte_offset))
    buf.free()
    if d_ops:
        assert (d_ops.download().reshape(num_ops, 5) == words).all()
    if d_bytes:
        assert (d_bytes.download().view(np.uint8)[byte_offset : byte_offset + data.size] == data).all()
    return got


# ---------------------------------------------------------------- the trace
@pytest.mark.gpu
@pytest.mark.parametrize("length", ki.LENGTHS)
def test_one_operation_of_every_length(gpu, length):
    name = "single%d" % length
    bits = _exact_bits(name)
    assert 1 << bits == max(2, kr.next_power_of_two(length // 136 + 1))
    assert th.first_difference(_run(gpu, name, bits, byte_offset=length % 8), _reference(name, bits)) is None


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 24, 25])
@pytest.mark.parametrize("extra_bits", [0, 1])
@pytest.mark.parametrize("name", ["mixed", "none", "many1", "many3", "many64", "many300"])
def test_trace_equals_generate_trace_rows(gpu, name, extra_bits, pad):
    """the exact degree_bits and one above it (generate_trace_rows' min_rows), tight and padded pitches"""
    bits = _exact_bits(name) + extra_bits
    exp = _reference(name, bits)
    if extra_bits:
        half = 1 << (bits - 1)
        assert (exp[:, :half] == _reference(name, bits - 1)).all() and not exp[:, half:].any()
    assert th.first_difference(_run(gpu, name, bits, pad), exp) is None


@pytest.mark.gpu
@pytest.mark.parametrize("byte_offset", [1, 3, 7])
def test_bytes_at_an_odd_address(gpu, byte_offset):
    assert th.first_difference(_run(gpu, "mixed", 5, byte_offset=byte_offset), _reference("mixed", 5)) is None


@pytest.mark.gpu
def test_generate_trace_rows_and_derive_ops_of_the_module(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import keccak_sponge_table as ks

    ops = [(o.context, o.segment, o.virt, o.timestamp, o.input) for o in _ops("mixed")]
    d = ks.generate_trace(gpu, ops)  # the count first, then the smallest trace
    assert d.rows == 22 and th.first_difference(d.download().reshape(COLUMNS, 32), _reference("mixed", 5)) is None
    words, data = ks.ops_to_words(ops)
    assert ks.rows(gpu, words) == 22 == ks.rows(gpu, pg.DeviceBuffer.from_host(gpu, words))
    d = ks.generate_trace(gpu, pg.DeviceBuffer.from_host(gpu, words), data, degree_bits=6, trace_stride=64 + 24)
    assert th.first_difference(d.download().reshape(COLUMNS, 88)[:, :64], _reference("mixed", 6)) is None
    empty = ks.generate_trace(gpu, [])
    assert empty.rows == 0 and empty.n == 2 * COLUMNS and not empty.download().any()
    keccak, logic, memory = ks.derive_ops(gpu, d, 6, 22, trace_stride=88)  # the byte count read back from the trace
    exp = kr.log_of_ops(_ops("mixed"))
    for got, want in zip((keccak, logic, memory), exp):
        assert (got.download().reshape(want.shape) == want).all()


# ---------------------------------------------------------------- count and refusals
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "many300", "single0"])
def test_count_alone(gpu, name):
    import plonky2_gpu_amd as pg

    words, _ = _words(name)
    d_ops = pg.DeviceBuffer.from_host(gpu, words)
    scratch = _scratch(gpu, len(words), 1)  # for any number of operations at least as large as for none
    rows, err = _call(gpu, d_ops.ptr, len(words), None, 1, None, 0, scratch.ptr)
    assert err is None and rows == kr.rows_needed(_ops(name))
    rows, err = _call(gpu, None, 0, None, 1, None, 0, scratch.ptr)
    assert err is None and rows == 0


@pytest.mark.gpu
def test_data_refusals_write_nothing_and_name_the_lowest_record(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import keccak_sponge_table as ks

    words, data = _words("mixed")
    num_ops, n = len(words), 32
    fill = np.full(COLUMNS * n, ONES, dtype=np.uint64)
    trace = pg.DeviceBuffer.from_host(gpu, fill)
    d_bytes, bytes_ptr = ks.upload_bytes(gpu, data)
    scratch = _scratch(gpu, num_ops, 5)

    def refused(w, degree_bits=5, with_bytes=True):
        d_ops = pg.DeviceBuffer.from_host(gpu, w)
        rows, err = _call(gpu, d_ops.ptr, len(w), bytes_ptr if with_bytes else None, degree_bits, trace.ptr, 1 << degree_bits, scratch.ptr)
        assert err is not None and err.code == pg.GL_E_INVALID
        gpu.synchronize()
        assert (trace.download() == fill).all()
        return rows, str(err)

    rows, why = refused(words, degree_bits=4)  # 22 rows do not fit 16: the count is named and returned
    assert rows == 22 and " 22 rows" in why and "more than" in why
    w = words.copy()
    w[[9, 4], 3] = 1 << 32  # a timestamp
    rows, why = refused(w)
    assert rows == 0 and "a word of record 4 " in why and "2^32 or more" in why and "9" not in why
    w = words.copy()
    w[7, 4], w[3, 0] = ONES, 1 << 40  # a len of record 7, the context of record 3
    assert "a word of record 3 " in refused(w)[1]
    w = words.copy()
    w[6, 2], w[10, 2] = (1 << 32) - 136, (1 << 32) - 272  # virt + len = 2^32 is allowed (record 6, len 136); record 10 has len 273
    assert "virt + len of record 10 exceeds 2^32" in refused(w)[1]
    w[2, 2], w[11, 1] = (1 << 32) - 2, 1 << 33  # record 2 has len 3; the lowest record is named whatever its fault
    assert "virt + len of record 2 exceeds 2^32" in refused(w)[1]
    w[1, 0] = 1 << 32
    assert "a word of record 1 " in refused(w)[1]
    rows, why = refused(words, with_bytes=False)  # the inputs are missing although lengths are not 0
    assert "null pointer" in why and "d_bytes" in why
    # the sum of the lengths, on a count-only call (no byte is read): 2^31 + 2^31 reaches 2^32 with record 2
    w = np.array([[0, 0, 0, 0, 1 << 31], [0, 0, 0, 0, 5], [0, 0, 5, 0, (1 << 31) - 5], [0, 0, 0, 0, 0]], dtype=np.uint64)
    d_ops = pg.DeviceBuffer.from_host(gpu, w)
    rows, err = _call(gpu, d_ops.ptr, 4, None, 1, None, 0, scratch.ptr)
    assert err is not None and err.code == pg.GL_E_INVALID and "with record 2 the sum of the lengths reaches 2^32" in str(err) and rows == 0
    w[2, 4] -= 1  # one byte less: 2^32 - 1 in all
    d_ops.upload(w)
    rows, err = _call(gpu, d_ops.ptr, 4, None, 1, None, 0, scratch.ptr)
    assert err is None and rows == ((1 << 31) // 136 + 1) + 1 + (((1 << 31) - 6) // 136 + 1) + 1
    # ... and the same buffers take the untouched list
    d_ops = pg.DeviceBuffer.from_host(gpu, words)
    rows, err = _call(gpu, d_ops.ptr, num_ops, bytes_ptr, 5, trace.ptr, n, scratch.ptr)
    assert err is None and rows == 22
    assert th.first_difference(trace.download().reshape(COLUMNS, n), _reference("mixed", 5)) is None
    del d_bytes


@pytest.mark.gpu
def test_argument_refusals_launch_nothing(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib
    from plonky2_gpu_amd import keccak_sponge_table as ks

    words, data = _words("mixed")
    num_ops, n = len(words), 32
    scratch_words = _lib.load().gl_keccak_sponge_table_scratch_bytes(num_ops, 5) // 8
    fill = np.full(COLUMNS * n + 5 * num_ops + scratch_words, ONES, dtype=np.uint64)
    fill[COLUMNS * n : COLUMNS * n + 5 * num_ops] = words.reshape(-1)
    buf = pg.DeviceBuffer.from_host(gpu, fill)  # a trace, behind it the records, behind them the scratch
    d_ops, d_scratch = buf.at(COLUMNS * n), buf.at(COLUMNS * n + 5 * num_ops)
    assert d_scratch % 16 == 0
    d_bytes, bytes_ptr = ks.upload_bytes(gpu, data)
    rows_out = ctypes.c_uint64()

    def refused(*args):
        rows, err = _call(gpu, *args)
        assert err is not None and err.code == pg.GL_E_INVALID
        return str(err)

    assert "degree_bits" in refused(d_ops, num_ops, bytes_ptr, 0, buf.ptr, n, d_scratch)
    assert "degree_bits" in refused(d_ops, num_ops, bytes_ptr, 24, buf.ptr, 1 << 24, d_scratch)
    assert "num_ops" in refused(d_ops, (1 << 30) + 1, bytes_ptr, 5, buf.ptr, n, d_scratch)
    assert "trace_stride" in refused(d_ops, num_ops, bytes_ptr, 5, buf.ptr, n - 1, d_scratch)
    assert "null pointer" in refused(None, num_ops, bytes_ptr, 5, buf.ptr, n, d_scratch)
    assert "null pointer" in refused(d_ops, num_ops, bytes_ptr, 5, buf.ptr, n, None)
    assert "null pointer" in refused(None, 0, None, 5, buf.ptr, n, None)  # without operations the scratch is still asked for
    assert "aligned" in refused(d_ops, num_ops, bytes_ptr, 5, buf.ptr, n, d_scratch + 8)
    assert "d_trace overlaps d_ops" in refused(buf.at(COLUMNS * n - 1), num_ops, bytes_ptr, 5, buf.ptr, n, d_scratch)
    assert "d_scratch overlaps d_ops" in refused(d_ops, num_ops, bytes_ptr, 5, buf.ptr, n, d_scratch - 16)
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, bytes_ptr, 5, buf.ptr, n, buf.at(4))
    for args in ((d_ops, num_ops, bytes_ptr, 5, buf.ptr, n, d_scratch, None, gpu.ptr), (d_ops, num_ops, bytes_ptr, 5, buf.ptr, n, d_scratch, ctypes.byref(rows_out), None)):
        with pytest.raises(pg.Plonky2HipError, match="null pointer"):
            _lib.call("gl_keccak_sponge_table_trace", *args)
    assert _lib.load().gl_keccak_sponge_table_scratch_bytes(num_ops, 0) == 0 == _lib.load().gl_keccak_sponge_table_scratch_bytes(num_ops, 24)
    assert _lib.load().gl_keccak_sponge_table_scratch_bytes((1 << 30) + 1, 5) == 0
    gpu.synchronize()
    assert (buf.download() == fill).all()
    # the input bytes inside the trace: known once the device has counted them, refused before the fill
    rows, err = _call(gpu, d_ops, num_ops, buf.at(7), 5, buf.ptr, n, d_scratch)
    assert err is not None and "d_trace overlaps d_bytes" in str(err) and rows == 22
    gpu.synchronize()
    assert (buf.download(0, COLUMNS * n) == fill[: COLUMNS * n]).all()
    rows, err = _call(gpu, d_ops, num_ops, bytes_ptr, 5, buf.ptr, n, d_scratch)  # the same buffers, accepted
    assert err is None and rows == 22
    assert (buf.download(0, COLUMNS * n).reshape(COLUMNS, n) == _reference("mixed", 5)).all()
    assert (buf.download(COLUMNS * n, 5 * num_ops) == words.reshape(-1)).all()
    rows, err = _call(gpu, None, 0, None, 5, buf.ptr, n, d_scratch)  # no operations, no list, no bytes
    assert err is None and rows == 0 and not buf.download(0, COLUMNS * n).any()
    del d_bytes


# ---------------------------------------------------------------- the derived lists
@functools.lru_cache(maxsize=None)
def _log(name):
    return kr.log_of_ops(_ops(name))


def _derive(gpu, d_trace, degree_bits, stride, rows, shapes, which):
    """gl_keccak_sponge_table_ops into sentinel-filled buffers with a guard word behind each list -> the lists asked for"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    bufs = [pg.DeviceBuffer.from_host(gpu, filler(shape[0] * shape[1] + 1)) if k in which else None for k, shape in enumerate(shapes)]
    scratch = _scratch(gpu, 0, degree_bits)
    _lib.call("gl_keccak_sponge_table_ops", d_trace, stride, degree_bits, rows, *[b.ptr if b else None for b in bufs], scratch.ptr, gpu.ptr)
    out = []
    for b, shape in zip(bufs, shapes):
        if b is None:
            out.append(None)
            continue
        host = b.download()
        assert host[-1] == filler(host.size)[-1], "the word behind the list was written"
        out.append(host[:-1].reshape(shape))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", [(0,), (1,), (2,), (0, 1, 2)])
@pytest.mark.parametrize("name,pad", [("mixed", 0), ("mixed", 25), ("many300", 0)])
def test_derived_lists_equal_keccak_sponge_log(gpu, name, pad, which):
    """each output alone and all three together, from a device-built trace; the trace is left as it was"""
    from plonky2_gpu_amd import keccak_sponge_table as ks

    words, data = _words(name)
    bits = _exact_bits(name)
    n = 1 << bits
    d_trace = ks.generate_trace(gpu, words, data, degree_bits=bits, trace_stride=n + pad)
    before = d_trace.download()
    exp = _log(name)
    got = _derive(gpu, d_trace.ptr, bits, n + pad, d_trace.rows, [e.shape for e in exp], which)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert (g is None) == (k not in which)
        if g is not None:
            assert th.first_difference(g, e) is None, k
    assert (d_trace.download() == before).all()


@pytest.mark.gpu
def test_ops_argument_refusals(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib
    from plonky2_gpu_amd import keccak_sponge_table as ks

    words, data = _words("mixed")
    d_trace = ks.generate_trace(gpu, words, data, degree_bits=5)
    out = pg.DeviceBuffer(gpu, 22 * 136 * 14)
    scratch = _scratch(gpu, 0, 5)

    def refused(*args):
        with pytest.raises(pg.Plonky2HipError) as e:
            _lib.call("gl_keccak_sponge_table_ops", *args)
        assert e.value.code == pg.GL_E_INVALID
        return str(e.value)

    assert "null pointer" in refused(None, 32, 5, 22, out.ptr, None, None, scratch.ptr, gpu.ptr)
    assert "null pointer" in refused(d_trace.ptr, 32, 5, 22, out.ptr, None, None, None, gpu.ptr)
    assert "null pointer" in refused(d_trace.ptr, 32, 5, 22, out.ptr, None, None, scratch.ptr, None)
    assert "degree_bits" in refused(d_trace.ptr, 32, 0, 22, out.ptr, None, None, scratch.ptr, gpu.ptr)
    assert "rows" in refused(d_trace.ptr, 32, 5, 33, out.ptr, None, None, scratch.ptr, gpu.ptr)
    assert "trace_stride" in refused(d_trace.ptr, 31, 5, 22, out.ptr, None, None, scratch.ptr, gpu.ptr)
    assert "aligned" in refused(d_trace.ptr, 32, 5, 22, out.ptr, None, None, scratch.ptr + 8, gpu.ptr)
    assert "d_keccak_inputs overlaps d_trace" in refused(d_trace.ptr, 32, 5, 22, d_trace.at(100), None, None, scratch.ptr, gpu.ptr)
    assert "d_logic_ops overlaps d_trace" in refused(d_trace.ptr, 32, 5, 22, None, d_trace.at(COLUMNS * 32 - 1), None, scratch.ptr, gpu.ptr)
    assert "d_memory_ops overlaps d_trace" in refused(d_trace.ptr, 32, 5, 22, None, None, d_trace.ptr, scratch.ptr, gpu.ptr)
    assert "d_keccak_inputs overlaps d_logic_ops" in refused(d_trace.ptr, 32, 5, 22, out.ptr, out.at(22 * 25 - 1), None, scratch.ptr, gpu.ptr)
    arena = pg.DeviceBuffer(gpu, 64 + 22 * 5 * 17)  # a scratch at its head and a logic list that starts inside that scratch
    assert "d_logic_ops overlaps d_scratch" in refused(d_trace.ptr, 32, 5, 22, None, arena.at(8), None, arena.ptr, gpu.ptr)
    assert "d_keccak_inputs overlaps d_scratch" in refused(d_trace.ptr, 32, 5, 22, arena.at(8), None, None, arena.ptr, gpu.ptr)
    assert "d_memory_ops overlaps d_scratch" in refused(d_trace.ptr, 32, 5, 22, None, None, arena.at(8), arena.ptr, gpu.ptr)
    _lib.call("gl_keccak_sponge_table_ops", d_trace.ptr, 32, 5, 0, out.ptr, None, None, scratch.ptr, gpu.ptr)  # no rows: nothing to do
    _lib.call("gl_keccak_sponge_table_ops", d_trace.ptr, 32, 5, 22, None, None, None, scratch.ptr, gpu.ptr)  # no output: nothing to do


@pytest.mark.gpu
def test_the_derived_lists_build_the_other_three_tables(gpu):
    """the device-built chain: bytes -> sponge trace -> three lists -> gl_keccak_table_trace, gl_logic_table_trace and
    gl_memory_table_trace, each against its own table's reference on the reference's list; nothing visits the host in between"""
    from plonky2_gpu_amd import keccak_sponge_table as ks
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import memory_table as mt

    traces = _device_traces(gpu)
    keccak_inputs, logic_ops, memory_ops = _log("system")
    assert traces[ki.SPONGE].rows == 5 and th.first_difference(traces[ki.SPONGE].download().reshape(COLUMNS, 8), _reference("system", 3)) is None
    assert th.first_difference(traces[ki.KECCAK].download().reshape(kt.NUM_COLUMNS, 128), keccak_table_ref.generate_trace_rows(keccak_inputs, 128).T) is None
    assert th.first_difference(traces[ki.LOGIC].download().reshape(lt.NUM_COLUMNS, 32), logic_table_ref.trace_of_words(logic_ops, 5)) is None
    exp, rows = memory_table_ref.trace_of_words(memory_ops)
    assert traces[ki.MEMORY].rows == rows == 440 and exp.shape == (mt.NUM_COLUMNS, 512)
    assert th.first_difference(traces[ki.MEMORY].download().reshape(mt.NUM_COLUMNS, 512), exp) is None
    assert ks.NUM_COLUMNS == COLUMNS


# ---------------------------------------------------------------- single proofs
PROVABLE = {8: "system", 64: "many34"}  # 5 rows in 8; 63 in 64
TABLE = th.Table("keccak_sponge_table", kr.KeccakSpongeTableStark, COLUMNS, (8, 64), reference_trace=lambda n: _reference(PROVABLE[n], n.bit_length() - 1),
                 device_trace=lambda ctx, n: TABLE.module.generate_trace(ctx, *_words(PROVABLE[n]), degree_bits=n.bit_length() - 1),
                 flip=lambda ks: (ks.UPDATED_STATE_U32S + 11, 2))
_stark = TABLE.stark


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("compiled", [False, True])
@pytest.mark.parametrize("hasher,num_challenges", [("poseidon", 2), ("keccak", 1)])
def test_proof_bytes_of_the_device_built_trace_equal_the_reference(gpu, hasher, num_challenges, compiled, n):
    """interpreted and compiled, with both hashers (Keccak with 2 challenges would have quotient leaves of 4 elements, which
    KeccakHash<25> cannot hash: 1 there); the reference's verifier accepts"""
    assert kr.rows_needed(_ops(PROVABLE[n])) == {8: 5, 64: 63}[n]
    th.check_proof_bytes(TABLE, gpu, hasher, num_challenges, n, compiled=compiled, verify="closure" if compiled else "program")


@pytest.mark.gpu
def test_a_flipped_cell_of_updated_state_on_a_full_block_row_is_rejected(gpu):
    """row 2 of the system's trace is the first full-block row of the 300-byte operation: its updated_state_u32s is the next row's
    original state (constraint family 7). The device proves the violated trace as the reference does, and the verifier
    (tests/stark_verify.py, which accepts the proof of the untouched trace) rejects at zeta."""
    column, row = TABLE.flip(TABLE.module)
    assert _reference("system", 3)[TABLE.module.IS_FULL_INPUT_BLOCK, row] == 1
    th.check_flipped_cell_is_rejected(TABLE, gpu, "stark_verify")


# ---------------------------------------------------------------- the system
SYSTEM_FPS = [si.fri_params(rate_bits=1, cap_height=1, arity_bits=ab, num_query_rounds=4, proof_of_work_bits=2) for ab in ((2,), (2,), (2,), (2,), (1,))]
FOUR = [ki.SPONGE, ki.LOGIC, ki.MEMORY, ki.CPU]  # the system without the Keccak-f table, in ki.WITHOUT_KECCAK's numbers


def _device_traces(ctx):
    """the five traces of the system, every one but the stand-in's built on the device from the two byte strings"""
    from plonky2_gpu_amd import keccak_sponge_table as ks
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import memory_table as mt

    words, data = _words("system")
    sponge = ks.generate_trace(ctx, words, data, degree_bits=3)
    keccak_inputs, logic_ops, memory_ops = ks.derive_ops(ctx, sponge, 3, sponge.rows, num_bytes=sum(ki.SYSTEM_LENGTHS))
    assert (keccak_inputs.n, logic_ops.n, memory_ops.n) == (5 * 25, 25 * 17, 440 * 14)
    return [sponge, kt.generate_trace(ctx, keccak_inputs, 7), lt.generate_trace(ctx, logic_ops, degree_bits=5), mt.generate_trace(ctx, memory_ops),
            ki.cpu_trace(_ops("system"))]


@functools.lru_cache(maxsize=None)
def _host_traces():
    keccak_inputs, logic_ops, memory_ops = _log("system")
    as_lists = lambda cols: [[int(v) for v in col] for col in cols]  # noqa: E731
    return [as_lists(_reference("system", 3)), as_lists(keccak_table_ref.generate_trace_rows(keccak_inputs, 128).T),
            as_lists(logic_table_ref.trace_of_words(logic_ops, 5)), as_lists(memory_table_ref.trace_of_words(memory_ops)[0]), ki.cpu_trace(_ops("system"))]


@functools.lru_cache(maxsize=None)
def _starks():
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import memory_table as mt

    return [_stark(), keccak_table_ref.KeccakTableStark(*kt.program()), logic_table_ref.LogicTableStark(*lt.program()),
            memory_table_ref.MemoryTableStark(*mt.program()), ki.CpuStandIn()]


def _descs(tables, num_challenges):
    from plonky2_gpu_amd import keccak_sponge_table as ks
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import memory_table as mt
    from plonky2_gpu_amd.stark import StarkDesc

    cpu = _starks()[ki.CPU]
    make = {ki.SPONGE: lambda fp: ks.stark_desc(3, num_challenges, fp), ki.KECCAK: lambda fp: kt.stark_desc(7, num_challenges, fp),
            ki.LOGIC: lambda fp: lt.stark_desc(5, num_challenges, fp), ki.MEMORY: lambda fp: mt.stark_desc(9, num_challenges, fp),
            ki.CPU: lambda fp: StarkDesc(2, ki.CPU_COLUMNS, 0, 3, num_challenges, fp, cpu.instrs, cpu.immediates)}
    return [make[k](SYSTEM_FPS[k]) for k in tables]


@functools.lru_cache(maxsize=None)
def _reference_system_proof(which, logic_filter="rows"):
    """(bytes, system, fri_params, the tables of the five it has) from tests/ctl_ref.py, Poseidon, 2 challenges"""
    from oracle import accel

    tables = list(range(5)) if "keccak" in which else FOUR
    numbers = None if "keccak" in which else ki.WITHOUT_KECCAK
    system = ki.System([_starks()[k] for k in tables], ki.lookups(which, logic_filter=logic_filter, numbers=numbers))
    fps = [SYSTEM_FPS[k] for k in tables]
    with accel.c_backend():
        # check=False: with the Keccak-f lookup the product identity cannot hold (see the test below)
        proofs = cr.prove_tables(HASHERS["poseidon"], system, 2, fps, [_host_traces()[k] for k in tables], check="keccak" not in which)
    return cr.proofs_bytes(HASHERS["poseidon"], proofs), system, fps, tables


def _prove_system(gpu, which, logic_filter="rows"):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd.stark import StarkTablesDesc

    exp, system, fps, tables = _reference_system_proof(which, logic_filter)
    desc = StarkTablesDesc(_descs(tables, 2), system.lookups)
    desc.validate()
    traces = _device_traces(gpu)
    nt = pg.NativeStarkTables(gpu, desc)
    try:
        data = nt.prove_bytes([traces[k] for k in tables])
    finally:
        nt.close()
    return data, exp, desc, system, fps


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("logic",), ("memory",), ("sponge",)])
def test_one_lookup_with_the_table_it_ties_equals_the_reference(gpu, which):
    """two tables each: the sponge and the logic table (5 lookers), the memory table (136 lookers, strict filter) or the stand-in for
    the CPU table (the sponge as the looked table)"""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark
    from plonky2_gpu_amd.stark import StarkTablesDesc

    other = {"logic": ki.LOGIC, "memory": ki.MEMORY, "sponge": ki.CPU}[which[0]]
    numbers = {"sponge": 0, {"logic": "logic", "memory": "memory", "sponge": "cpu"}[which[0]]: 1}
    system = ki.System([_starks()[ki.SPONGE], _starks()[other]], ki.lookups(which, numbers=numbers))
    fps = [SYSTEM_FPS[ki.SPONGE], SYSTEM_FPS[other]]
    with accel.c_backend():
        exp = cr.proofs_bytes(HASHERS["poseidon"], cr.prove_tables(HASHERS["poseidon"], system, 2, fps, [_host_traces()[ki.SPONGE], _host_traces()[other]]))
    desc = StarkTablesDesc(_descs([ki.SPONGE, other], 2), system.lookups)
    desc.validate()
    traces = _device_traces(gpu)
    nt = pg.NativeStarkTables(gpu, desc)
    try:
        data = nt.prove_bytes([traces[ki.SPONGE], traces[other]])
        if which == ("memory",):  # the 136-looker case through gl_stark_tables_ctl_zs
            challenges = [(3, 5), (1 << 40, P_MINUS_1)]
            got = nt.ctl_zs(0, _reference("system", 3), challenges)
            want = np.array(cr.ctl_z_polys(system.lookups, 2, 0, _host_traces()[ki.SPONGE], challenges), dtype=np.uint64)
            assert got.shape == want.shape == (272, 8) and (got == want).all()
    finally:
        nt.close()
    assert data == exp
    with accel.c_backend():
        assert cr.verify_tables(HASHERS["poseidon"], system, 2, fps, pstark.tables_proof_from_bytes(data, desc))


P_MINUS_1 = 0xFFFFFFFF00000000


@pytest.mark.gpu
def test_the_system_without_the_keccak_f_lookup_is_proved_and_accepted(gpu):
    """Sponge (8 rows, 5 used), logic (32 rows, 25 XORs), memory (512 rows from 440 reads), the stand-in for the CPU table (4 rows),
    every trace but the stand-in's built on the device; three lookups — logic with ctl_looking_logic_filter(), memory with its 136
    lookers and the strict filter, the looked sponge — put 142 table-with-columns entries on the sponge table: 284 CTL Zs with 2
    challenges. Byte for byte tests/ctl_ref.py's proof, and its verifier accepts. With remainders 4 and 28 the reference's own logic
    filter selects the same rows and gives the same proof. Interpreted: the generated quotient kernel of a table with 284 CTL Zs
    takes minutes to compile; the compiled path is covered on the single table above."""
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    which = ("logic", "memory", "sponge")
    data, exp, desc, system, fps = _prove_system(gpu, which)
    assert desc.num_ctl_zs(0) == 2 * 142
    assert data == exp
    with accel.c_backend():
        assert cr.verify_tables(HASHERS["poseidon"], system, 2, fps, pstark.tables_proof_from_bytes(data, desc))
    data_ref, exp_ref, _, _, _ = _prove_system(gpu, which, logic_filter="reference")
    assert data_ref == exp_ref == exp


@pytest.mark.gpu
def test_the_whole_system_is_proved_as_the_reference_proves_it_and_rejected_for_the_keccak_f_lookup(gpu):
    """All five tables and all four lookups (Keccak-f with xored=True; 128 Keccak-f rows hold exactly the 5 permutations:
    24 * 5 <= 128 < 24 * 6, so no padding permutation reaches its looked round-23 row): 143 table-with-columns entries on the
    sponge table. The device's proof is tests/ctl_ref.py's byte for byte. Its verifier accepts every table's own proof and REJECTS
    at the cross-table product of the Keccak-f lookup: the Keccak-f table's ctl_data offers the state entering round 23 where the
    sponge sends the permutation's input (tests/test_keccak_sponge_table_ref.py
    test_the_keccak_f_table_s_own_lookup_offers_round_23_s_input) — a prover cannot mend what the looked table's description
    says."""
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    data, exp, desc, system, fps = _prove_system(gpu, ("keccak", "logic", "memory", "sponge"))
    assert desc.num_ctl_zs(0) == 2 * 143
    assert data == exp
    with accel.c_backend():
        with pytest.raises(AssertionError, match="cross-table lookup: the products of the looking and of the looked table differ"):
            cr.verify_tables(HASHERS["poseidon"], system, 2, fps, pstark.tables_proof_from_bytes(data, desc))
