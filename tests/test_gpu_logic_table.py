"""The logic table on the device: gl_logic_table_trace against tests/logic_table_ref.py's restatement of generate_trace_rows on all
523 columns, its refusals, and the table proved by gl_stark_prove / gl_stark_tables_prove from the device-built trace against
tests/stark_ref.py and tests/ctl_ref.py, byte for byte: there is no tolerance anywhere.

The shapes cross the edges of the kernel as built: no operation, 1 and 2 in the smallest trace, 3 (an odd count: a pair of rows that
straddles operations and padding), 31 / 32 (below a wave), 255 and 257 (a 256-thread workgroup; one row beyond), 2049 (more than one
workgroup at either store width: 2048 rows are four workgroups of two rows per thread). Every shape runs at the tight pitch, at an
even padded pitch and at an odd one, which the 16-byte store path of the measurement hook cannot take."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref as cr  # noqa: E402
import logic_table_instances as li  # noqa: E402
import logic_table_ref as lr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
import table_harness as th  # noqa: E402
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from strided import Strided, filler  # noqa: E402

P = 0xFFFFFFFF00000001
ONES = (1 << 64) - 1
HASHERS = th.HASHERS
COLUMNS = 523


# ---------------------------------------------------------------- instances and reference traces
@functools.lru_cache(maxsize=None)
def _ops(num_ops, family="mixed"):
    w = li.FAMILIES[family](num_ops)
    assert w.shape == (num_ops, 17)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _reference(num_ops, degree_bits, family="mixed"):
    """[523][2^degree_bits] columns; never changed"""
    cols = lr.trace_of_words(_ops(num_ops, family), degree_bits)
    assert cols.shape == (COLUMNS, 1 << degree_bits)
    cols.setflags(write=False)
    return cols


def _call(gpu, d_ops, num_ops, degree_bits, d_trace, stride, d_scratch):
    """gl_logic_table_trace; None or the error"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    try:
        _lib.call("gl_logic_table_trace", d_ops, num_ops, degree_bits, d_trace, stride, d_scratch, gpu.ptr)
    except pg.Plonky2HipError as e:
        return e
    return None


SHAPES = [(0, 1), (1, 1), (2, 1), (3, 2), (31, 5), (32, 5), (255, 8), (257, 9), (2049, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 24, 25])
@pytest.mark.parametrize("num_ops,degree_bits", SHAPES)
def test_trace_equals_generate_trace_rows(gpu, num_ops, degree_bits, pad):
    """The buffer is pre-filled with 0xFF bytes — an unwritten word shows —, guards and the gap of a padded pitch hold sentinels that
    must survive. The operations are left as they were."""
    import plonky2_gpu_amd as pg

    exp = _reference(num_ops, degree_bits)
    n = 1 << degree_bits
    assert degree_bits == max(1, (max(num_ops, 1) - 1).bit_length())  # the reference's height
    buf = Strided(gpu, np.full((COLUMNS, n), ONES, dtype=np.uint64), n + pad)
    d_ops = pg.DeviceBuffer.from_host(gpu, _ops(num_ops)) if num_ops else None
    scratch = pg.DeviceBuffer(gpu, 2)
    assert _call(gpu, d_ops.ptr if d_ops else None, num_ops, degree_bits, buf.ptr, n + pad, scratch.ptr) is None
    got = buf.polys((num_ops, degree_bits, pad))
    buf.free()
    if d_ops:
        assert (d_ops.download().reshape(num_ops, 17) == _ops(num_ops)).all()
    assert th.first_difference(got, exp) is None


@pytest.mark.gpu
@pytest.mark.parametrize("num_ops,degree_bits", [(3, 2), (257, 9)])
def test_trace_one_word_off_a_16_byte_boundary(gpu, num_ops, degree_bits):
    """d_trace at 8 modulo 16 with an even pitch: only 8-byte stores can write it. Sentinels in front, between the columns and behind."""
    import plonky2_gpu_amd as pg

    exp = _reference(num_ops, degree_bits)
    n = 1 << degree_bits
    stride, front, tail = n + 2, 3, 64
    total = front + COLUMNS * stride + tail
    buf = pg.DeviceBuffer.from_host(gpu, filler(total))
    assert buf.at(front) % 16 == 8
    d_ops, scratch = pg.DeviceBuffer.from_host(gpu, _ops(num_ops)), pg.DeviceBuffer(gpu, 2)
    assert _call(gpu, d_ops.ptr, num_ops, degree_bits, buf.at(front), stride, scratch.ptr) is None
    out, fill = buf.download(), filler(total)
    assert (out[:front] == fill[:front]).all() and (out[-tail:] == fill[-tail:]).all()
    body, pads = out[front:-tail].reshape(COLUMNS, stride), fill[front:-tail].reshape(COLUMNS, stride)
    assert (body[:, n:] == pads[:, n:]).all()
    assert th.first_difference(body[:, :n], exp) is None


@pytest.mark.gpu
@pytest.mark.parametrize("num_ops,degree_bits", [(3, 3), (257, 10)])
def test_degree_bits_one_above_the_need_plays_min_rows(gpu, num_ops, degree_bits):
    from plonky2_gpu_amd import logic_table as lt

    exp = _reference(num_ops, degree_bits)
    assert (exp[:, : 1 << (degree_bits - 1)] == _reference(num_ops, degree_bits - 1)).all() and not exp[:, 1 << (degree_bits - 1) :].any()
    got = lt.generate_trace(gpu, _ops(num_ops), degree_bits=degree_bits).download().reshape(COLUMNS, 1 << degree_bits)
    assert th.first_difference(got, exp) is None


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["random", "edge_limbs", "equal_inputs", "and_only", "or_only", "xor_only"])
def test_generate_trace_of_the_module_on_every_family(gpu, family):
    """65 operations (a wave and one) through logic_table.generate_trace: host words, the smallest height, then a padded pitch from
    a DeviceBuffer of the words"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import logic_table as lt

    w, exp = _ops(65, family), _reference(65, 7, family)
    assert th.first_difference(lt.generate_trace(gpu, w).download().reshape(COLUMNS, 128), exp) is None
    d_ops = pg.DeviceBuffer.from_host(gpu, w)
    got = lt.generate_trace(gpu, d_ops, trace_stride=128 + 24).download().reshape(COLUMNS, 152)[:, :128]
    assert th.first_difference(got, exp) is None
    assert not lt.generate_trace(gpu, lt.ops_to_words([])).download().any()


@pytest.mark.gpu
@pytest.mark.parametrize("num_ops,degree_bits", [(0, 1), (3, 2), (255, 8), (257, 9), (2049, 12)])
def test_both_store_widths_write_the_same_trace(gpu, num_ops, degree_bits):
    """gl_debug_logic_table_fill: one row per thread and two adjacent rows per thread (16-byte stores; an odd count of operations
    puts an operation and a padding row into one pair), at the tight and at an even padded pitch. Two rows per thread are refused
    at an odd pitch and off a 16-byte boundary."""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    exp = _reference(num_ops, degree_bits)
    n = 1 << degree_bits
    d_ops = pg.DeviceBuffer.from_host(gpu, _ops(num_ops)) if num_ops else None
    ops_ptr = d_ops.ptr if d_ops else None
    for pad in (0, 24):
        for width in (1, 2):
            buf = Strided(gpu, np.full((COLUMNS, n), ONES, dtype=np.uint64), n + pad)
            _lib.call("gl_debug_logic_table_fill", ops_ptr, num_ops, degree_bits, buf.ptr, n + pad, width, gpu.ptr)
            got = buf.polys((num_ops, degree_bits, pad, width))
            buf.free()
            assert th.first_difference(got, exp) is None, width
    buf = pg.DeviceBuffer(gpu, COLUMNS * (n + 25) + 1)
    for ptr, stride, width, why in ((buf.ptr, n + 25, 2, "even trace_stride"), (buf.at(1), n + 24, 2, "16-byte aligned"), (buf.ptr, n, 3, "rows_per_thread"),
                                    (buf.ptr, n, 0, "rows_per_thread"), (buf.ptr, n - 1, 1, "trace_stride")):
        with pytest.raises(pg.Plonky2HipError, match=why) as e:
            _lib.call("gl_debug_logic_table_fill", ops_ptr, num_ops, degree_bits, ptr, stride, width, gpu.ptr)
        assert e.value.code == pg.GL_E_INVALID


# ---------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_data_refusals_write_nothing_and_name_the_lowest_record(gpu):
    import plonky2_gpu_amd as pg

    n, num_ops = 512, 300
    fill = np.full(COLUMNS * n, ONES, dtype=np.uint64)
    trace = pg.DeviceBuffer.from_host(gpu, fill)
    scratch = pg.DeviceBuffer(gpu, 2)

    def refused(w):
        d_ops = pg.DeviceBuffer.from_host(gpu, w)
        err = _call(gpu, d_ops.ptr, len(w), 9, trace.ptr, n, scratch.ptr)
        assert err is not None and err.code == pg.GL_E_INVALID
        gpu.synchronize()
        assert (trace.download() == fill).all()
        return str(err)

    w = _ops(num_ops).copy()
    w[[290, 37], 0] = 3
    why = refused(w)
    assert "operator of record 37 " in why and "290" not in why
    w = _ops(num_ops).copy()
    w[270, 16], w[41, 9] = 1 << 32, ONES
    why = refused(w)
    assert "limb of record 41 " in why and "2^32 or more" in why and "270" not in why
    w = _ops(num_ops).copy()
    w[260, 0], w[258, 1], w[299, 0] = 3, 1 << 32, ONES  # the limb comes first
    assert "limb of record 258 " in refused(w)
    w = _ops(num_ops).copy()
    w[0, 0], w[1, 5] = 1 << 32, 1 << 63  # the operator comes first: an operator word is not cut to 32 bits
    assert "operator of record 0 " in refused(w)
    w = _ops(num_ops).copy()
    w[299, 0], w[299, 16] = 4, 1 << 40  # both in one record, the last: the operator is named
    assert "operator of record 299 " in refused(w)
    # ... and the same buffers take the untouched list
    d_ops = pg.DeviceBuffer.from_host(gpu, _ops(num_ops))
    assert _call(gpu, d_ops.ptr, num_ops, 9, trace.ptr, n, scratch.ptr) is None
    assert th.first_difference(trace.download().reshape(COLUMNS, n), _reference(num_ops, 9)) is None


@pytest.mark.gpu
def test_argument_refusals_launch_nothing(gpu):
    import plonky2_gpu_amd as pg

    num_ops, n = 10, 32
    w = _ops(num_ops)
    fill = np.full(COLUMNS * n + 17 * num_ops + 2, ONES, dtype=np.uint64)
    fill[COLUMNS * n : COLUMNS * n + 17 * num_ops] = w.reshape(-1)
    buf = pg.DeviceBuffer.from_host(gpu, fill)  # a trace, behind it the operations, behind them the scratch
    d_ops, d_scratch = buf.at(COLUMNS * n), buf.at(COLUMNS * n + 17 * num_ops)
    assert d_scratch % 16 == 0

    def refused(*args):
        err = _call(gpu, *args)
        assert err is not None and err.code == pg.GL_E_INVALID
        return str(err)

    assert "degree_bits" in refused(d_ops, num_ops, 0, buf.ptr, n, d_scratch)
    assert "degree_bits" in refused(d_ops, num_ops, 24, buf.ptr, 1 << 24, d_scratch)
    assert "num_ops" in refused(d_ops, n + 1, 5, buf.ptr, n, d_scratch)
    assert "num_ops" in refused(d_ops, 3, 1, buf.ptr, n, d_scratch)
    assert "trace_stride" in refused(d_ops, num_ops, 5, buf.ptr, n - 1, d_scratch)
    assert "null pointer" in refused(None, num_ops, 5, buf.ptr, n, d_scratch)
    assert "null pointer" in refused(d_ops, num_ops, 5, None, n, d_scratch)
    assert "null pointer" in refused(d_ops, num_ops, 5, buf.ptr, n, None)
    assert "null pointer" in refused(None, 0, 5, buf.ptr, n, None)  # without operations the scratch is still asked for
    assert "aligned" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch + 8)
    assert "d_trace overlaps d_ops" in refused(buf.at(COLUMNS * n - 1), num_ops, 5, buf.ptr, n, d_scratch)  # its first word is the trace's last
    assert "d_trace overlaps d_ops" in refused(buf.at(5), num_ops, 5, buf.ptr, n, d_scratch)
    assert "d_scratch overlaps d_ops" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch - 16)
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, 5, buf.ptr, n, buf.at(COLUMNS * n - 2))  # the trace's last two words
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, 5, buf.ptr, n, buf.at(4))
    from plonky2_gpu_amd import _lib

    with pytest.raises(pg.Plonky2HipError, match="null pointer"):
        _lib.call("gl_logic_table_trace", d_ops, num_ops, 5, buf.ptr, n, d_scratch, None)
    gpu.synchronize()
    assert (buf.download() == fill).all()
    assert _call(gpu, d_ops, num_ops, 5, buf.ptr, n, d_scratch) is None  # the same buffers, accepted
    assert (buf.download(0, COLUMNS * n).reshape(COLUMNS, n) == _reference(num_ops, 5)).all()
    assert (buf.download(COLUMNS * n, 17 * num_ops) == fill[COLUMNS * n : COLUMNS * n + 17 * num_ops]).all()
    assert _call(gpu, None, 0, 5, buf.ptr, n, d_scratch) is None  # no operations, no list
    assert not buf.download(0, COLUMNS * n).any()


# ---------------------------------------------------------------- proofs
FP = th.FP
PROVABLE = {32: 21, 64: 64}  # 11 padding rows in 32; none in 64
TABLE = th.Table("logic_table", lr.LogicTableStark, COLUMNS, (32, 64), reference_trace=lambda n: _reference(PROVABLE[n], n.bit_length() - 1),
                 device_trace=lambda ctx, n: TABLE.module.generate_trace(ctx, _ops(PROVABLE[n]), degree_bits=n.bit_length() - 1),
                 flip=lambda lt: (lt.RESULT + 5, 7))
_stark, _reference_proof, _device_trace = TABLE.stark, TABLE.reference_proof, TABLE.device_trace


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("hasher,num_challenges", [("poseidon", 1), ("poseidon", 2), ("keccak", 1), ("keccak", 3)])
def test_proof_bytes_of_the_device_built_trace_equal_the_reference(gpu, hasher, num_challenges, n):
    """Keccak with 2 challenges would have quotient leaves of 4 elements, which KeccakHash<25> cannot hash (the reference panics): 1
    and 3 there."""
    verify = "closure" if (hasher, num_challenges) in (("poseidon", 2), ("keccak", 1)) else None
    th.check_proof_bytes(TABLE, gpu, hasher, num_challenges, n, verify=verify)


@pytest.mark.gpu
def test_compiled_in_units_gives_the_same_bytes(gpu):
    """unit_instrs=0: the library's cap. num_units is what split_program cuts the program into, and one more where the checks
    behind the program do not fit the last unit — this table has none, so the numbers agree."""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import stark as pstark

    exp = _reference_proof("poseidon", 2, 32)
    desc = lt.stark_desc(5, 2, FP)
    program_units = len(pstark.split_program(desc, 0))
    ns = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=0)
    try:
        assert ns.is_compiled and ns.num_units == program_units >= 1
        assert len(ns.unit_sources) == program_units
        data = ns.prove_bytes(_device_trace(gpu, 32), [])
        assert data == exp
    finally:
        ns.close()
    with accel.c_backend():
        assert sr.verify(HASHERS["poseidon"], _stark(), 2, FP, pstark.proof_from_bytes(data, desc))


@pytest.mark.gpu
def test_quotient_polys_on_random_words_equal_the_reference(gpu):
    """uniformly random u64 words, the non-canonical ones (about 2^-32 of them) and a planted 2^64 - 1 and p included, in place of
    the LDE of the trace (every constraint non-zero), at the tight and at a padded column pitch"""
    rng = np.random.default_rng(523)
    lde = rng.integers(0, 1 << 64, size=(COLUMNS, 64), dtype=np.uint64)
    lde[3, 0], lde[259, 1], lde[515, 2], lde[0, 3], lde[2, 63] = ONES, P, ONES, P + 1, ONES - 1
    alphas = [int(x) for x in rng.integers(0, 1 << 64, size=2, dtype=np.uint64)]
    th.check_quotient_polys(TABLE, gpu, lde, alphas)


@pytest.mark.gpu
def test_a_flipped_result_limb_gives_a_proof_the_verifier_rejects(gpu):
    """quotient_degree_factor 2 is a power of two: the reference's trim cannot fail, its prover returns a proof of the violated trace,
    and verification (tests/stark_verify.py, which accepts the proof of the untouched trace) fails at zeta. The device does the same."""
    th.check_flipped_cell_is_rejected(TABLE, gpu, "stark_verify")


# ---------------------------------------------------------------- the lookup: a sponge-shaped looker and a plain one
U32S, BYTES, XORED, F_XOR, PLAIN, F_PLAIN, LOOKER_COLUMNS = 0, 8, 40, 48, 49, 76, 77


class _Looker:
    """the 77-column stand-in for the tables that look into the logic table. Columns 0 .. 7: eight u32s (the sponge's
    original_rate_u32s), 8 .. 39: 32 bytes (block_bytes), 40 .. 47: eight u32s (xored_rate_u32s), 48: the filter of the XOR lookup;
    49 .. 75: an operation as the logic table's lookup spells it (three flags, 8 + 8 + 8 limbs), 76: its filter. Its own
    constraints: both filters are boolean."""
    num_columns, num_public_inputs, constraint_degree, pairs = LOOKER_COLUMNS, 0, 3, []

    def __init__(self):
        from plonky2_gpu_amd.stark import StarkAsm

        a = StarkAsm()
        for c in (F_XOR, F_PLAIN):
            a.release()
            f = a.local(c)
            a.emit(a.mul(f, a.sub(f, a.imm(1))))
        self.instrs, self.immediates = a.program()

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        for c in (F_XOR, F_PLAIN):
            consumer.constraint(F.mul(local[c], F.sub(local[c], F.one)))


def _ctl_looking_logic():
    """ctl_looking_logic(i) of the sponge (keccak_sponge_stark.rs:88-126) over the looker's columns: is_and = 0, is_or = 0,
    is_xor = 1 as constants, eight single u32 columns, eight le_bytes combinations of four byte columns, eight single u32 columns"""
    from plonky2_gpu_amd.stark import CtlColumn

    res = [CtlColumn((), 0), CtlColumn((), 0), CtlColumn((), 1)]
    res += [CtlColumn.single(U32S + k) for k in range(8)]
    res += [CtlColumn([(BYTES + 4 * k + j, 1 << (8 * j)) for j in range(4)]) for k in range(8)]
    res += [CtlColumn.single(XORED + k) for k in range(8)]
    return res


@functools.lru_cache(maxsize=None)
def _lookup_system():
    """(looker trace [77][16], logic words [20][17], lookups): the XORs of mixed(20) in the sponge-shaped columns, its ANDs and ORs in
    the plain ones, one per row from row 0; the other rows carry sevens under a filter of 0"""
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, TableWithColumns

    w = _ops(20)
    rows = np.full((16, LOOKER_COLUMNS), 7, dtype=np.uint64)
    rows[:, F_XOR] = rows[:, F_PLAIN] = 0
    xors, plains = [rec for rec in w if rec[0] == 2], [rec for rec in w if rec[0] != 2]
    assert 0 < len(xors) <= 16 and 0 < len(plains) <= 16 and {int(rec[0]) for rec in plains} == {0, 1}
    for r, rec in enumerate(xors):
        x, y = rec[1:9], rec[9:17]
        rows[r, U32S : U32S + 8], rows[r, XORED : XORED + 8], rows[r, F_XOR] = x, x ^ y, 1
        rows[r, BYTES : BYTES + 32] = [(int(limb) >> (8 * j)) & 0xFF for limb in y for j in range(4)]
    for r, rec in enumerate(plains):
        x, y = rec[1:9], rec[9:17]
        rows[r, PLAIN : PLAIN + 3] = [int(rec[0] == f) for f in range(3)]
        rows[r, PLAIN + 3 : PLAIN + 11], rows[r, PLAIN + 11 : PLAIN + 19], rows[r, F_PLAIN] = x, y, 1
        rows[r, PLAIN + 19 : PLAIN + 27] = x & y if rec[0] == 0 else x | y
    lookups = [CrossTableLookup([TableWithColumns(0, _ctl_looking_logic(), CtlColumn.single(F_XOR)),
                                 TableWithColumns(0, [CtlColumn.single(PLAIN + k) for k in range(27)], CtlColumn.single(F_PLAIN))],
                                TableWithColumns(1, lt.ctl_data(), lt.ctl_filter()))]
    return [[int(v) for v in col] for col in rows.T], w, lookups


# Keccak with 2 challenges would give the looker 4 CTL Zs and both tables 4 quotient polynomials: 1 there
@pytest.mark.gpu
@pytest.mark.parametrize("hasher,num_challenges,compiled", [("poseidon", 2, False), ("poseidon", 2, True), ("keccak", 1, False)])
def test_three_twcs_with_the_logic_lookup_equal_the_reference(gpu, hasher, num_challenges, compiled):
    """The logic table, 32 rows built on the device from 20 operations, is looked with ctl_filter() = IS_AND + IS_OR + IS_XOR: its 12
    padding rows have filter 0. One lookup over 27 columns, two looking TWCs of one 16-row table: the sponge's ctl_looking_logic
    shape for the XORs (constants, single columns, le_bytes combinations) and plain single columns for the ANDs and ORs."""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import logic_table as lt
    from plonky2_gpu_amd import stark as pstark
    from plonky2_gpu_amd.stark import StarkDesc, StarkTablesDesc

    looker_trace, w, lookups = _lookup_system()
    cols = _reference(20, 5)
    looker = _Looker()
    fps = [si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,), num_query_rounds=4, proof_of_work_bits=2) for _ in range(2)]
    system = th.System([looker, _stark()], lookups)
    with accel.c_backend():
        exp = cr.proofs_bytes(HASHERS[hasher], cr.prove_tables(HASHERS[hasher], system, num_challenges, fps,
                                                               [looker_trace, [[int(v) for v in col] for col in cols]]))
    desc = StarkTablesDesc([StarkDesc(4, LOOKER_COLUMNS, 0, 3, num_challenges, fps[0], looker.instrs, looker.immediates),
                            lt.stark_desc(5, num_challenges, fps[1])], lookups)
    desc.validate(hasher)
    nt = pg.NativeStarkTables(gpu, desc, hasher, compiled=compiled, unit_instrs=0 if compiled else None)
    try:
        if compiled:
            assert nt.is_compiled and nt.num_units[1] >= len(pstark.split_program(desc.tables[1], 0))
        data = nt.prove_bytes([looker_trace, lt.generate_trace(gpu, w, degree_bits=5)])
    finally:
        nt.close()
    assert data == exp
    with accel.c_backend():
        assert cr.verify_tables(HASHERS[hasher], system, num_challenges, fps, pstark.tables_proof_from_bytes(data, desc, hasher))


# ---------------------------------------------------------------- two contexts, two threads
@pytest.mark.gpu
def test_two_contexts_on_two_threads_build_and_prove(gpu):
    th.check_two_contexts_on_two_threads(TABLE, gpu)
