"""The memory table on the device: gl_memory_table_trace from UNSORTED operations against tests/memory_table_ref.py's literal
generate_trace on all 26 columns, its count and its refusals, and the table proved by gl_stark_prove / gl_stark_tables_prove from
the device-built trace against tests/stark_ref.py and tests/ctl_ref.py, byte for byte: there is no tolerance anywhere.

The numbers of operations cross the edges of the kernels as built: 2 (the least), 3 and 5 (no power of two), 64 / 65 (a wave),
257 (a 256-thread workgroup), 2048 / 2049 (a tile of the radix sort and a block of the scans, both 2048), 5000 (three tiles, the
last ragged), 65537 (33 tiles, whose 256 x 33 digit counters take five blocks of the scan)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref as cr  # noqa: E402
import memory_table_instances as mi  # noqa: E402
import memory_table_ref as mr  # noqa: E402
import stark_instances as si  # noqa: E402
import table_harness as th  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = 0xFFFFFFFF00000001
ONES = (1 << 64) - 1
HASHERS = th.HASHERS
COLUMNS = 26


# ---------------------------------------------------------------- instances and reference traces
@functools.lru_cache(maxsize=None)
def _ops(family, num_ops):
    if family == "one_long_gap":
        w = mi.one_long_gap()
    elif family == "provable":
        w = mi.provable(seed=num_ops, extra=num_ops - 10)
    elif family in ("in_order", "reversed"):
        w = mi.in_order(num_ops, reverse=family == "reversed")
    else:
        w = getattr(mi, family)(num_ops)
    assert w.shape == (num_ops, 14)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _reference(family, num_ops, extra_bits=0):
    """([26][n] columns, operations + dummies); never changed"""
    w = _ops(family, num_ops)
    rows = mr.rows_needed(w)
    cols, rows_again = mr.trace_of_words(w, (rows - 1).bit_length() + extra_bits if extra_bits else None)
    assert rows_again == rows and cols.shape[1] == mr.next_power_of_two(rows) << extra_bits
    cols.setflags(write=False)
    return cols, rows


def _call(gpu, d_ops, num_ops, degree_bits, d_trace, stride, d_scratch):
    """gl_memory_table_trace; (rows, None) or (rows, the error)"""
    import ctypes

    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    rows = ctypes.c_uint64(ONES)
    try:
        _lib.call("gl_memory_table_trace", d_ops, num_ops, degree_bits, d_trace, stride, d_scratch, ctypes.byref(rows), gpu.ptr)
    except pg.Plonky2HipError as e:
        return int(rows.value), e
    return int(rows.value), None


def _scratch(gpu, num_ops, degree_bits):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    size = _lib.load().gl_memory_table_scratch_bytes(num_ops, degree_bits)
    assert size and size % 16 == 0
    return pg.DeviceBuffer(gpu, size // 8)


# family, operations, pitch beyond n, degree_bits above the need
TRACES = [("small_keys", 2, 0, 0), ("small_keys", 3, 24, 0), ("small_keys", 5, 0, 0), ("small_keys", 64, 24, 0), ("small_keys", 65, 0, 0),
          ("small_keys", 257, 24, 0), ("small_keys", 2048, 0, 0), ("small_keys", 2049, 24, 0), ("small_keys", 5000, 0, 0), ("small_keys", 65537, 24, 0),
          ("mixed", 5, 24, 0), ("mixed", 65, 24, 0), ("mixed", 257, 0, 0), ("mixed", 2049, 0, 0), ("mixed", 5000, 24, 0),
          ("in_order", 2049, 0, 0), ("reversed", 2049, 24, 0), ("one_address", 257, 0, 0), ("at_the_top", 65, 0, 0), ("at_the_top", 2048, 24, 0),
          ("one_long_gap", 4, 0, 0), ("one_long_gap", 4, 24, 0), ("gaps_in_the_first_half", 300, 0, 0), ("gaps_in_the_first_half", 2049, 24, 0),
          ("provable", 10, 0, 0), ("provable", 13, 24, 1), ("no_gap", 64, 0, 0), ("no_gap", 2048, 24, 0), ("wide", 65537, 0, 0),
          ("small_keys", 65, 24, 2), ("mixed", 257, 24, 2), ("no_gap", 64, 0, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,num_ops,pad,extra_bits", TRACES)
def test_trace_equals_generate_trace(gpu, family, num_ops, pad, extra_bits):
    """small_keys: many fully equal keys with differing values (stability), every field's upper radix passes skipped; mixed: dummies
    of both kinds in many pairs; in_order / reversed; one_address: rising timestamps; at_the_top: fields at 2^32 - 1;
    one_long_gap: 2999 dummies in one pair, more than a scan block; gaps_in_the_first_half and provable: the last gap, and so the
    padding, in the middle; no_gap; wide: every radix pass of all four fields runs (contexts and segments up to 2 10^7,
    timestamps below 2^32); the last three: degree_bits two above the need. The buffer is pre-filled with 0xFF bytes — an
    unwritten word shows —, guards and the gap of a padded pitch hold sentinels that must survive."""
    import plonky2_gpu_amd as pg

    exp, exp_rows = _reference(family, num_ops, extra_bits)
    n = exp.shape[1]
    degree_bits = n.bit_length() - 1
    buf = Strided(gpu, np.full((COLUMNS, n), ONES, dtype=np.uint64), n + pad)
    d_ops = pg.DeviceBuffer.from_host(gpu, _ops(family, num_ops))
    scratch = _scratch(gpu, num_ops, degree_bits)
    rows, err = _call(gpu, d_ops.ptr, num_ops, degree_bits, buf.ptr, n + pad, scratch.ptr)
    assert err is None and rows == exp_rows
    got = buf.polys((family, num_ops, pad, extra_bits))
    buf.free()
    assert (d_ops.download().reshape(num_ops, 14) == _ops(family, num_ops)).all()
    bad = np.argwhere(got != exp)
    assert bad.size == 0, ("first (column, row) that differs", bad[0].tolist(), len(bad), hex(int(got[tuple(bad[0])])), hex(int(exp[tuple(bad[0])])))


@pytest.mark.gpu
def test_generate_trace_and_rows_of_the_module(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import memory_table as mt

    w = _ops("mixed", 65)
    exp, exp_rows = _reference("mixed", 65)
    n = exp.shape[1]
    assert mt.rows(gpu, w) == exp_rows
    for stride in (None, n + 24):
        d = mt.generate_trace(gpu, w, trace_stride=stride)  # the count first, then the smallest trace
        assert d.rows == exp_rows and (d.download().reshape(COLUMNS, stride or n)[:, :n] == exp).all()
    d_ops = pg.DeviceBuffer.from_host(gpu, w)
    assert mt.rows(gpu, d_ops) == exp_rows
    exp2 = _reference("mixed", 65, 2)[0]
    assert (mt.generate_trace(gpu, d_ops, degree_bits=n.bit_length() + 1).download().reshape(COLUMNS, 4 * n) == exp2).all()


# ---------------------------------------------------------------- counting and refusals
@pytest.mark.gpu
@pytest.mark.parametrize("family,num_ops", [("small_keys", 2), ("mixed", 5), ("mixed", 2049), ("one_long_gap", 4), ("one_address", 257), ("wide", 65537)])
def test_rows_alone(gpu, family, num_ops):
    import plonky2_gpu_amd as pg

    d_ops = pg.DeviceBuffer.from_host(gpu, _ops(family, num_ops))
    scratch = _scratch(gpu, num_ops, 1)
    assert _call(gpu, d_ops.ptr, num_ops, 1, None, 0, scratch.ptr) == (_reference(family, num_ops)[1], None)


@pytest.mark.gpu
def test_two_operations_at_the_ends_of_the_address_space(gpu):
    """virtual addresses 0 and 2^32 - 1 under max_rc = 1: floor((2^32 - 2) / 2) = 2^31 - 1 dummies — the count of one pair needs 64
    bits once it is added to its position —, 2^31 + 1 rows. A count-only call reports them; with a trace the call is refused and
    still reports them."""
    import plonky2_gpu_amd as pg

    w = mi.words([1, 1], [1, 2], [0, 1], [0, 0], [0, 0], [(1 << 32) - 1, 0], np.ones((2, 8)))
    d_ops = pg.DeviceBuffer.from_host(gpu, w)
    scratch = _scratch(gpu, 2, 5)
    assert _call(gpu, d_ops.ptr, 2, 5, None, 0, scratch.ptr) == ((1 << 31) + 1, None)
    fill = np.full(COLUMNS * 32, ONES, dtype=np.uint64)
    trace = pg.DeviceBuffer.from_host(gpu, fill)
    rows, err = _call(gpu, d_ops.ptr, 2, 5, trace.ptr, 32, scratch.ptr)
    assert rows == (1 << 31) + 1 and err is not None and err.code == pg.GL_E_INVALID and "2147483649 rows" in str(err)
    gpu.synchronize()
    assert (trace.download() == fill).all()


@pytest.mark.gpu
def test_data_refusals_write_nothing_and_name_their_reason(gpu):
    import plonky2_gpu_amd as pg

    fill = np.full(COLUMNS * 8, ONES, dtype=np.uint64)
    trace = pg.DeviceBuffer.from_host(gpu, fill)

    def refused(w, degree_bits):
        d_ops = pg.DeviceBuffer.from_host(gpu, w)
        scratch = _scratch(gpu, len(w), degree_bits)
        rows, err = _call(gpu, d_ops.ptr, len(w), degree_bits, trace.ptr, 1 << degree_bits, scratch.ptr)
        assert err is not None and err.code == pg.GL_E_INVALID
        gpu.synchronize()
        assert (trace.download() == fill).all()
        return rows, str(err)

    base = dict(filter_=[1, 1], timestamp=[1, 2], is_read=[0, 1], context=[0, 0], segment=[0, 0], virt=[0, 1], values=np.ones((2, 8)))
    rows, why = refused(mi.words(**{**base, "virt": [0, 9]}), 1)  # max_rc 1: dummies at 2, 4, 6, 8
    assert rows == 6 and "6 rows" in why and "2^degree_bits" in why
    rows, why = refused(mi.words(**{**base, "timestamp": [1, 1 << 32]}), 1)
    assert rows == 0 and "2^32 or more" in why
    rows, why = refused(mi.words(**{**base, "values": np.full((2, 8), 1 << 32)}), 1)
    assert rows == 0 and "2^32 or more" in why
    rows, why = refused(mi.words(**{**base, "filter_": [1, 2]}), 1)
    assert rows == 0 and "neither 0 nor 1" in why
    rows, why = refused(mi.words(**{**base, "is_read": [ONES, 1]}), 1)
    assert rows == 0 and "neither 0 nor 1" in why
    rows, why = refused(mi.words(**{**base, "context": [6, 0]}), 1)  # the range check would be 5 in a 2-row trace
    assert rows == 2 and "context or segment gap" in why
    rows, why = refused(mi.words(**{**base, "segment": [0, 3]}), 1)  # 2 is no range check of a 2-row trace either
    assert rows == 2 and "context or segment gap" in why
    # ... and in a trace of 8 rows both are fine
    for change, rc in (({"context": [6, 0]}, 5), ({"segment": [0, 3]}, 2)):
        w = mi.words(**{**base, **change})
        d_ops, scratch = pg.DeviceBuffer.from_host(gpu, w), _scratch(gpu, 2, 3)
        assert _call(gpu, d_ops.ptr, 2, 3, trace.ptr, 8, scratch.ptr) == (2, None)
        got = trace.download().reshape(COLUMNS, 8)
        assert (got == mr.trace_of_words(w, 3)[0]).all() and got[mr.RANGE_CHECK, 0] == rc


@pytest.mark.gpu
def test_argument_refusals_launch_nothing(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    num_ops, n = 10, 32
    w = _ops("provable", 10)
    scratch_words = _lib.load().gl_memory_table_scratch_bytes(num_ops, 5) // 8
    fill = np.full(COLUMNS * n + 14 * num_ops + scratch_words, ONES, dtype=np.uint64)
    fill[COLUMNS * n : COLUMNS * n + 14 * num_ops] = w.reshape(-1)
    buf = pg.DeviceBuffer.from_host(gpu, fill)  # a trace, behind it the operations, behind them the scratch
    d_ops, d_scratch = buf.at(COLUMNS * n), buf.at(COLUMNS * n + 14 * num_ops)
    assert d_scratch % 16 == 0

    def refused(*args):
        rows, err = _call(gpu, *args)
        assert err is not None and err.code == pg.GL_E_INVALID and rows == ONES  # *h_rows is not written either
        return str(err)

    assert "degree_bits" in refused(d_ops, num_ops, 0, buf.ptr, n, d_scratch)
    assert "degree_bits" in refused(d_ops, num_ops, 24, buf.ptr, 1 << 24, d_scratch)
    assert "num_ops" in refused(d_ops, 1, 5, buf.ptr, n, d_scratch)
    assert "num_ops" in refused(d_ops, (1 << 30) + 1, 5, buf.ptr, n, d_scratch)
    assert "trace_stride" in refused(d_ops, num_ops, 5, buf.ptr, n - 1, d_scratch)
    assert "null pointer" in refused(None, num_ops, 5, buf.ptr, n, d_scratch)
    assert "null pointer" in refused(d_ops, num_ops, 5, buf.ptr, n, None)
    assert "aligned" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch + 8)
    assert "d_trace overlaps d_ops" in refused(buf.at(COLUMNS * n - 1), num_ops, 5, buf.ptr, n, d_scratch)  # its first word is the trace's last
    assert "d_trace overlaps d_ops" in refused(buf.at(5), num_ops, 5, buf.ptr, n, d_scratch)
    assert "d_scratch overlaps d_ops" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch - 16)
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, 5, buf.at(COLUMNS * n + 14 * num_ops + 2), n, d_scratch)
    assert _lib.load().gl_memory_table_scratch_bytes(1, 5) == 0 and _lib.load().gl_memory_table_scratch_bytes(2, 24) == 0
    import ctypes

    with pytest.raises(pg.Plonky2HipError, match="null pointer"):
        _lib.call("gl_memory_table_trace", d_ops, num_ops, 5, buf.ptr, n, d_scratch, ctypes.POINTER(ctypes.c_uint64)(), gpu.ptr)
    gpu.synchronize()
    assert (buf.download() == fill).all()
    assert _call(gpu, d_ops, num_ops, 5, buf.ptr, n, d_scratch) == (18, None)  # the same buffers, accepted
    assert (buf.download(0, COLUMNS * n).reshape(COLUMNS, n) == _reference("provable", 10)[0]).all()


# ---------------------------------------------------------------- proofs
FP = th.FP
PROVABLE = {32: ("provable", 10, 0), 64: ("provable", 13, 1)}  # 18 rows in 32; 21 rows in 64 (one bit above the need)


@functools.lru_cache(maxsize=None)
def _provable_reference(n):
    cols = _reference(*PROVABLE[n])[0]
    assert cols.shape == (COLUMNS, n) and mr.satisfies_its_constraints(cols)  # on the CPU first: only some inputs are provable
    return cols


TABLE = th.Table("memory_table", mr.MemoryTableStark, COLUMNS, (32, 64), reference_trace=_provable_reference,
                 device_trace=lambda ctx, n: TABLE.module.generate_trace(ctx, _ops(*PROVABLE[n][:2]), degree_bits=n.bit_length() - 1),
                 flip=lambda mt: (mt.value_limb(2), 1))
_stark, _reference_proof, _device_trace = TABLE.stark, TABLE.reference_proof, TABLE.device_trace


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("hasher,num_challenges", [("poseidon", 1), ("poseidon", 2), ("keccak", 1), ("keccak", 3)])
def test_proof_bytes_of_the_device_built_trace_equal_the_reference(gpu, hasher, num_challenges, n):
    """Keccak with 2 challenges would have quotient leaves of 4 elements, which KeccakHash<25> cannot hash (the reference panics): 1
    and 3 there. The padding rows stand in the middle of both traces."""
    th.check_proof_bytes(TABLE, gpu, hasher, num_challenges, n)


@pytest.mark.gpu
def test_the_compiled_kernel_gives_the_same_bytes(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import memory_table as mt

    exp = _reference_proof("poseidon", 2, 32)
    ns = pg.NativeStark(gpu, mt.stark_desc(5, 2, FP), compiled=True)
    try:
        assert ns.is_compiled
        assert ns.prove_bytes(_device_trace(gpu, 32), []) == exp
    finally:
        ns.close()


@pytest.mark.gpu
def test_quotient_polys_on_random_words_equal_the_reference(gpu):
    """uniformly random words in place of the LDEs of the trace and of the two permutation Zs (every constraint non-zero), at the
    tight and at a padded column pitch"""
    rng = np.random.default_rng(2226)
    lde = rng.integers(0, P, size=(COLUMNS, 64), dtype=np.uint64)
    zs = rng.integers(0, P, size=(2, 64), dtype=np.uint64)
    alphas = [int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)]
    sets = [[tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)) for _ in range(2)] for _ in range(2)]
    th.check_quotient_polys(TABLE, gpu, lde, alphas, zs, sets)


@pytest.mark.gpu
def test_a_flipped_value_limb_gives_a_proof_the_verifier_rejects(gpu):
    """row 1 is the read of address 0 behind its write: with another limb the value constraints of rows 0 and 1 fail.
    quotient_degree_factor 2 is a power of two: the reference's trim cannot fail, its prover returns a proof of the violated trace,
    and verification fails at zeta. The device does the same."""
    column, row = TABLE.flip(TABLE.module)
    assert _provable_reference(32)[TABLE.module.IS_READ, row] == 1
    th.check_flipped_cell_is_rejected(TABLE, gpu, "stark_ref")


# ---------------------------------------------------------------- two tables and the cross-table lookup
class _Cpu:
    """the 14-column stand-in for the table that issues the operations: the 13 CTL columns and a 0 / 1 filter f with f (f - 1) = 0"""
    num_columns, num_public_inputs, constraint_degree, pairs = 14, 0, 3, []

    def __init__(self):
        from plonky2_gpu_amd.stark import StarkAsm

        a = StarkAsm()
        f = a.local(13)
        a.emit(a.mul(f, a.sub(f, a.imm(1))))
        self.instrs, self.immediates = a.program()

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        consumer.constraint(F.mul(local[13], F.sub(local[13], F.one)))


@pytest.mark.gpu
def test_two_tables_with_the_memory_lookup_equal_the_reference(gpu):
    """14 operations in list order with filter 1 and two rows of filter 0 (one of zeros, one of sevens) in the 16 rows of the looking
    table; the memory table, 32 rows built on the device from the same list, is the looked table with ctl_filter(): its 22 - 14
    dummies and its 10 padding rows have filter 0. One lookup over 13 columns with filters on both sides."""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import memory_table as mt
    from plonky2_gpu_amd import stark as pstark
    from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, StarkDesc, StarkTablesDesc, TableWithColumns

    w = _ops("provable", 14)
    cols, rows = _reference("provable", 14)
    assert rows == 22 and cols.shape == (COLUMNS, 32) and mr.satisfies_its_constraints(cols)
    order = [mr.IS_READ, mr.ADDR_CONTEXT, mr.ADDR_SEGMENT, mr.ADDR_VIRTUAL] + [mr.value_limb(i) for i in range(8)] + [mr.TIMESTAMP]
    cpu_rows = [[int(op[c]) for c in order] + [1] for op in w] + [[0] * 14, [7] * 13 + [0]]
    cpu_trace = [[r[c] for r in cpu_rows] for c in range(14)]
    cpu = _Cpu()
    lookups = [CrossTableLookup([TableWithColumns(0, [CtlColumn.single(c) for c in range(13)], CtlColumn.single(13))],
                                TableWithColumns(1, mt.ctl_data(), mt.ctl_filter()))]
    fps = [si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,), num_query_rounds=4, proof_of_work_bits=2) for _ in range(2)]
    system = th.System([cpu, _stark()], lookups)
    with accel.c_backend():
        exp = cr.proofs_bytes(HASHERS["poseidon"], cr.prove_tables(HASHERS["poseidon"], system, 1, fps, [cpu_trace, [[int(v) for v in col] for col in cols]]))
    desc = StarkTablesDesc([StarkDesc(4, 14, 0, 3, 1, fps[0], cpu.instrs, cpu.immediates), mt.stark_desc(5, 1, fps[1])], lookups)
    desc.validate()
    nt = pg.NativeStarkTables(gpu, desc)
    try:
        data = nt.prove_bytes([cpu_trace, mt.generate_trace(gpu, w)])
    finally:
        nt.close()
    assert data == exp
    with accel.c_backend():
        assert cr.verify_tables(HASHERS["poseidon"], system, 1, fps, pstark.tables_proof_from_bytes(data, desc))


# ---------------------------------------------------------------- two contexts, two threads
@pytest.mark.gpu
def test_two_contexts_on_two_threads_build_and_prove(gpu):
    th.check_two_contexts_on_two_threads(TABLE, gpu)
