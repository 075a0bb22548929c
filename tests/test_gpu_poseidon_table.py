"""The Poseidon table on the device: gl_poseidon_table_trace against tests/poseidon_table_ref.py's restatement of
generate_permutation_unit on all 249 columns, its refusals, and the table proved by gl_stark_prove / gl_stark_tables_prove from
the device-built trace against tests/stark_ref.py and tests/ctl_ref.py, byte for byte: there is no tolerance anywhere.

The shapes cross the edges of the kernels as built: no record, 1 and 2 in the smallest trace (a trace far smaller than a wave:
the rows kernel keeps its waves whole and clamps), 3, 63 / 64 / 65 (the wave edge on both sides), 255 and 257 (a 256-thread
workgroup; one row beyond), 2049 (more than one workgroup; with one_run the serial pass crosses workgroups). Every shape runs at
the tight pitch, at an even padded pitch and at an odd one."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref as cr  # noqa: E402
import poseidon_table_instances as pi  # noqa: E402
import poseidon_table_ref as pr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
import table_harness as th  # noqa: E402
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = 0xFFFFFFFF00000001
ONES = (1 << 64) - 1
HASHERS = th.HASHERS
COLUMNS = 249
OPW = 13


# ---------------------------------------------------------------- instances and reference traces
@functools.lru_cache(maxsize=None)
def _ops(num_ops, family="mixed"):
    w = pi.FAMILIES[family](num_ops)
    assert w.shape == (num_ops, OPW)
    w.setflags(write=False)
    return w


def _reference_of(words, degree_bits):
    cols = pr.trace_of_words(words, degree_bits)
    assert cols.shape == (COLUMNS, 1 << degree_bits)
    cols.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def _reference(num_ops, degree_bits, family="mixed"):
    """[249][2^degree_bits] columns; never changed"""
    return _reference_of(_ops(num_ops, family), degree_bits)


def _call(gpu, d_ops, num_ops, degree_bits, d_trace, stride, d_scratch):
    """gl_poseidon_table_trace; None or the error"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    try:
        _lib.call("gl_poseidon_table_trace", d_ops, num_ops, degree_bits, d_trace, stride, d_scratch, gpu.ptr)
    except pg.Plonky2HipError as e:
        return e
    return None


def _built(gpu, words, degree_bits, pad=0):
    """the trace of `words` in a buffer pre-filled with 0xFF bytes — an unwritten word shows —, guards and the gap of a padded pitch
    hold sentinels that must survive; the records are left as they were"""
    import plonky2_gpu_amd as pg

    n, num_ops = 1 << degree_bits, len(words)
    buf = Strided(gpu, np.full((COLUMNS, n), ONES, dtype=np.uint64), n + pad)
    d_ops = pg.DeviceBuffer.from_host(gpu, words) if num_ops else None
    scratch = pg.DeviceBuffer(gpu, 2)
    assert _call(gpu, d_ops.ptr if d_ops else None, num_ops, degree_bits, buf.ptr, n + pad, scratch.ptr) is None
    got = buf.polys((num_ops, degree_bits, pad))
    buf.free()
    if d_ops:
        assert (d_ops.download().reshape(num_ops, OPW) == words).all()
    return got


SHAPES = [(0, 1), (1, 1), (2, 1), (3, 2), (63, 6), (64, 6), (65, 7), (255, 8), (257, 9), (2049, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 24, 25])
@pytest.mark.parametrize("num_ops,degree_bits", SHAPES)
def test_trace_equals_generate_permutation_unit(gpu, num_ops, degree_bits, pad):
    exp = _reference(num_ops, degree_bits)
    assert degree_bits == max(1, (max(num_ops, 1) - 1).bit_length())
    assert th.first_difference(_built(gpu, _ops(num_ops), degree_bits, pad), exp) is None


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 24, 25])
@pytest.mark.parametrize("family", ["starts", "pairs", "leaves135", "one_run", "noncanonical"])
def test_every_other_family_at_a_workgroup_and_one_row(gpu, family, pad):
    assert th.first_difference(_built(gpu, _ops(257, family), 9, pad), _reference(257, 9, family)) is None


@pytest.mark.gpu
def test_one_run_puts_the_serial_pass_across_workgroups(gpu):
    assert th.first_difference(_built(gpu, _ops(2049, "one_run"), 12), _reference(2049, 12, "one_run")) is None


@pytest.mark.gpu
def test_generate_trace_of_the_module(gpu):
    """host words at the smallest height, then a padded pitch from a DeviceBuffer of the words, a height above the need, and the
    all-padding trace of no records"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import poseidon_table as pt

    w, exp = _ops(65), _reference(65, 7)
    assert th.first_difference(pt.generate_trace(gpu, w).download().reshape(COLUMNS, 128), exp) is None
    d_ops = pg.DeviceBuffer.from_host(gpu, w)
    got = pt.generate_trace(gpu, d_ops, trace_stride=128 + 24).download().reshape(COLUMNS, 152)[:, :128]
    assert th.first_difference(got, exp) is None
    wide = pt.generate_trace(gpu, w, degree_bits=8).download().reshape(COLUMNS, 256)
    assert th.first_difference(wide, _reference_of(w, 8)) is None
    empty = pt.generate_trace(gpu, pt.ops_to_words([])).download().reshape(COLUMNS, 2)
    assert th.first_difference(empty, _reference(0, 1)) is None and empty[236:248].all() and not empty[248].any()


def _stage_ms(gpu, words, degree_bits, mds=0):
    """gl_debug_poseidon_table_stage_ms -> (the trace, the three stage times)"""
    import ctypes

    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    n = 1 << degree_bits
    d_ops, scratch = pg.DeviceBuffer.from_host(gpu, words), pg.DeviceBuffer(gpu, 2)
    trace = pg.DeviceBuffer.from_host(gpu, np.full(COLUMNS * n, ONES, dtype=np.uint64))
    ms = (ctypes.c_float * 3)()
    _lib.call("gl_debug_poseidon_table_stage_ms", d_ops.ptr, len(words), degree_bits, trace.ptr, n, scratch.ptr, mds, ms, gpu.ptr)
    return trace.download().reshape(COLUMNS, n), list(ms)


@pytest.mark.gpu
def test_a_list_without_an_absorb_skips_the_serial_pass(gpu):
    """an all-START list and the same list with one ABSORB appended give equal rows where they share records; the first does not
    run stage 2, the second does"""
    w = _ops(300, "starts")
    longer = np.concatenate([w, _ops(20)[1:2]])
    assert longer[-1, 0] == 1 and not longer[:-1, 0].any()
    short_trace, short_ms = _stage_ms(gpu, w, 9)
    long_trace, long_ms = _stage_ms(gpu, longer, 9)
    assert short_ms[0] >= 0 and short_ms[1] < 0 and short_ms[2] > 0  # negative: not run
    assert all(v >= 0 for v in long_ms) and long_ms[2] > 0
    assert th.first_difference(short_trace, _reference(300, 9, "starts")) is None
    assert th.first_difference(long_trace, _reference_of(longer, 9)) is None
    assert (short_trace[:, :300] == long_trace[:, :300]).all() and (short_trace[:, 301:] == long_trace[:, 301:]).all()
    assert th.first_difference(_built(gpu, w, 9), short_trace) is None  # gl_poseidon_table_trace takes the same path


@pytest.mark.gpu
@pytest.mark.parametrize("mds", [1, 2])
@pytest.mark.parametrize("family", ["mixed", "noncanonical"])
def test_both_mds_variants_of_the_rows_kernel_write_the_same_trace(gpu, family, mds):
    """mds 1: the layers on the matrix cores, 2: on the vector ALU; 300 records and 212 padding rows"""
    got, _ = _stage_ms(gpu, _ops(300, family), 9, mds)
    assert th.first_difference(got, _reference(300, 9, family)) is None


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [2048, 2047])
def test_padding_after_a_run(gpu, cut):
    """mixed(2049) cut to the 2048 records of a full 2^11 trace and to one short of it; a prefix only shortens its last run, and
    its rows are the rows of the whole list (tests/test_poseidon_table_ref.py holds that), so the reference is cut with it.
    Records 2045 .. 2048 of the list are a START and three ABSORBs: either cut ends on an ABSORB, nothing has to be appended.
    A run ends exactly on the last row; a run ends one row before padding begins."""
    w = _ops(2049)[:cut]
    assert w[-1, 0] != 0 and w[2045, 0] == 0  # a run of more than one row ends on the last record
    exp = np.concatenate([_reference(2049, 12)[:, :cut], _reference(0, 1)[:, : 2048 - cut]], axis=1)
    assert exp.shape == (COLUMNS, 2048) and exp[248].tolist() == [1] * cut + [0] * (2048 - cut)
    assert th.first_difference(_built(gpu, w, 11), exp) is None


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
    w[[290, 37], 0] = 9
    why = refused(w)
    assert "the kind of record 37 is not 0 (START) or 1 .. 8 (ABSORB)" in why and "290" not in why
    w = _ops(num_ops).copy()
    w[299, 0] = 1 << 32  # a kind word is not cut to 32 bits
    assert "the kind of record 299 " in refused(w)
    w = _ops(num_ops).copy()
    w[260, 0] = ONES
    assert "the kind of record 260 " in refused(w)
    w = _ops(num_ops).copy()
    w[0, 0] = 5
    assert "record 0 is an ABSORB: it continues a sponge that no record starts" in refused(w)
    w[77, 0] = 9  # record 0 is the lower one
    assert "record 0 is an ABSORB" in refused(w)
    w[0, 0] = 9  # ... and with a kind above 8 it is no ABSORB
    assert "the kind of record 0 " in refused(w)
    # ... and the same buffers take the untouched list
    d_ops = pg.DeviceBuffer.from_host(gpu, _ops(num_ops))
    assert _call(gpu, d_ops.ptr, num_ops, 9, trace.ptr, n, scratch.ptr) is None
    assert th.first_difference(trace.download().reshape(COLUMNS, n), _reference(num_ops, 9)) is None


@pytest.mark.gpu
def test_argument_refusals_launch_nothing(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    num_ops, n = 10, 32
    w = _ops(num_ops)
    fill = np.full(COLUMNS * n + OPW * num_ops + 2, ONES, dtype=np.uint64)
    fill[COLUMNS * n : COLUMNS * n + OPW * num_ops] = w.reshape(-1)
    buf = pg.DeviceBuffer.from_host(gpu, fill)  # a trace, behind it the records, behind them the scratch
    d_ops, d_scratch = buf.at(COLUMNS * n), buf.at(COLUMNS * n + OPW * num_ops)
    assert d_scratch % 16 == 0

    def refused(*args):
        err = _call(gpu, *args)
        assert err is not None and err.code == pg.GL_E_INVALID
        return str(err)

    assert "degree_bits must be in 1 ..= 23" in refused(d_ops, num_ops, 0, buf.ptr, n, d_scratch)
    assert "degree_bits must be in 1 ..= 23" in refused(d_ops, num_ops, 24, buf.ptr, 1 << 24, d_scratch)
    assert "num_ops exceeds the 2^degree_bits rows of the trace" in refused(d_ops, n + 1, 5, buf.ptr, n, d_scratch)
    assert "num_ops exceeds" in refused(d_ops, 3, 1, buf.ptr, n, d_scratch)
    assert "trace_stride smaller than 2^degree_bits" in refused(d_ops, num_ops, 5, buf.ptr, n - 1, d_scratch)
    assert "trace_stride too large" in refused(d_ops, num_ops, 5, buf.ptr, (1 << 40) + 1, d_scratch)
    assert "null pointer" in refused(None, num_ops, 5, buf.ptr, n, d_scratch)
    assert "null pointer" in refused(d_ops, num_ops, 5, None, n, d_scratch)
    assert "null pointer" in refused(d_ops, num_ops, 5, buf.ptr, n, None)
    assert "null pointer" in refused(None, 0, 5, buf.ptr, n, None)  # without records the scratch is still asked for
    assert "d_scratch must be 16-byte aligned" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch + 8)
    assert "d_trace overlaps d_ops" in refused(buf.at(COLUMNS * n - 1), num_ops, 5, buf.ptr, n, d_scratch)  # its first word is the trace's last
    assert "d_trace overlaps d_ops" in refused(buf.at(5), num_ops, 5, buf.ptr, n, d_scratch)
    assert "d_scratch overlaps d_ops" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch - 16)
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, 5, buf.ptr, n, buf.at(COLUMNS * n - 2))  # the trace's last two words
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, 5, buf.ptr, n, buf.at(4))
    with pytest.raises(pg.Plonky2HipError, match="null pointer"):
        _lib.call("gl_poseidon_table_trace", d_ops, num_ops, 5, buf.ptr, n, d_scratch, None)
    gpu.synchronize()
    assert (buf.download() == fill).all()
    assert _call(gpu, d_ops, num_ops, 5, buf.ptr, n, d_scratch) is None  # the same buffers, accepted
    assert (buf.download(0, COLUMNS * n).reshape(COLUMNS, n) == _reference(num_ops, 5)).all()
    assert (buf.download(COLUMNS * n, OPW * num_ops) == fill[COLUMNS * n : COLUMNS * n + OPW * num_ops]).all()
    assert _call(gpu, None, 0, 5, buf.ptr, n, d_scratch) is None  # no records, no list
    assert (buf.download(0, COLUMNS * n).reshape(COLUMNS, n) == _reference(0, 5)).all()


# ---------------------------------------------------------------- proofs
FP = th.FP
UNIT_INSTRS = 8192  # above the program's length: one unit
TABLE = th.Table("poseidon_table", pr.PoseidonTableStark, COLUMNS, (32,), reference_trace=lambda n: _reference(20, n.bit_length() - 1),
                 device_trace=lambda ctx, n: TABLE.module.generate_trace(ctx, _ops(20), degree_bits=n.bit_length() - 1),
                 flip=lambda pt: (pt.col_partial_after_sbox(11), 7))


@pytest.mark.gpu
@pytest.mark.parametrize("hasher,num_challenges", [("poseidon", 2), ("keccak", 1)])
def test_proof_bytes_of_the_device_built_trace_equal_the_reference(gpu, hasher, num_challenges):
    """2^5 rows, 20 records, interpreted. Keccak with 2 challenges would have quotient leaves of 4 elements, which KeccakHash<25>
    cannot hash (the reference panics): 1 there."""
    th.check_proof_bytes(TABLE, gpu, hasher, num_challenges, 32, verify="closure")


@pytest.mark.gpu
def test_compiled_in_units_gives_the_same_bytes(gpu):
    """unit_instrs=8192: the whole program (6 627 instructions) as ONE unit, a cold compile of about ten seconds. The state of the
    permutation runs through all 237 constraints, so a unit has to re-derive it from the columns: at the library's cap
    (unit_instrs=0) split_program cuts this program into 58 units of up to 3 800 instructions, whose cold compile took 200 s
    (DESIGN.md §3.7.9). num_units is what split_program cuts the program into."""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import poseidon_table as pt
    from plonky2_gpu_amd import stark as pstark

    exp = TABLE.reference_proof("poseidon", 2, 32)
    desc = pt.stark_desc(5, 2, FP)
    program_units = len(pstark.split_program(desc, UNIT_INSTRS))
    assert program_units == 1 < len(pstark.split_program(desc, 0))
    ns = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=UNIT_INSTRS)
    try:
        assert ns.is_compiled and ns.num_units == program_units
        assert ns.prove_bytes(TABLE.device_trace(gpu, 32), []) == exp
    finally:
        ns.close()


@pytest.mark.gpu
def test_a_flipped_cell_gives_a_proof_the_verifier_rejects(gpu):
    th.check_flipped_cell_is_rejected(TABLE, gpu, "stark_verify")


# ---------------------------------------------------------------- the lookup: a plain looker of (input, output) pairs
PAIR, F_PAIR, LOOKER_COLUMNS = 0, 24, 25


class _Looker:
    """the 25-column stand-in for a table that hashes: per row an (input, output) pair of a permutation in columns 0 .. 23 under
    the filter of column 24. Its own constraint: the filter is boolean."""
    num_columns, num_public_inputs, constraint_degree, pairs = LOOKER_COLUMNS, 0, 3, []

    def __init__(self):
        from plonky2_gpu_amd.stark import StarkAsm

        a = StarkAsm()
        f = a.local(F_PAIR)
        a.emit(a.mul(f, a.sub(f, a.imm(1))))
        self.instrs, self.immediates = a.program()

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        consumer.constraint(F.mul(local[F_PAIR], F.sub(local[F_PAIR], F.one)))


@functools.lru_cache(maxsize=None)
def _lookup_system():
    """(looker trace [25][32], lookups): the 20 (input, output) pairs of mixed(20) in REVERSED order from row 0; the other rows
    carry sevens under a filter of 0"""
    from plonky2_gpu_amd import poseidon_table as pt
    from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, TableWithColumns

    cols = _reference(20, 5)
    rows = np.full((32, LOOKER_COLUMNS), 7, dtype=np.uint64)
    rows[:, F_PAIR] = 0
    for r in range(20):
        rows[19 - r, PAIR : PAIR + 12], rows[19 - r, PAIR + 12 : PAIR + 24], rows[19 - r, F_PAIR] = cols[0:12, r], cols[236:248, r], 1
    lookups = [CrossTableLookup([TableWithColumns(0, [CtlColumn.single(PAIR + k) for k in range(24)], CtlColumn.single(F_PAIR))],
                                TableWithColumns(1, pt.ctl_data(), pt.ctl_filter()))]
    return [[int(v) for v in col] for col in rows.T], lookups


@pytest.mark.gpu
@pytest.mark.parametrize("hasher,num_challenges", [("poseidon", 2), ("keccak", 1)])
def test_a_looker_of_reversed_pairs_with_the_permutation_lookup_equals_the_reference(gpu, hasher, num_challenges):
    """The Poseidon table, 32 rows built on the device from 20 records, is looked with ctl_filter() = IS_REAL: its 12 padding rows
    have filter 0. One lookup over 24 columns. Keccak with 2 challenges would give both tables 4 quotient polynomials: 1 there."""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import poseidon_table as pt
    from plonky2_gpu_amd import stark as pstark
    from plonky2_gpu_amd.stark import StarkDesc, StarkTablesDesc

    looker_trace, lookups = _lookup_system()
    cols = _reference(20, 5)
    looker = _Looker()
    fps = [si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,), num_query_rounds=4, proof_of_work_bits=2) for _ in range(2)]
    system = th.System([looker, TABLE.stark()], lookups)
    with accel.c_backend():
        exp = cr.proofs_bytes(HASHERS[hasher], cr.prove_tables(HASHERS[hasher], system, num_challenges, fps,
                                                               [looker_trace, [[int(v) for v in col] for col in cols]]))
    desc = StarkTablesDesc([StarkDesc(5, LOOKER_COLUMNS, 0, 3, num_challenges, fps[0], looker.instrs, looker.immediates),
                            pt.stark_desc(5, num_challenges, fps[1])], lookups)
    desc.validate(hasher)
    nt = pg.NativeStarkTables(gpu, desc, hasher)
    try:
        data = nt.prove_bytes([looker_trace, pt.generate_trace(gpu, _ops(20), degree_bits=5)])
    finally:
        nt.close()
    assert data == exp
    with accel.c_backend():
        assert cr.verify_tables(HASHERS[hasher], system, num_challenges, fps, pstark.tables_proof_from_bytes(data, desc, hasher))


# ---------------------------------------------------------------- two contexts, two threads
@pytest.mark.gpu
def test_two_contexts_on_two_threads_build_and_prove(gpu):
    th.check_two_contexts_on_two_threads(TABLE, gpu)
