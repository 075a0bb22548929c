"""The arithmetic table on the device: gl_arithmetic_table_trace against tests/arithmetic_table_ref.py's restatement of the
reference's generate functions on all 92 columns, its refusals, and the table proved by gl_stark_prove / gl_stark_tables_prove from
the device-built trace against tests/stark_ref.py and tests/ctl_ref.py, byte for byte: there is no tolerance anywhere.

The shapes cross the edges of the kernels as built: 1 operation, 63 / 64 / 65 (a wave of the fill, which is one lane per operation
in workgroups of 64, and one beyond), 257 (a 256-thread workgroup of the counting pass and one beyond), and LOOKUP_SCAN_BLOCK and
one more (the scan runs over num_ops + 1 counts: one word and two words into its second block). The lists interleave one- and
two-row operators, so a lane's first row depends on the scan. The edge list takes every branch of the division
(tests/test_arithmetic_table_ref.py shows that on the model).

The proofs bring their own FRI parameters: a trace with a DIV row needs constraint_degree 5, quotient_degree_factor 4 and
rate_bits 2 (tests/table_harness.py fixes rate_bits 1). KeccakHash<25> cannot hash a Merkle leaf of four elements, which is what
degree 5 with ONE challenge gives the quotient: Keccak proves the DIV trace with 2 challenges, and with 1 challenge a trace without
DIV rows at the reference's declared degree 3."""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arithmetic_table_instances as ai  # noqa: E402
import arithmetic_table_ref as ar  # noqa: E402
import ctl_ref as cr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
import table_harness as th  # noqa: E402
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = 0xFFFFFFFF00000001
ONES = (1 << 64) - 1
HASHERS = th.HASHERS
COLUMNS, W = 92, 25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_BLOCK = int(re.search(r"constexpr uint32_t LOOKUP_SCAN_BLOCK = (\d+);", open(os.path.join(ROOT, "plonky2_gpu_amd", "csrc", "lookup.h")).read()).group(1))


# ---------------------------------------------------------------- instances and reference traces
@functools.lru_cache(maxsize=None)
def _ops(name, *args):
    w = getattr(ai, name)(*args)
    assert w.shape[1] == W
    w.setflags(write=False)
    return w


def _bits(rows):
    return max(1, (max(rows, 1) - 1).bit_length())


@functools.lru_cache(maxsize=None)
def _reference(name, *args, degree_bits=None):
    """[92][n] columns, n the smallest trace that holds the operations unless degree_bits says otherwise; never changed"""
    cols = ar.trace_of_words(_ops(name, *args), degree_bits)
    cols.setflags(write=False)
    return cols


def _call(gpu, d_ops, num_ops, degree_bits, d_trace, stride, d_scratch, ctx=True):
    """gl_arithmetic_table_trace: (None or the error, *h_rows)"""
    import ctypes

    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    rows = ctypes.c_uint64(12345)
    try:
        _lib.call("gl_arithmetic_table_trace", d_ops, num_ops, degree_bits, d_trace, stride, d_scratch, ctypes.byref(rows), gpu.ptr if ctx else None)
    except pg.Plonky2HipError as e:
        return e, int(rows.value)
    return None, int(rows.value)


def _scratch(gpu, num_ops, degree_bits):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    size = _lib.load().gl_arithmetic_table_scratch_bytes(num_ops, degree_bits)
    assert size and size % 16 == 0
    return pg.DeviceBuffer(gpu, size // 8)


def _build(gpu, w, degree_bits, pad=0):
    """the trace of the words `w` on a buffer pre-filled with ones, guards and pads checked: ([92][n], rows)"""
    import plonky2_gpu_amd as pg

    n = 1 << degree_bits
    buf = Strided(gpu, np.full((COLUMNS, n), ONES, dtype=np.uint64), n + pad)
    d_ops = pg.DeviceBuffer.from_host(gpu, w) if len(w) else None
    scratch = _scratch(gpu, len(w), degree_bits)
    err, rows = _call(gpu, d_ops.ptr if d_ops else None, len(w), degree_bits, buf.ptr, n + pad, scratch.ptr)
    assert err is None, err
    got = buf.polys((len(w), degree_bits, pad))  # the download waits for the fill: the scratch may go behind it
    buf.free()
    if d_ops:
        assert (d_ops.download().reshape(-1, W) == w).all()  # the operations are left as they were
    return got, rows


# ---------------------------------------------------------------- the trace
@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 24, 25])
@pytest.mark.parametrize("num_ops", [1, 63, 64, 65, 257, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_trace_equals_the_restatement(gpu, num_ops, pad):
    """one- and two-row operators interleaved, at the tight pitch and at two padded ones; the buffer is pre-filled with ones — an
    unwritten word shows —, guards and the gap of a padded pitch hold sentinels that must survive"""
    w, exp = _ops("mixed", num_ops), _reference("mixed", num_ops)
    rows = ar.num_rows(w)
    assert exp.shape[1] == 1 << _bits(rows) and rows > num_ops - (num_ops == 1)
    got, got_rows = _build(gpu, w, _bits(rows), pad)
    assert got_rows == rows
    assert th.first_difference(got, exp) is None


@pytest.mark.gpu
def test_the_edge_list_with_every_branch_of_the_division(gpu):
    """operands 0, 1, 2^256 - 1, single set limbs, rippling carries, moduli 0, 1, 2^256 - 1 and of 1 .. 16 limbs, the 512-bit
    quotient, negative quotients, and the operands found for the division's rare branches"""
    w, exp = _ops("edge"), _reference("edge")
    got, rows = _build(gpu, w, _bits(ar.num_rows(w)))
    assert rows == ar.num_rows(w)
    assert th.first_difference(got, exp) is None


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["random_ops", "add_only", "mulmod_only"])
def test_generate_trace_of_the_module_on_every_family(gpu, family):
    """65 operations through arithmetic_table.generate_trace: host words at the smallest height (the module asks for the count
    first), then a larger trace at a padded pitch from a DeviceBuffer of the words"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import arithmetic_table as at

    w, exp = _ops(family, 65), _reference(family, 65)
    n = exp.shape[1]
    d = at.generate_trace(gpu, w)
    assert d.rows == ar.num_rows(w)
    assert th.first_difference(d.download().reshape(COLUMNS, n), exp) is None
    d_ops = pg.DeviceBuffer.from_host(gpu, w)
    wide = _reference(family, 65, degree_bits=8)
    got = at.generate_trace(gpu, d_ops, degree_bits=8, trace_stride=256 + 24).download().reshape(COLUMNS, 280)[:, :256]
    assert th.first_difference(got, wide) is None
    assert at.rows(gpu, d_ops) == ar.num_rows(w)


@pytest.mark.gpu
def test_rows_fill_the_trace_to_its_last_row_and_one_more_is_refused(gpu):
    """2 ADD + 7 MOD: 16 rows, the last MOD's second row on row n - 1; one more ADD: 17 rows, refused with the count and the trace
    untouched; the count-only call; no operations"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import arithmetic_table as at

    ops = [(ai.ADD, 5, 6, 0), (ai.ADD, ai.MAX, 1, 0)] + [(ai.MOD, ai.MAX - k, 0, (1 << (30 * k + 1)) + k) for k in range(7)]
    w = ai.words(ops)
    exp = ar.trace_of_words(w)
    assert exp.shape == (COLUMNS, 16) and exp[59, 15] == 0 and not exp[:12, 15].any() and exp[60:76, 15].any()
    got, rows = _build(gpu, w, 4)
    assert rows == 16 and th.first_difference(got, exp) is None

    w17 = ai.words(ops + [(ai.ADD, 1, 2, 0)])
    fill = np.full(COLUMNS * 16, ONES, dtype=np.uint64)
    trace, d_ops, scratch = pg.DeviceBuffer.from_host(gpu, fill), pg.DeviceBuffer.from_host(gpu, w17), _scratch(gpu, 10, 4)
    err, rows = _call(gpu, d_ops.ptr, 10, 4, trace.ptr, 16, scratch.ptr)
    assert err is not None and err.code == pg.GL_E_INVALID and "take 17 rows" in str(err) and rows == 17
    gpu.synchronize()
    assert (trace.download() == fill).all()
    # d_trace == NULL asks for the count alone: the stride is not read, the height does not matter
    err, rows = _call(gpu, d_ops.ptr, 10, 1, None, 0, scratch.ptr)
    assert err is None and rows == 17
    assert at.rows(gpu, w17) == 17 and at.rows(gpu, ai.words([])) == 0
    # no operations: an all-padding trace, no list
    got, rows = _build(gpu, ai.words([]), 3, pad=5)
    assert rows == 0 and not got.any()
    d = at.generate_trace(gpu, [])
    assert d.rows == 0 and d.n == COLUMNS * 2 and not d.download().any()


# ---------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_data_refusals_write_nothing_and_name_the_lowest_record(gpu):
    import plonky2_gpu_amd as pg

    num_ops = 300
    base = _ops("mixed", num_ops)
    n = 1 << _bits(ar.num_rows(base))
    fill = np.full(COLUMNS * n, ONES, dtype=np.uint64)
    trace = pg.DeviceBuffer.from_host(gpu, fill)
    scratch = _scratch(gpu, num_ops, _bits(n))

    def refused(w):
        d_ops = pg.DeviceBuffer.from_host(gpu, w)
        err, rows = _call(gpu, d_ops.ptr, len(w), _bits(n), trace.ptr, n, scratch.ptr)
        assert err is not None and err.code == pg.GL_E_INVALID and rows == 0
        gpu.synchronize()
        assert (trace.download() == fill).all()
        return str(err)

    order = [int(x) for x in base[:10, 0]]
    one_row, div, mulmod = order.index(ai.ADD), order.index(ai.DIV), order.index(ai.MULMOD)
    for bad in (10, 11, 12, 1 << 32, ONES):  # SHL, SHR and beyond; an operator word is not cut to 32 bits
        w = base.copy()
        w[[290, 37], 0] = bad
        why = refused(w)
        assert "operator of record 37 " in why and "290" not in why
    w = base.copy()
    w[270, 24], w[41, 9] = 1 << 32, ONES
    why = refused(w)
    assert "limb of record 41 " in why and "2^32 or more" in why and "270" not in why
    w = base.copy()
    w[260, 0], w[258, 1], w[299, 0] = 10, 1 << 32, ONES  # the limb comes first
    assert "limb of record 258 " in refused(w)
    w = base.copy()
    w[299, 0], w[299, 16] = 10, 1 << 40  # both in one record, the last: the operator is named
    assert "operator of record 299 " in refused(w)
    w = base.copy()
    w[200 + one_row, 17], w[100 + div, 16] = 1, 1  # in2 of an ADD, in1 of a DIV: the lower one
    why = refused(w)
    assert "record %d " % (100 + div) in why and "must be zero" in why and str(200 + one_row) not in why
    w = base.copy()
    w[50 + one_row, 24] = 7
    assert "record %d " % (50 + one_row) in refused(w)
    w = base.copy()
    w[50 + one_row, 24], w[50 + one_row, 3] = 7, 1 << 32  # a limb too wide and a must-be-zero input in one record: the limb
    assert "limb of record %d " % (50 + one_row) in refused(w)
    w = base.copy()
    w[20 + mulmod, 9:17] = 0  # a MULMOD may have any in1
    d_ops = pg.DeviceBuffer.from_host(gpu, w)
    err, rows = _call(gpu, d_ops.ptr, num_ops, _bits(n), trace.ptr, n, scratch.ptr)
    assert err is None and rows == ar.num_rows(w)
    assert th.first_difference(trace.download().reshape(COLUMNS, n), ar.trace_of_words(w, _bits(n))) is None


@pytest.mark.gpu
def test_argument_refusals_launch_nothing(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    num_ops, n = 10, 32
    w = _ops("mixed", num_ops)
    scratch_words = _lib.load().gl_arithmetic_table_scratch_bytes(num_ops, 5) // 8
    fill = np.full(COLUMNS * n + W * num_ops + scratch_words, ONES, dtype=np.uint64)
    fill[COLUMNS * n : COLUMNS * n + W * num_ops] = w.reshape(-1)
    buf = pg.DeviceBuffer.from_host(gpu, fill)  # a trace, behind it the operations, behind them the scratch
    d_ops, d_scratch = buf.at(COLUMNS * n), buf.at(COLUMNS * n + W * num_ops)
    assert d_scratch % 16 == 0 and scratch_words % 2 == 0

    def refused(*args, **kw):
        err, rows = _call(gpu, *args, **kw)
        assert err is not None and err.code == pg.GL_E_INVALID
        return str(err)

    assert "degree_bits" in refused(d_ops, num_ops, 0, buf.ptr, n, d_scratch)
    assert "degree_bits" in refused(d_ops, num_ops, 23, buf.ptr, 1 << 23, d_scratch)
    assert "num_ops" in refused(d_ops, (1 << 22) + 1, 5, buf.ptr, n, d_scratch)
    assert "trace_stride" in refused(d_ops, num_ops, 5, buf.ptr, n - 1, d_scratch)
    assert "null pointer" in refused(None, num_ops, 5, buf.ptr, n, d_scratch)
    assert "null pointer" in refused(d_ops, num_ops, 5, buf.ptr, n, None)
    assert "null pointer" in refused(None, 0, 5, buf.ptr, n, None)  # without operations the scratch is still asked for
    assert "null pointer" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch, ctx=False)
    with pytest.raises(pg.Plonky2HipError, match="null pointer"):
        _lib.call("gl_arithmetic_table_trace", d_ops, num_ops, 5, buf.ptr, n, d_scratch, None, gpu.ptr)  # h_rows
    assert "aligned" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch + 8)
    assert "d_trace overlaps d_ops" in refused(buf.at(COLUMNS * n - 1), num_ops, 5, buf.ptr, n, d_scratch)  # its first word is the trace's last
    assert "d_trace overlaps d_ops" in refused(buf.at(5), num_ops, 5, buf.ptr, n, d_scratch)
    assert "d_scratch overlaps d_ops" in refused(d_ops, num_ops, 5, buf.ptr, n, d_scratch - 16)
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, 5, buf.ptr, n, buf.at(COLUMNS * n - scratch_words))  # the trace's last words
    assert "d_trace overlaps d_scratch" in refused(d_ops, num_ops, 5, buf.ptr, n, buf.at(4))
    assert _lib.load().gl_arithmetic_table_scratch_bytes((1 << 22) + 1, 5) == 0
    assert _lib.load().gl_arithmetic_table_scratch_bytes(1, 0) == 0 and _lib.load().gl_arithmetic_table_scratch_bytes(1, 23) == 0
    gpu.synchronize()
    assert (buf.download(0, COLUMNS * n + W * num_ops) == fill[: COLUMNS * n + W * num_ops]).all()
    err, rows = _call(gpu, d_ops, num_ops, 5, buf.ptr, n, d_scratch)  # the same buffers, accepted
    assert err is None and rows == 15
    assert (buf.download(0, COLUMNS * n).reshape(COLUMNS, n) == _reference("mixed", num_ops, degree_bits=5)).all()
    assert (buf.download(COLUMNS * n, W * num_ops) == fill[COLUMNS * n : COLUMNS * n + W * num_ops]).all()
    err, rows = _call(gpu, None, 0, 5, buf.ptr, n, d_scratch)  # no operations, no list
    assert err is None and rows == 0 and not buf.download(0, COLUMNS * n).any()


# ---------------------------------------------------------------- proofs
FP5 = si.fri_params(rate_bits=2, cap_height=1, arity_bits=(2,))
FP3 = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,))


@functools.lru_cache(maxsize=None)
def _provable(n, with_div=True):
    """32: every operator (16 rows) and ten more operations, 31 rows and a padding row; 64: every operator and 32 more, 64 rows, a
    MULMOD's second row on the last. Without DIV: the same lists with MOD in DIV's place."""
    w = np.concatenate([ai.every_operator(), ai.mixed({32: 10, 64: 32}[n])])
    assert ar.num_rows(w) == {32: 31, 64: 64}[n] and {int(x) for x in w[:, 0]} == set(range(10))
    if not with_div:
        w[w[:, 0] == ai.DIV, 0] = ai.MOD
    w.setflags(write=False)
    cols = ar.trace_of_words(w, n.bit_length() - 1)
    cols.setflags(write=False)
    return w, cols


@functools.lru_cache(maxsize=None)
def _stark(constraint_degree=5):
    from plonky2_gpu_amd import arithmetic_table as at

    instrs, immediates = at.program()
    return ar.ArithmeticTableStark(instrs, immediates, constraint_degree)


@functools.lru_cache(maxsize=None)
def _reference_proof(hasher, num_challenges, n, constraint_degree=5):
    """tests/stark_ref.py's proof of the reference trace, computed once"""
    from oracle import accel

    fp = FP5 if constraint_degree == 5 else FP3
    trace = [[int(v) for v in col] for col in _provable(n, constraint_degree == 5)[1]]
    with accel.c_backend():
        return sr.proof_bytes(HASHERS[hasher], sr.prove(HASHERS[hasher], _stark(constraint_degree), num_challenges, fp, trace, []))


def _device_trace(ctx, n, with_div=True):
    from plonky2_gpu_amd import arithmetic_table as at

    return at.generate_trace(ctx, _provable(n, with_div)[0], degree_bits=n.bit_length() - 1)


def _desc(n, num_challenges, constraint_degree=5):
    from plonky2_gpu_amd import arithmetic_table as at

    if constraint_degree == 5:
        return at.stark_desc(n.bit_length() - 1, num_challenges, FP5)  # the default degree
    return at.stark_desc(n.bit_length() - 1, num_challenges, FP3, constraint_degree=3)


def _check_proof_bytes(gpu, hasher, num_challenges, n, constraint_degree=5, compiled=False, verify=None):
    """the device's proof of the device-built trace is the reference's, again on recycled buffers, and parses back to its bytes;
    `verify`: the evaluator with which tests/stark_ref.py's verifier must accept it as well"""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    exp = _reference_proof(hasher, num_challenges, n, constraint_degree)
    desc = _desc(n, num_challenges, constraint_degree)
    ns = pg.NativeStark(gpu, desc, hasher, compiled=compiled, unit_instrs=0 if compiled else None)
    try:
        assert bool(ns.is_compiled) == compiled
        if compiled:
            assert ns.num_units == len(pstark.split_program(desc, 0)) >= 1
        d_trace = _device_trace(gpu, n, constraint_degree == 5)
        data = ns.prove_bytes(d_trace, [])
        assert data == exp
        assert ns.prove_bytes(d_trace, []) == exp  # on recycled buffers
    finally:
        ns.close()
    parsed = pstark.proof_from_bytes(data, desc, hasher)
    assert pstark.proof_to_bytes(parsed, desc, hasher) == data
    if verify:
        fp = FP5 if constraint_degree == 5 else FP3
        with accel.c_backend():
            assert sr.verify(HASHERS[hasher], _stark(constraint_degree), num_challenges, fp, parsed, evaluator=verify)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("hasher,num_challenges,constraint_degree", [("poseidon", 2, 5), ("keccak", 2, 5), ("keccak", 1, 3), ("poseidon", 1, 3)])
def test_proof_bytes_of_the_device_built_trace_equal_the_reference(gpu, hasher, num_challenges, constraint_degree, n):
    """interpreted. Degree 5 on the traces with DIV rows; degree 3, the reference's, on the same lists with MOD in DIV's place."""
    verify = "closure" if (hasher, n) in (("poseidon", 32), ("keccak", 64)) else "program"
    _check_proof_bytes(gpu, hasher, num_challenges, n, constraint_degree, verify=verify)


@pytest.mark.gpu
def test_compiled_in_units_gives_the_same_bytes(gpu):
    """unit_instrs=0: the library's cap; num_units is what split_program cuts the program into — twelve kernels, whose cold
    compile is this test's ten seconds"""
    _check_proof_bytes(gpu, "poseidon", 2, 32, compiled=True, verify="program")


@pytest.mark.gpu
def test_the_verifier_accepts_the_proof_and_refuses_a_flipped_cell(gpu):
    """tests/stark_verify.py on the bytes: it accepts the proof of the device-built trace; with the low bit of a MULMOD's output
    limb flipped the device still returns a proof (quotient_degree_factor 4 is a power of two: nothing is trimmed), and the
    verifier refuses it at zeta"""
    import plonky2_gpu_amd as pg
    import stark_verify

    n = 32
    w, cols = _provable(n)
    ops = [int(x) for x in w[:, 0]]
    row = sum(2 if op in ar.MODULAR else 1 for op in ops[: ops.index(ai.MULMOD)])
    column = 60 + 3
    ns = pg.NativeStark(gpu, _desc(n, 2))
    try:
        d_trace = _device_trace(gpu, n)
        assert stark_verify.accepts(ns.desc, ns.prove_bytes(d_trace, []))
        cell = d_trace.download(column * n + row, 1)
        assert cell[0] == cols[column, row] and cols[ai.MULMOD, row] == 1
        d_trace.upload(cell ^ np.uint64(1), column * n + row)
        data = ns.prove_bytes(d_trace, [])
    finally:
        ns.close()
    with pytest.raises(AssertionError, match=th.REJECTED_AT_ZETA):
        stark_verify.accepts(ns.desc, data)


@pytest.mark.gpu
def test_quotient_polys_on_random_words_equal_the_reference(gpu):
    """uniformly random u64 words, non-canonical ones planted, in place of the LDE of a 32-row trace at quotient_degree_factor 4
    (every constraint non-zero), at the tight and at a padded column pitch"""
    import plonky2_gpu_amd as pg

    rng = np.random.default_rng(92)
    lde = rng.integers(0, 1 << 64, size=(COLUMNS, 128), dtype=np.uint64)
    lde[3, 0], lde[59, 1], lde[60, 2], lde[0, 3], lde[91, 127] = ONES, P, ONES, P + 1, ONES - 1
    alphas = [int(x) for x in rng.integers(0, 1 << 64, size=2, dtype=np.uint64)]
    leaves = [[int(v) % P for v in row] for row in lde.T]
    exp = np.array(sr.compute_quotient_polys(_stark(), 2, 5, 2, leaves, None, None, [], alphas), dtype=np.uint64)
    assert exp.shape == (2, 128) and exp.all()
    ns = pg.NativeStark(gpu, _desc(32, 2))
    try:
        for stride in (128, 128 + 6):
            buf = Strided(gpu, lde, stride)
            got = ns.quotient_polys(buf.ptr, None, stride, alphas, None, [])
            assert (buf.polys() == lde).all()
            buf.free()
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("column pitch", stride, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad))
    finally:
        ns.close()


# ---------------------------------------------------------------- the lookups: a plain looker through the three entries
B_FLAGS, B_VALUES, F_BINARY = 0, 5, 29          # five flags, in0, in1, result
M_FLAGS, M_VALUES, F_MODULAR = 30, 34, 66       # four flags, in0, in1, in2, result
D_VALUES, F_DIV, LOOKER_COLUMNS = 67, 91, 92    # in0, in2, quotient


class _Looker:
    """the stand-in for a table that looks into the arithmetic table: per row an operation as each of the three entries spells it
    — flags, the inputs and the result as eight 32-bit limbs each — under a filter of its own. Its own constraints: the three
    filters are boolean."""
    num_columns, num_public_inputs, constraint_degree, pairs = LOOKER_COLUMNS, 0, 3, []

    def __init__(self):
        from plonky2_gpu_amd.stark import StarkAsm

        a = StarkAsm()
        for c in (F_BINARY, F_MODULAR, F_DIV):
            a.release()
            f = a.local(c)
            a.emit(a.mul(f, a.sub(f, a.imm(1))))
        self.instrs, self.immediates = a.program()

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        for c in (F_BINARY, F_MODULAR, F_DIV):
            consumer.constraint(F.mul(local[c], F.sub(local[c], F.one)))


@functools.lru_cache(maxsize=None)
def _lookup_system():
    """(looker trace [92][16], arithmetic words, lookups): the operations of the 32-row provable list, each in the section of its
    entry, one per row from row 0; the other rows carry sevens under a filter of 0"""
    from plonky2_gpu_amd import arithmetic_table as at
    from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, TableWithColumns

    w = _provable(32)[0]
    limbs = lambda v: [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]  # noqa: E731
    rows = np.full((16, LOOKER_COLUMNS), 7, dtype=np.uint64)
    rows[:, F_BINARY] = rows[:, F_MODULAR] = rows[:, F_DIV] = 0
    at_row = {"binary": 0, "modular": 0, "div": 0}
    for op, in0, in1, in2 in ar.ops_from_words(w):
        res = limbs(at.result(op, in0, in1, in2))
        if op in ar.ONE_ROW:
            r = at_row["binary"]
            rows[r, B_FLAGS:F_BINARY] = [int(op == f) for f in (0, 1, 2, 8, 9)] + limbs(in0) + limbs(in1) + res
            rows[r, F_BINARY] = 1
            at_row["binary"] += 1
        elif op == ai.DIV:
            r = at_row["div"]
            rows[r, D_VALUES:F_DIV] = limbs(in0) + limbs(in2) + res
            rows[r, F_DIV] = 1
            at_row["div"] += 1
        else:
            r = at_row["modular"]
            rows[r, M_FLAGS:F_MODULAR] = [int(op == f) for f in (4, 5, 6, 7)] + limbs(in0) + limbs(in1) + limbs(in2) + res
            rows[r, F_MODULAR] = 1
            at_row["modular"] += 1
    assert all(0 < v <= 16 for v in at_row.values()), at_row
    single = lambda a, b: [CtlColumn.single(c) for c in range(a, b)]  # noqa: E731
    lookups = [CrossTableLookup([TableWithColumns(0, single(B_FLAGS, F_BINARY), CtlColumn.single(F_BINARY))],
                                TableWithColumns(1, at.ctl_data("binary"), at.ctl_filter("binary"))),
               CrossTableLookup([TableWithColumns(0, single(M_FLAGS, F_MODULAR), CtlColumn.single(F_MODULAR))],
                                TableWithColumns(1, at.ctl_data("modular"), at.ctl_filter("modular"))),
               CrossTableLookup([TableWithColumns(0, single(D_VALUES, F_DIV), CtlColumn.single(F_DIV))],
                                TableWithColumns(1, at.ctl_data("div"), at.ctl_filter("div")))]
    return [[int(v) for v in col] for col in rows.T], w, lookups


@pytest.mark.gpu
@pytest.mark.parametrize("compiled", [False, True])
def test_a_looker_through_the_three_entries_equals_the_reference(gpu, compiled):
    """The arithmetic table, 32 rows built on the device, is looked through "binary", "modular" and "div": second rows and the
    padding row have every filter 0. Three lookups, one looking TWC each, all of one 16-row table of plain single columns."""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import arithmetic_table as at
    from plonky2_gpu_amd import stark as pstark
    from plonky2_gpu_amd.stark import StarkDesc, StarkTablesDesc

    hasher, num_challenges = "poseidon", 2
    looker_trace, w, lookups = _lookup_system()
    cols = _provable(32)[1]
    looker = _Looker()
    fps = [si.fri_params(rate_bits=2, cap_height=1, arity_bits=(2,), num_query_rounds=4, proof_of_work_bits=2) for _ in range(2)]
    system = th.System([looker, _stark()], lookups)
    with accel.c_backend():
        exp = cr.proofs_bytes(HASHERS[hasher], cr.prove_tables(HASHERS[hasher], system, num_challenges, fps,
                                                               [looker_trace, [[int(v) for v in col] for col in cols]]))
    desc = StarkTablesDesc([StarkDesc(4, LOOKER_COLUMNS, 0, 3, num_challenges, fps[0], looker.instrs, looker.immediates),
                            at.stark_desc(5, num_challenges, fps[1])], lookups)
    desc.validate(hasher)
    nt = pg.NativeStarkTables(gpu, desc, hasher, compiled=compiled, unit_instrs=0 if compiled else None)
    try:
        if compiled:
            assert nt.is_compiled and nt.num_units[1] >= len(pstark.split_program(desc.tables[1], 0))
        data = nt.prove_bytes([looker_trace, at.generate_trace(gpu, w, degree_bits=5)])
    finally:
        nt.close()
    assert data == exp
    with accel.c_backend():
        assert cr.verify_tables(HASHERS[hasher], system, num_challenges, fps, pstark.tables_proof_from_bytes(data, desc, hasher))
