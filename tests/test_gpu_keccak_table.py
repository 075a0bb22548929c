"""The Keccak-f table on the device: gl_keccak_table_trace against tests/keccak_table_ref.py's generate_trace_rows on all 2430
columns, and the table proved by gl_stark_prove / gl_stark_tables_prove from the device-built trace against tests/stark_ref.py and
tests/ctl_ref.py, byte for byte: there is no tolerance anywhere. The reference provers run with oracle.accel.c_backend (hashes,
trees and transforms in C); the algebra of the STARK stays Python."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref as cr  # noqa: E402
import keccak_ref  # noqa: E402
import keccak_table_ref as kr  # noqa: E402
import stark_instances as si  # noqa: E402
import table_harness as th  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = 0xFFFFFFFF00000001
ONES = (1 << 64) - 1
HASHERS = th.HASHERS
COLUMNS = 2430


# ---------------------------------------------------------------- inputs and reference traces
@functools.lru_cache(maxsize=None)
def _pool():
    """341 states: a random one, all ones, all zero, every word with low limb / with high limb 0xFFFFFFFF, a single bit at z = 0, 31, 32,
    63 of lane (0, 0) (word 0) and of lane (4, 4) (word 24), then random states; the first 42 are what they were when there were 42"""
    rng = np.random.default_rng(2430)
    rand = rng.integers(0, 1 << 64, size=(42, 25), dtype=np.uint64)
    states = [rand[0], np.full(25, ONES, dtype=np.uint64), np.zeros(25, dtype=np.uint64), rand[1] | np.uint64(0xFFFFFFFF),
              rand[2] | np.uint64(0xFFFFFFFF00000000)]
    for word in (0, 24):
        for z in (0, 31, 32, 63):
            s = np.zeros(25, dtype=np.uint64)
            s[word] = np.uint64(1 << z)
            states.append(s)
    states += [rand[k] for k in range(3, 3 + 42 - len(states))]
    out = np.array(states, dtype=np.uint64)
    assert out.shape == (42, 25)
    out = np.concatenate([out, np.random.default_rng(341).integers(0, 1 << 64, size=(341 - 42, 25), dtype=np.uint64)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference_trace(count, n):
    """[2430][n] columns; never changed"""
    cols = np.ascontiguousarray(kr.generate_trace_rows(_pool()[:count], n).T)
    cols.setflags(write=False)
    return cols


def _trace_call(gpu, d_inputs, count, degree_bits, d_trace, stride):
    from plonky2_gpu_amd import _lib

    _lib.call("gl_keccak_table_trace", d_inputs, count, degree_bits, d_trace, stride, gpu.ptr)


# inputs, rows, pitch beyond n
SHAPES = [(0, 32, 0), (1, 32, 0), (1, 64, 24), (2, 64, 0), (3, 128, 0), (11, 512, 24), (42, 1024, 0), (341, 8192, 0), (170, 4096, 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("count,n,pad", SHAPES)
def test_trace_equals_generate_trace_rows(gpu, count, n, pad):
    """0 inputs: all padding; 1 / 32: one permutation and a padding permutation cut after 8 rounds; 1 / 64: a whole padding permutation
    and a cut one; 2 / 64: a permutation ending 16 rows before the end; 3 / 128: a permutation across the wave boundary at row 64;
    11 / 512: one across the 256-thread block boundary; 42 / 1024: 1008 rows of inputs, 16 of padding; 341 / 8192: 32 blocks, 8184 rows
    of inputs and a padding permutation cut after 8 rounds; 170 / 4096: a padded pitch over 16 blocks. The buffer is pre-filled with
    0xFF bytes — an unwritten word shows —, guards and the gap of a padded pitch hold sentinels that must survive."""
    import plonky2_gpu_amd as pg

    exp = _reference_trace(count, n)
    buf = Strided(gpu, np.full((COLUMNS, n), ONES, dtype=np.uint64), n + pad)
    d_in = pg.DeviceBuffer.from_host(gpu, _pool()[:count]) if count else None
    _trace_call(gpu, d_in.ptr if d_in else None, count, n.bit_length() - 1, buf.ptr, n + pad)
    got = buf.polys(("trace", count, n, pad))
    buf.free()
    bad = np.argwhere(got != exp)
    assert bad.size == 0, ("first (column, row) that differs", bad[0].tolist(), len(bad), hex(int(got[tuple(bad[0])])), hex(int(exp[tuple(bad[0])])))
    outputs = keccak_ref.keccak_f1600(_pool()[:count]) if count else []  # all permutations at once
    for k in range(count):
        assert kr.outputs_of(got.T, k) == [int(v) for v in outputs[k]]


@pytest.mark.gpu
def test_generate_trace_of_the_module(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import keccak_table as kt

    for stride in (None, 64 + 24):
        d = kt.generate_trace(gpu, _pool()[:2], 6, trace_stride=stride)
        got = d.download().reshape(COLUMNS, stride or 64)[:, :64]
        assert (got == _reference_trace(2, 64)).all()
    d_in = pg.DeviceBuffer.from_host(gpu, _pool()[:2])
    assert (kt.generate_trace(gpu, d_in, 6).download().reshape(COLUMNS, 64) == _reference_trace(2, 64)).all()


@pytest.mark.gpu
def test_trace_refusals_write_nothing(gpu):
    import plonky2_gpu_amd as pg

    n = 32
    fill = np.full(COLUMNS * n + 25, ONES, dtype=np.uint64)
    fill[-25:] = _pool()[0]
    buf = pg.DeviceBuffer.from_host(gpu, fill)  # a trace and, behind it, one input
    d_in = buf.at(COLUMNS * n)

    def refused(*args):
        with pytest.raises(pg.Plonky2HipError) as e:
            _trace_call(gpu, *args)
        assert e.value.code == pg.GL_E_INVALID
        return str(e.value)

    assert "degree_bits" in refused(d_in, 0, 0, buf.ptr, n)
    assert "degree_bits" in refused(d_in, 1, 25, buf.ptr, 1 << 25)
    assert "24 * num_inputs" in refused(d_in, 2, 5, buf.ptr, n)
    assert "trace_stride" in refused(d_in, 1, 5, buf.ptr, n - 1)
    assert "null pointer" in refused(d_in, 1, 5, None, n)
    assert "null pointer" in refused(None, 1, 5, buf.ptr, n)
    assert "overlaps" in refused(buf.at(COLUMNS * n - 1), 1, 5, buf.ptr, n)  # the input's first word is the trace's last
    assert "overlaps" in refused(buf.at(5), 1, 5, buf.ptr, n)
    gpu.synchronize()
    assert (buf.download() == fill).all()
    _trace_call(gpu, None, 0, 5, buf.ptr, n)  # no inputs and no input pointer: allowed
    assert (buf.download(0, COLUMNS * n).reshape(COLUMNS, n) == _reference_trace(0, n)).all()


# ---------------------------------------------------------------- proofs of the 32-row trace
TABLE = th.Table("keccak_table", kr.KeccakTableStark, COLUMNS, (32,), reference_trace=lambda n: _reference_trace(1, n),
                 device_trace=lambda ctx, n: TABLE.module.generate_trace(ctx, _pool()[:1], n.bit_length() - 1),
                 flip=lambda kt: (kt.reg_a_prime(2, 3, 40), 7))
_stark = TABLE.stark


@pytest.mark.gpu
@pytest.mark.parametrize("hasher,num_challenges", [("poseidon", 1), ("poseidon", 2), ("keccak", 1), ("keccak", 3)])
def test_proof_bytes_of_the_device_built_trace_equal_the_reference(gpu, hasher, num_challenges):
    """2430 columns and a program of 47 000 instructions through every stage of gl_stark_prove. Keccak with 2 challenges would have
    quotient leaves of 4 elements, which KeccakHash<25> cannot hash (the reference panics): 1 and 3 there."""
    th.check_proof_bytes(TABLE, gpu, hasher, num_challenges, 32)


@pytest.mark.gpu
def test_quotient_polys_on_random_words_equal_the_reference(gpu):
    """the 47 000-instruction program through the interpreter at 2430 columns, 2^5 rows, on uniformly random words in place of the
    LDEs (every constraint non-zero), at the tight and at a padded column pitch"""
    rng = np.random.default_rng(55)
    lde = rng.integers(0, P, size=(COLUMNS, 64), dtype=np.uint64)
    alphas = [int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)]
    th.check_quotient_polys(TABLE, gpu, lde, alphas)


@pytest.mark.gpu
def test_a_flipped_a_prime_bit_gives_a_proof_the_verifier_rejects(gpu):
    """quotient_degree_factor 2 is a power of two: the reference's trim cannot fail, its prover returns a proof of the violated trace,
    and verification fails at zeta. The device does the same."""
    column, row = TABLE.flip(TABLE.module)
    assert _reference_trace(1, 32)[column, row] in (0, 1)
    th.check_flipped_cell_is_rejected(TABLE, gpu, "stark_ref")


# ---------------------------------------------------------------- two tables and the cross-table lookup
class _Sponge:
    """the 101-column stand-in for the table that uses the permutations: 50 input limbs, 50 output limbs, a 0 / 1 filter f with
    f (f - 1) = 0"""
    num_columns, num_public_inputs, constraint_degree, pairs = 101, 0, 3, []

    def __init__(self):
        from plonky2_gpu_amd.stark import StarkAsm

        a = StarkAsm()
        f = a.local(100)
        a.emit(a.mul(f, a.sub(f, a.imm(1))))
        self.instrs, self.immediates = a.program()

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        consumer.constraint(F.mul(local[100], F.sub(local[100], F.one)))


@pytest.mark.gpu
def test_two_tables_with_the_keccak_lookup_equal_the_reference(gpu):
    """2 inputs in 64 Keccak rows (the padding permutation behind them is cut after 16 rounds: it completes nothing, so the looking
    table has no row for it), 4 rows of the looking table: two with filter 1, two with filter 0. One lookup over 100 columns with
    filters on both sides. A filtered row holds what the Keccak table shows where ITS filter is 1, the row of round 23:
    reg_input_limb is reg_a of that row (keccak_stark.rs:34-43 with columns.rs:15-26), so the 50 "input" limbs of the lookup are the
    state entering round 23, not the permutation's input, and the 50 output limbs are Keccak-f of the input. That is the lookup as
    the reference has it; with the permutation's own input in those columns the products differ and no verifier accepts."""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd import stark as pstark
    from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, StarkDesc, StarkTablesDesc, TableWithColumns

    inputs = _pool()[:2]
    outputs = keccak_ref.keccak_f1600(inputs)
    limbs = lambda words: [int(w) >> (32 * h) & 0xFFFFFFFF for w in words for h in range(2)]  # noqa: E731
    last_rows = [_reference_trace(2, 64)[:, 24 * k + 23] for k in range(2)]
    round_23_inputs = [[int(row[kr.reg_input_limb(i)]) for i in range(50)] for row in last_rows]
    assert round_23_inputs[0] != limbs(inputs[0])
    sponge_rows = [round_23_inputs[k] + limbs(outputs[k]) + [1] for k in range(2)] + [[0] * 101, [7] * 100 + [0]]
    sponge_trace = [[r[c] for r in sponge_rows] for c in range(101)]
    sponge = _Sponge()
    lookups = [CrossTableLookup([TableWithColumns(0, [CtlColumn.single(c) for c in range(100)], CtlColumn.single(100))],
                                TableWithColumns(1, kt.ctl_data(), kt.ctl_filter()))]
    fps = [si.fri_params(rate_bits=1, cap_height=1, arity_bits=ab, num_query_rounds=4, proof_of_work_bits=2) for ab in ((), (2,))]
    system = th.System([sponge, _stark()], lookups)
    keccak_trace = [[int(v) for v in col] for col in _reference_trace(2, 64)]
    with accel.c_backend():
        exp = cr.proofs_bytes(HASHERS["poseidon"], cr.prove_tables(HASHERS["poseidon"], system, 1, fps, [sponge_trace, keccak_trace]))
    desc = StarkTablesDesc([StarkDesc(2, 101, 0, 3, 1, fps[0], sponge.instrs, sponge.immediates), kt.stark_desc(6, 1, fps[1])], lookups)
    desc.validate()
    nt = pg.NativeStarkTables(gpu, desc)
    try:
        data = nt.prove_bytes([sponge_trace, kt.generate_trace(gpu, inputs, 6)])
    finally:
        nt.close()
    assert data == exp
    with accel.c_backend():
        assert cr.verify_tables(HASHERS["poseidon"], system, 1, fps, pstark.tables_proof_from_bytes(data, desc))


# ---------------------------------------------------------------- two contexts, two threads
@pytest.mark.gpu
def test_two_contexts_on_two_threads_build_and_prove(gpu):
    th.check_two_contexts_on_two_threads(TABLE, gpu)
