"""STARK proofs on the device (gl_stark_create / gl_stark_prove and the two kernels alone) against tests/stark_ref.py, bit for bit:
there is no tolerance anywhere. The STARKs A (Fibonacci, qdf 1), B (degree 3, every opcode, three permutation pairs, qdf 2) and C
(degree 4, qdf 3, no pairs) and the family D(d) (degree d up to 17: qdf up to the library's 16, with up to 4 challenges; a variant without
public inputs, a variant with five columns for Keccak) are tests/stark_instances.py's. The reference runs with oracle.accel.c_backend (its Poseidon, trees and
transforms in C): the algebra of the STARK stays Python."""
import ctypes
import functools
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generic_prove_ref as gr  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = 0xFFFFFFFF00000001
HASHERS = {"poseidon": gr.PoseidonHasher(), "keccak": gr.KeccakHasher()}


def _challenge_sets(seed, qdf, num_challenges):
    rng = np.random.default_rng(seed)
    return [[(int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64))) for _ in range(num_challenges)] for _ in range(qdf)]


def _native(gpu, stark, degree_bits, num_challenges, fri_params, hasher="poseidon"):
    import plonky2_gpu_amd as pg

    return pg.NativeStark(gpu, stark.desc(degree_bits, num_challenges, fri_params), hasher)


# ---------------------------------------------------------------- the permutation Zs
@functools.lru_cache(maxsize=None)
def _trace(name, degree_bits):
    return si.STARKS[name].make_trace(degree_bits, seed=degree_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("num_challenges", [1, 2, 3])
@pytest.mark.parametrize("degree_bits", [3, 8])
@pytest.mark.parametrize("name", ["A", "B"])
def test_permutation_zs_equal_the_reference(gpu, name, degree_bits, num_challenges):
    """B: 3 pairs x num_challenges instances in batches of 2 — a short last batch for 1 and 3 challenges; 2^8 rows: more than one
    scan element per thread; the trace at a padded pitch as well as the tight one"""
    stark = si.STARKS[name]
    trace, _ = _trace(name, degree_bits)
    sets = _challenge_sets(100 * degree_bits + num_challenges, sr.quotient_degree_factor(stark), num_challenges)
    exp = np.array(sr.compute_permutation_z_polys(stark, num_challenges, trace, sets), dtype=np.uint64)
    assert exp.shape[0] == sr.num_zs(stark, num_challenges) and (exp[:, 0] == 1).all()
    ns = _native(gpu, stark, degree_bits, num_challenges, si.fri_params(rate_bits=2))
    try:
        n = 1 << degree_bits
        for stride in (n, n + 6):
            assert (ns.permutation_zs(trace, sets, trace_stride=stride) == exp).all(), ("trace pitch", stride)
    finally:
        ns.close()


@pytest.mark.gpu
def test_permutation_zs_at_two_scan_blocks(gpu):
    """2^11 rows are two blocks of the prefix product (1024 rows each): the block totals are scanned and multiplied in"""
    from oracle import accel

    stark, degree_bits = si.A, 11
    trace, _ = _trace("A", degree_bits)
    sets = _challenge_sets(7, 1, 2)
    with accel.c_backend():
        exp = np.array(sr.compute_permutation_z_polys(stark, 2, trace, sets), dtype=np.uint64)
    ns = _native(gpu, stark, degree_bits, 2, si.fri_params(rate_bits=1))
    try:
        assert (ns.permutation_zs(trace, sets) == exp).all()
    finally:
        ns.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,degree_bits,num_challenges", [("A", 10, 2), ("B", 13, 3), ("D17", 3, 4)])
def test_permutation_zs_at_one_and_at_eight_scan_blocks_and_at_the_limits(gpu, name, degree_bits, num_challenges):
    """2^10 rows: exactly one block of the prefix product; 2^13 rows of B with 3 challenges: 5 Zs over 8 blocks each (the block
    totals of Z b start at b * 8), at the tight and at a padded trace pitch; D(17) with 4 challenges: 8 instances in one short batch
    of 16, the challenge sets 0 .. 7 of 16"""
    stark = si.STARKS[name]
    trace, _ = _trace(name, degree_bits)
    sets = _challenge_sets(300 + degree_bits, sr.quotient_degree_factor(stark), num_challenges)
    exp = np.array(sr.compute_permutation_z_polys(stark, num_challenges, trace, sets), dtype=np.uint64)
    assert exp.shape == (sr.num_zs(stark, num_challenges), 1 << degree_bits) and (exp[:, 0] == 1).all() and exp.all()
    ns = _native(gpu, stark, degree_bits, num_challenges, si.fri_params(rate_bits=4))
    try:
        n = 1 << degree_bits
        for stride in (n, n + 6):
            got = ns.permutation_zs(trace, sets, trace_stride=stride)
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("trace pitch", stride, "first (Z, row) that differs", bad[0].tolist(), len(bad))
    finally:
        ns.close()


@pytest.mark.gpu
def test_permutation_zs_at_more_block_totals_than_one_workgroup_has_threads(gpu):
    """2^19 rows are 512 blocks of the prefix product: every thread of the workgroup that scans the block totals takes two. The
    expected values come from stark_fuzz.fast_permutation_z_polys (one batch inversion instead of one inversion per row), which
    tests/test_stark_fuzz.py holds against sr.compute_permutation_z_polys"""
    import stark_fuzz as sf

    stark, degree_bits = si.A, 19
    trace, _ = _trace("A", degree_bits)
    sets = _challenge_sets(19, 1, 1)
    exp = np.array(sf.fast_permutation_z_polys(stark, 1, trace, sets), dtype=np.uint64)
    assert exp.shape == (1, 1 << degree_bits) and exp.all()
    ns = _native(gpu, stark, degree_bits, 1, si.fri_params(rate_bits=1))
    try:
        got = ns.permutation_zs(trace, sets)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, ("first (Z, row) that differs", bad[0].tolist(), len(bad))
    finally:
        ns.close()


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits,row", [(3, 2), (11, 1500)])
def test_a_zero_denominator_gives_quotient_zero(gpu, degree_bits, row):
    """the rule of include/plonky2_hip.h (gl_stark_permutation_zs): where the product of the right-hand sides vanishes the row's
    quotient is 0, as the reference's pow(0, p - 2) is, and every later Z value is 0. A has one pair of single columns (2, 3): the
    right-hand cell of `row` becomes p - gamma"""
    trace, _ = _trace("A", degree_bits)
    trace = [list(col) for col in trace]
    sets = _challenge_sets(55 + degree_bits, 1, 1)
    trace[3][row] = (P - sets[0][0][1]) % P
    exp = np.array(sr.compute_permutation_z_polys(si.A, 1, trace, sets), dtype=np.uint64)
    assert exp[0, : row + 1].all() and not exp[0, row + 1 :].any()
    ns = _native(gpu, si.A, degree_bits, 1, si.fri_params(rate_bits=1))
    try:
        got = ns.permutation_zs(trace, sets)
        assert not got[0, row + 1 :].any()
        assert (got == exp).all()
    finally:
        ns.close()


# ---------------------------------------------------------------- the quotient
@functools.lru_cache(maxsize=None)
def _quotient_case(name, degree_bits, rate_bits):
    """(trace LDE columns, Zs LDE columns or None, challenge sets, alphas, public inputs, the reference's coefficients); B with 3
    challenges: 9 permutation instances in 5 batches, the last one short"""
    from oracle import accel

    stark = si.STARKS[name]
    num_challenges = {"B": 3, "D6": 3, "D17": 4}.get(name, 2)
    trace, pis = _trace(name, degree_bits)
    rng = np.random.default_rng(1000 * degree_bits + rate_bits)
    alphas = [int(x) for x in rng.integers(0, P, size=num_challenges, dtype=np.uint64)]
    with accel.c_backend():
        trace_leaves = sr.lde_leaves(trace, rate_bits)
        sets = zs_leaves = None
        if stark.pairs:
            sets = _challenge_sets(degree_bits + rate_bits, sr.quotient_degree_factor(stark), num_challenges)
            zs_leaves = sr.lde_leaves(sr.compute_permutation_z_polys(stark, num_challenges, trace, sets), rate_bits)
        exp = sr.compute_quotient_polys(stark, num_challenges, degree_bits, rate_bits, trace_leaves, zs_leaves, sets, pis, alphas)
    cols = lambda leaves: None if leaves is None else np.array(leaves, dtype=np.uint64).T.copy()  # noqa: E731
    return cols(trace_leaves), cols(zs_leaves), sets, alphas, pis, np.array(exp, dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits", [3, 9])
@pytest.mark.parametrize("name,rate_bits", [("A", 1), ("A", 3), ("B", 1), ("B", 2), ("C", 2), ("C", 3)])
def test_quotient_polys_equal_the_reference(gpu, name, rate_bits, degree_bits):
    """step > 1 (rate_bits above qdb) and step = 1, the wrap of the next row at the end of the domain, the LDEs at the tight and at a
    padded column pitch (guards and pads checked: the kernel only reads them)"""
    _check_quotient(gpu, name, rate_bits, degree_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name,degree_bits,rate_bits", [("D5n", 3, 2), ("D5n", 3, 3), ("D6", 3, 3), ("D17", 3, 4), ("D17", 1, 5), ("A", 1, 1), ("A", 2, 2)])
def test_quotient_polys_at_the_limits_equal_the_reference(gpu, name, degree_bits, rate_bits):
    """D5n: no public inputs at all (an empty public-inputs buffer); D6: qdf 5 in a domain of 8 n points with 3 challenges; D17: qdf 16
    with 4 challenges, all 16 values of Z_H on the coset, 8 instances in one short batch, also on two rows; A on two and four rows"""
    _check_quotient(gpu, name, rate_bits, degree_bits)


def _check_quotient(gpu, name, rate_bits, degree_bits):
    stark = si.STARKS[name]
    trace_lde, zs_lde, sets, alphas, pis, exp = _quotient_case(name, degree_bits, rate_bits)
    qdf = sr.quotient_degree_factor(stark)
    n_ext = 1 << (degree_bits + rate_bits)
    num_challenges = len(alphas)
    assert exp.shape == (num_challenges, (1 << degree_bits) << (qdf - 1).bit_length())
    assert not exp[:, (qdf << degree_bits):].any() and exp[:, : qdf << degree_bits].any()  # a valid trace: no tail
    ns = _native(gpu, stark, degree_bits, num_challenges, si.fri_params(rate_bits=rate_bits))
    try:
        for stride in (n_ext, n_ext + 2, n_ext + 48):
            t = Strided(gpu, trace_lde, stride)
            z = Strided(gpu, zs_lde, stride) if zs_lde is not None else None
            got = ns.quotient_polys(t.ptr, z.ptr if z else None, stride, alphas, sets, pis)
            assert (t.polys() == trace_lde).all() and (z is None or (z.polys() == zs_lde).all())
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("column pitch", stride, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad))
            t.free()
            if z:
                z.free()
    finally:
        ns.close()


# ---------------------------------------------------------------- whole proofs
@functools.lru_cache(maxsize=None)
def _reference_proof(name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher):
    from oracle import accel

    stark = si.STARKS[name]
    fp = si.fri_params(rate_bits=rate_bits, cap_height=cap_height, arity_bits=arity_bits)
    trace, pis = _trace(name, degree_bits)
    with accel.c_backend():
        return sr.proof_bytes(HASHERS[hasher], sr.prove(HASHERS[hasher], stark, num_challenges, fp, trace, pis))


# name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher
PROOFS = [
    ("A", 3, 2, 1, 0, (1, 2), "poseidon"),
    ("A", 9, 2, 3, 2, (3,), "poseidon"),
    ("A", 3, 1, 3, 2, (), "poseidon"),
    ("B", 3, 1, 1, 0, (1, 2), "poseidon"),
    ("B", 9, 3, 2, 2, (3,), "poseidon"),
    ("B", 3, 3, 2, 0, (3,), "keccak"),
    ("B", 9, 1, 1, 2, (2, 2), "keccak"),
    ("C", 3, 2, 2, 0, (1, 2), "poseidon"),
    ("C", 9, 2, 3, 2, (3,), "poseidon"),
    ("C", 3, 1, 2, 2, (), "keccak"),
    ("C", 9, 2, 2, 0, (3,), "keccak"),
    ("B", 10, 2, 1, 2, (1, 2), "poseidon"),
    ("D5", 3, 2, 2, 0, (1, 2), "poseidon"),  # qdf 4: one full batch of 4 instances
    ("D6", 3, 3, 3, 1, (3,), "poseidon"),  # qdf 5, qdb 3: the chunk copy of 5 out of 8, batches of 5 + 1, the tail check
    ("D9", 4, 1, 3, 2, (2,), "poseidon"),  # qdf 8
    ("D17", 3, 4, 4, 0, (1, 2), "poseidon"),  # the limits: qdf 16, 4 challenges, 64 quotient polynomials, 8 instances in one short batch
    ("A", 1, 2, 1, 0, (), "poseidon"),  # the smallest traces
    ("A", 2, 1, 2, 1, (1,), "poseidon"),
    ("D17", 1, 4, 4, 0, (1,), "poseidon"),  # the smallest trace at the largest qdf
    ("D5n", 3, 2, 2, 0, (1, 2), "poseidon"),  # no public inputs
    ("D5k", 3, 2, 2, 0, (3,), "keccak"),  # five columns: Keccak cannot hash a leaf of four
    ("D17k", 1, 3, 4, 1, (), "keccak"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,degree_bits,num_challenges,rate_bits,cap_height,arity_bits,hasher", PROOFS)
def test_proof_bytes_equal_the_reference_and_verify(gpu, name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher):
    """5 query rounds, 3 proof-of-work bits; the second proof of the handle runs on recycled buffers"""
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    stark = si.STARKS[name]
    fp = si.fri_params(rate_bits=rate_bits, cap_height=cap_height, arity_bits=arity_bits)
    trace, pis = _trace(name, degree_bits)
    exp = _reference_proof(name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher)
    ns = _native(gpu, stark, degree_bits, num_challenges, fp, hasher)
    try:
        timing = {}
        data = ns.prove_bytes(trace, pis, timing=timing)
        assert data == exp
        assert ns.prove_bytes(trace, pis) == exp
        ns.trim()
        assert ns.prove_bytes(trace, pis) == exp
        assert len(timing) == 11 and all(v >= 0 for v in timing.values())
    finally:
        ns.close()
    parsed = pstark.proof_from_bytes(data, ns.desc, hasher)
    assert pstark.proof_to_bytes(parsed, ns.desc, hasher) == data
    assert (parsed["permutation_zs_cap"] is None) == (not stark.pairs)
    with accel.c_backend():
        assert sr.verify(HASHERS[hasher], stark, num_challenges, fp, parsed)


# ---------------------------------------------------------------- refusals
def _refused(gpu, stark, degree_bits, num_challenges, fp, hasher="poseidon", **changes):
    """gl_stark_create through NativeStark's own marshalling with fields of the description changed; returns the error"""
    import plonky2_gpu_amd as pg

    desc = stark.desc(degree_bits, num_challenges, fp)
    for k, v in changes.items():
        setattr(desc, k, v)
    with pytest.raises(pg.Plonky2HipError) as e:
        pg.NativeStark(gpu, desc, hasher).close()
    assert e.value.code == pg.GL_E_INVALID and len(str(e.value)) > 30
    return str(e.value)


@pytest.mark.gpu
def test_create_refuses_what_it_cannot_prove(gpu):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    assert "rate" in _refused(gpu, si.C, 4, 2, si.fri_params(rate_bits=1))  # qdb = 2 > rate_bits
    assert "hiding" in _refused(gpu, si.A, 4, 2, dict(si.fri_params(), hiding=True))
    assert "4 elements" in _refused(gpu, si.A, 4, 2, si.fri_params(arity_bits=(2,)), hasher="keccak")  # 4 trace columns
    assert "4 elements" in _refused(gpu, si.B, 4, 2, si.fri_params(arity_bits=(2,)), hasher="keccak")  # 2 challenges x qdf 2
    assert "arity_bits = 1" in _refused(gpu, si.C, 4, 2, si.fri_params(rate_bits=2, arity_bits=(1, 2)), hasher="keccak")
    instrs = si.A.instrs.copy()
    instrs[0, 0] = 1
    assert "LOAD_CONST" in _refused(gpu, si.A, 4, 2, si.fri_params(), instrs=instrs)
    instrs[0, 0] = 15
    assert "unknown opcode" in _refused(gpu, si.A, 4, 2, si.fri_params(), instrs=instrs)
    instrs = si.A.instrs.copy()
    instrs[0, 2] = 4
    assert "column out of range" in _refused(gpu, si.A, 4, 2, si.fri_params(), instrs=instrs)
    assert "public input out of range" in _refused(gpu, si.A, 4, 2, si.fri_params(), num_public_inputs=2)
    only_loads = si.A.instrs[:2].copy()
    assert "no EMIT" in _refused(gpu, si.A, 4, 2, si.fri_params(), instrs=only_loads)
    # the ACC contract: a term of weight 2^32 - 1 can reach (2^32 - 1)^2 > 2^63
    acc_prog = np.array([[0, 0, 0, 0], [9, 0, 0, 0], [9, 0, 0, 0], [9, 0, 0, 0], [10, 1, 0, 0], [7, 0, 1, 0]], dtype=np.uint16)
    assert "2^63" in _refused(gpu, si.A, 4, 2, si.fri_params(), instrs=acc_prog, immediates=[0xFFFFFFFF])
    assert "below 2^32" in _refused(gpu, si.A, 4, 2, si.fri_params(), instrs=acc_prog[[0, 1, 4, 5]], immediates=[1 << 32])
    assert "column out of range" in _refused(gpu, si.A, 4, 2, si.fri_params(), pairs=[[(2, 4)]])
    # a stale struct_size
    desc = _lib.GlStarkDesc()
    desc.struct_size = ctypes.sizeof(_lib.GlStarkDesc) - 8
    keep = np.zeros(8, dtype=np.uint64)
    desc.h_instrs = keep.ctypes.data
    h = ctypes.c_void_p()
    with pytest.raises(pg.Plonky2HipError) as e:
        _lib.call("gl_stark_create", 0, ctypes.byref(desc), ctypes.byref(h), gpu.ptr)
    assert e.value.code == pg.GL_E_INVALID and "struct_size" in str(e.value) and not h.value
    with pytest.raises(pg.Plonky2HipError) as e:
        _lib.call("gl_stark_create", 7, ctypes.byref(desc), ctypes.byref(h), gpu.ptr)
    assert e.value.code == pg.GL_E_INVALID and not h.value


@pytest.mark.gpu
def test_stark_opcodes_stay_out_of_gate_programs(gpu):
    """opcode 11 (LOAD_NEXT) in a gate program is refused by gl_gate_kernel_build exactly as an opcode nobody knows (here 99)"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    def build(op):
        instrs = np.array([[0, 0, 0, 0], [op, 1, 0, 0], [7, 0, 0, 0]], dtype=np.uint16)
        descs = np.array([[0, 0, 0, 1, 0, 3]], dtype=np.uint32)
        k = ctypes.c_void_p()
        with pytest.raises(pg.Plonky2HipError) as e:
            _lib.call("gl_gate_kernel_build", instrs, 3, descs, 1, None, 0, 1, 1, 2, ctypes.byref(k))
        assert not k.value
        return e.value.code, str(e.value)

    assert build(11) == build(99) and build(11)[0] == pg.GL_E_INVALID and "unknown opcode" in build(11)[1]
    assert build(14) == build(99)


# ---------------------------------------------------------------- a trace that violates the constraints
def _corrupted(name, degree_bits):
    trace, pis = _trace(name, degree_bits)
    trace = [list(col) for col in trace]
    trace[1][5] = (trace[1][5] + 1) % P
    return trace, pis


@pytest.mark.gpu
def test_a_corrupted_trace_of_c_fails_the_trim(gpu):
    """C has qdf = 3: coefficients 3n .. 4n of the quotient must vanish, and for a trace with one wrong cell they do not"""
    import plonky2_gpu_amd as pg

    trace, pis = _corrupted("C", 4)
    ns = _native(gpu, si.C, 4, 2, si.fri_params(rate_bits=2, arity_bits=(2,)))
    try:
        with pytest.raises(pg.Plonky2HipError) as e:
            ns.prove_bytes(trace, pis)
        assert e.value.code == pg.GL_E_INVALID and "Quotient has failed" in str(e.value)
        good, pis = _trace("C", 4)
        assert ns.prove_bytes(good, pis) == _reference_proof("C", 4, 2, 2, 0, (2,), "poseidon")  # the handle is still usable
    finally:
        ns.close()


@pytest.mark.gpu
def test_a_corrupted_trace_of_d6_fails_the_trim(gpu):
    """qdf 5 in a domain of 8 n: coefficients 5n .. 8n must vanish; after the refusal the handle proves a valid trace"""
    import plonky2_gpu_amd as pg

    trace, pis = _corrupted("D6", 3)
    ns = _native(gpu, si.STARKS["D6"], 3, 3, si.fri_params(rate_bits=3, cap_height=1, arity_bits=(3,)))
    try:
        with pytest.raises(pg.Plonky2HipError) as e:
            ns.prove_bytes(trace, pis)
        assert e.value.code == pg.GL_E_INVALID and "Quotient has failed" in str(e.value)
        good, pis = _trace("D6", 3)
        assert ns.prove_bytes(good, pis) == _reference_proof("D6", 3, 3, 3, 1, (3,), "poseidon")
    finally:
        ns.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_a_corrupted_trace_of_a_and_b_gives_a_proof_the_verifier_rejects(gpu, name):
    """for a power-of-two qdf the reference's trim cannot fail: prove() returns a proof, and verification fails at zeta"""
    from plonky2_gpu_amd import stark as pstark

    stark = si.STARKS[name]
    fp = si.fri_params(rate_bits=2, arity_bits=(2,))
    trace, pis = _corrupted(name, 4)
    ns = _native(gpu, stark, 4, 2, fp)
    try:
        parsed = pstark.proof_from_bytes(ns.prove_bytes(trace, pis), ns.desc)
    finally:
        ns.close()
    with pytest.raises(AssertionError, match="Mismatch between evaluation and opening"):
        sr.verify(HASHERS["poseidon"], stark, 2, fp, parsed)


# ---------------------------------------------------------------- two contexts, two threads
@pytest.mark.gpu
def test_two_proofs_of_one_handle_on_two_contexts_from_two_threads(gpu):
    import plonky2_gpu_amd as pg

    fp = si.fri_params(rate_bits=2, cap_height=1, arity_bits=(2, 2))
    traces = [si.B.make_trace(8, seed=s) for s in (1, 2)]
    ns = _native(gpu, si.B, 8, 2, fp)
    other = pg.Context(0)
    try:
        alone = [ns.prove_bytes(t, p) for t, p in traces]
        assert alone[0] != alone[1]
        got, errors = [None, None], []

        def work(k, ctx):
            try:
                for _ in range(3):
                    got[k] = ns.prove_bytes(traces[k][0], traces[k][1], ctx=ctx)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(k, ctx)) for k, ctx in enumerate((gpu, other))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert got == alone
    finally:
        ns.close()
        other.close()
