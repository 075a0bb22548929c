"""Device STARK proofs at the sizes the benchmarks prove (tools/bench_stark_prove.py, tools/bench_keccak_table.py), held against the
reference in two ways:

1. VERIFIER-PINNED: the proof of the device is parsed and handed to the reference verifier (tests/stark_ref.py verify,
   tests/ctl_ref.py verify_tables), which must accept it. The verifier shares no line with the prover: a wrong quotient value at
   any point, a wrong opening, a wrong fold or a wrong Merkle path is rejected except with negligible probability at 84 queries.
   fibonacci at 2^12, 2^16, 2^20 rows; wide at 2^12, 2^16; counter (tests/stark_scale.py) at 2^21, 2^22, 2^23 — the last is the
   largest description gl_stark_create accepts; the benchmark's three-table `ctl` system; the Keccak-f table at 2^12 and 2^14 rows.
   With rate_bits 1 the LDEs have 2^13 (the first two-pass NTT), 2^17, 2^21 (the wide-tile plan) and 2^22 .. 2^24 points (the
   special and three-pass plans). One negative control at size: a flipped cell of `wide` at 2^16 rows is rejected at zeta.
2. BYTE-PINNED: where the reference PROVER reaches, the bytes are equal: the STARKs A and B of tests/stark_instances.py under
   standard_fast_config parameters, through an interpreted and through a compiled handle. The reference's times on the CPU that
   wrote this (oracle.accel.c_backend: hashes, trees and transforms in C, the algebra Python):
       A at 2^12 rows, Poseidon, 2 challenges     5.2 s
       B at 2^13 rows, Poseidon, 2 challenges    11.3 s
       B at 2^12 rows, Keccak, 1 challenge        7.3 s  (under the 30 s at which the case would have gone down to 2^11 rows)
3. The compiled quotient kernel beyond 2^12 points, where sj::root_pow first multiplies by its low-level table: compiled bytes =
   interpreted bytes for fibonacci, wide and ctl at every size of 1., and `dense` (1 466 instructions, ACC / ACCR) through
   quotient_polys on random words at 2^12 and 2^16 rows, compiled = interpreted, at the tight and at a padded column pitch and
   once on non-canonical words. There is no Python reference for `dense` at 2^13 points; the interpreter is what 1. and 2. pin.
   The Keccak table is not handed to the compiler.
4. CPU-side pins of the adaptor, the counter STARK and the list of sizes: not marked gpu.

All parameters are starky's standard_fast_config (2 challenges unless said, rate_bits 1, cap_height 4, 16 proof-of-work bits,
arity 16 down to 2^5, 84 queries). Every test prints the proof's size, the time of one device proof and the time of the
verification; none of those is asserted. Every compilation goes to a kernel cache in a temporary directory."""
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_ref as cr  # noqa: E402
import generic_prove_ref as gr  # noqa: E402
import representatives as rep  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
import stark_scale as ss  # noqa: E402
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from stark_scale import bkt, bsp  # noqa: E402
from strided import Strided  # noqa: E402

P = sr.P
HASHERS = {"poseidon": gr.PoseidonHasher(), "keccak": gr.KeccakHasher()}
_BUILT, _BYTES = {}, {}  # per case: (description, trace in HBM, public inputs) and the interpreted handle's proof


@pytest.fixture(scope="module", autouse=True)
def built_traces_freed():
    """behind the module the traces it kept in HBM are freed"""
    yield
    for built in _BUILT.values():
        for d_trace in built[1] if isinstance(built[1], list) else [built[1]]:
            d_trace.free()
    _BUILT.clear(), _BYTES.clear()


def _report(case, data, device_ms, verify_s=None):
    print("scale: %s: %d bytes, one device proof %.1f ms%s" % (case, len(data), device_ms, "" if verify_s is None else ", CPU verification %.2f s" % verify_s))


def _built(gpu, shape, degree_bits):
    """the benchmark's (description, trace in HBM, public inputs), built once and only read afterwards"""
    key = (shape, degree_bits)
    if key not in _BUILT:
        _BUILT[key] = ss.MAKERS[shape](gpu, degree_bits)
    return _BUILT[key]


def _prove_twice(prove, case):
    """two proofs of one handle — the second on recycled pool buffers —, equal; (bytes, milliseconds of the second)"""
    first = prove()
    t0 = time.perf_counter()
    again = prove()
    ms = (time.perf_counter() - t0) * 1e3
    assert again == first, (case, "the second proof of the handle differs from the first")
    return first, ms


def _interpreted_bytes(gpu, shape, degree_bits):
    import plonky2_gpu_amd as pg

    key = (shape, degree_bits)
    if key not in _BYTES:
        desc, d_trace, pis = _built(gpu, shape, degree_bits)
        ns = pg.NativeStark(gpu, desc)
        try:
            assert not ns.is_compiled
            _BYTES[key] = _prove_twice(lambda: ns.prove_bytes(d_trace, pis), key)
        finally:
            ns.close()
    return _BYTES[key]


def _verify(desc, data, hasher="poseidon"):
    """the reference verifier on the parsed bytes: (True or AssertionError, seconds)"""
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    parsed = pstark.proof_from_bytes(data, desc, hasher)
    stark = ss.RefStark(desc)
    t0 = time.perf_counter()
    with accel.c_backend():
        # Keccak trees: the same hasher with the queries' Merkle paths hashed in numpy batches (tests/stark_scale.py KeccakAtOnce)
        h = HASHERS[hasher] if hasher == "poseidon" else ss.keccak_at_once(stark, desc.num_challenges, desc.fri_params, parsed)
        ok = sr.verify(h, stark, desc.num_challenges, desc.fri_params, parsed)
    return ok, time.perf_counter() - t0


# ---------------------------------------------------------------- 1. proofs the reference verifier must accept
@pytest.mark.gpu
@pytest.mark.parametrize("shape,degree_bits", ss.ACCEPTED)
def test_the_reference_verifier_accepts_the_device_proof(gpu, shape, degree_bits):
    """fibonacci: one permutation pair, qdf 1; wide: 100 columns, qdf 2 — a quotient domain of 2^13 points and more, where root_pow
    multiplies by its low-level table; counter: LDEs of 2^22, 2^23 and 2^24 points, Z scans over 2048 to 8192 blocks, query indices of
    22 to 24 bits, the next row's wrap in a domain of 2^21 and more"""
    desc = _built(gpu, shape, degree_bits)[0]
    assert desc.fri_params == bsp.fast_config_fri_params(degree_bits) and desc.num_challenges == 2
    data, ms = _interpreted_bytes(gpu, shape, degree_bits)
    ok, seconds = _verify(desc, data)
    _report("%s 2^%d" % (shape, degree_bits), data, ms, seconds)
    assert ok is True


@pytest.mark.gpu
def test_the_reference_verifier_accepts_the_ctl_system(gpu):
    """the benchmark's three tables of 100, 30 and 8 columns at 2^18, 2^16 and 2^14 rows with four lookups (4, 4 and 8 CTL Zs): the
    CTL-Z scan over 256 blocks, the one transcript across the tables, the cross-table product"""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    desc, traces = _ctl(gpu)
    assert [(d.num_columns, d.degree_bits) for d in desc.tables] == [(100, 18), (30, 16), (8, 14)] and len(desc.lookups) == 4
    nt = pg.NativeStarkTables(gpu, desc)
    try:
        assert not nt.is_compiled
        data, ms = _BYTES["ctl"] = _prove_twice(lambda: nt.prove_bytes(traces), "ctl")
    finally:
        nt.close()
    parsed = pstark.tables_proof_from_bytes(data, desc)
    t0 = time.perf_counter()
    with accel.c_backend():
        ok = cr.verify_tables(HASHERS["poseidon"], ss.RefSystem(desc), 2, [d.fri_params for d in desc.tables], parsed)
    _report("ctl 2^18 + 2^16 + 2^14", data, ms, time.perf_counter() - t0)
    assert ok is True


def _ctl(gpu):
    if "ctl" not in _BUILT:
        desc, _, traces = bsp.ctl_system(gpu)
        _BUILT["ctl"] = (desc, traces)
    return _BUILT["ctl"]


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits,hasher,num_challenges", ss.KECCAK_TABLE)
def test_the_reference_verifier_accepts_the_keccak_table(gpu, degree_bits, hasher, num_challenges):
    """the benchmark's inputs: 170 permutations in 2^12 rows, 682 in 2^14, in each the padding permutation behind them cut after 16
    rounds; the trace built on the device, 2430-wide leaves, the 47 227-instruction program on 2^13 and 2^15 points. Keccak trees
    cannot hash the 4-element quotient leaves of 2 challenges: 1 there."""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import keccak_table as kt

    n = 1 << degree_bits
    inputs = bkt.inputs_for(degree_bits)
    assert inputs.shape == ({12: 170, 14: 682}[degree_bits], 25) and n - 24 * inputs.shape[0] == 16
    desc = kt.stark_desc(degree_bits, num_challenges, bkt.fast_config_fri_params(degree_bits))
    assert desc.fri_params == bsp.fast_config_fri_params(degree_bits)
    d_trace = kt.generate_trace(gpu, inputs, degree_bits)
    ns = pg.NativeStark(gpu, desc, hasher)
    try:
        data, ms = _prove_twice(lambda: ns.prove_bytes(d_trace, []), ("keccak table", degree_bits, hasher))
    finally:
        ns.close()
        d_trace.free()
    ok, seconds = _verify(desc, data, hasher)
    _report("keccak table 2^%d, %s, %d challenge(s)" % (degree_bits, hasher, num_challenges), data, ms, seconds)
    assert ok is True


@pytest.mark.gpu
def test_a_flipped_cell_of_wide_at_2_16_rows_is_rejected(gpu):
    """the negative control at size: quotient_degree_factor 2 is a power of two, so the trim cannot fail and the device returns a
    proof of the violated trace, as the reference's prover does; the verifier rejects it at zeta"""
    import plonky2_gpu_amd as pg

    degree_bits = 16
    n = 1 << degree_bits
    desc, d_good, pis = _built(gpu, "wide", degree_bits)
    column, row = 3, n - 3  # c of the first triple
    d_trace = pg.DeviceBuffer.from_host(gpu, d_good.download())  # the shared trace stays as it is
    ns = pg.NativeStark(gpu, desc)
    try:
        cell = d_trace.download(column * n + row, 1)
        d_trace.upload(cell ^ np.uint64(1), column * n + row)
        data = ns.prove_bytes(d_trace, pis)
    finally:
        ns.close()
        d_trace.free()
    assert data != _interpreted_bytes(gpu, "wide", degree_bits)[0]
    with pytest.raises(AssertionError, match="Mismatch between evaluation and opening"):
        _verify(desc, data)


# ---------------------------------------------------------------- 2. byte equality where the reference prover reaches
BYTE_PINNED = [("A", 12, 2, "poseidon"), ("B", 13, 2, "poseidon"), ("B", 12, 1, "keccak")]


@functools.lru_cache(maxsize=None)
def _instance_trace(name, degree_bits):
    return si.STARKS[name].make_trace(degree_bits, seed=degree_bits)


@functools.lru_cache(maxsize=None)
def _reference_proof(name, degree_bits, num_challenges, hasher):
    from oracle import accel

    trace, pis = _instance_trace(name, degree_bits)
    t0 = time.perf_counter()
    with accel.c_backend():
        data = sr.proof_bytes(HASHERS[hasher], sr.prove(HASHERS[hasher], si.STARKS[name], num_challenges, bsp.fast_config_fri_params(degree_bits), trace, pis))
    print("scale: reference proof of %s at 2^%d rows, %s: %.1f s on the CPU" % (name, degree_bits, hasher, time.perf_counter() - t0))
    return data


@pytest.mark.gpu
@pytest.mark.parametrize("name,degree_bits,num_challenges,hasher", BYTE_PINNED)
def test_proof_bytes_equal_the_reference_under_fast_config(gpu, name, degree_bits, num_challenges, hasher):
    """A has qdb 0: at 2^12 rows its quotient domain has 2^12 points and its LDE 2^13; B has qdb 1: quotient domains of 2^13 and 2^14
    points, three pairs, every opcode. Two arity-16 reductions, 84 queries, 16 proof-of-work bits, cap height 4."""
    import plonky2_gpu_amd as pg

    trace, pis = _instance_trace(name, degree_bits)
    exp = _reference_proof(name, degree_bits, num_challenges, hasher)
    desc = si.STARKS[name].desc(degree_bits, num_challenges, bsp.fast_config_fri_params(degree_bits))
    d_trace = pg.DeviceBuffer.from_host(gpu, np.array(trace, dtype=np.uint64))
    interpreted = pg.NativeStark(gpu, desc, hasher)
    compiled = pg.NativeStark(gpu, desc, hasher, compiled=True)
    try:
        assert not interpreted.is_compiled and compiled.is_compiled
        data, ms = _prove_twice(lambda: interpreted.prove_bytes(d_trace, pis), (name, degree_bits, hasher))
        _report("%s 2^%d, %s" % (name, degree_bits, hasher), data, ms)
        assert data == exp
        assert compiled.prove_bytes(d_trace, pis) == exp
    finally:
        interpreted.close()
        compiled.close()
        d_trace.free()


# ---------------------------------------------------------------- 3. the compiled kernel beyond 2^12 points
@pytest.mark.gpu
@pytest.mark.parametrize("shape,degree_bits", ss.COMPILED)
def test_compiled_proof_bytes_equal_the_interpreted(gpu, shape, degree_bits):
    """what the verifier accepted carries over to the compiled path"""
    import plonky2_gpu_amd as pg

    desc, d_trace, pis = _built(gpu, shape, degree_bits)
    exp = _interpreted_bytes(gpu, shape, degree_bits)[0]
    ns = pg.NativeStark(gpu, desc, compiled=True)
    try:
        assert ns.is_compiled and "stark_quotient_kernel" in ns.kernel_source
        data, ms = _prove_twice(lambda: ns.prove_bytes(d_trace, pis), (shape, degree_bits, "compiled"))
    finally:
        ns.close()
    _report("%s 2^%d, compiled" % (shape, degree_bits), data, ms)
    assert data == exp


@pytest.mark.gpu
def test_compiled_ctl_proof_bytes_equal_the_interpreted(gpu):
    import plonky2_gpu_amd as pg

    desc, traces = _ctl(gpu)
    if "ctl" not in _BYTES:
        nt = pg.NativeStarkTables(gpu, desc)
        try:
            _BYTES["ctl"] = _prove_twice(lambda: nt.prove_bytes(traces), "ctl")
        finally:
            nt.close()
    nt = pg.NativeStarkTables(gpu, desc, compiled=True)
    try:
        assert nt.is_compiled and len(nt.kernel_source) == 3
        data, ms = _prove_twice(lambda: nt.prove_bytes(traces), "ctl compiled")
    finally:
        nt.close()
    _report("ctl, compiled", data, ms)
    assert data == _BYTES["ctl"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits,lifted", [(12, False), (12, True), (16, False)])
def test_compiled_quotient_of_dense_equals_the_interpreted(gpu, degree_bits, lifted):
    """1 466 instructions with ACC / ACCR on 2^13 and 2^17 points of uniformly random words (every constraint non-zero), at the tight
    and at a padded column pitch. lifted: mostly small words (representatives.field_data) and every one that has a second
    representative word + p given that one, alphas too: compiled = interpreted = interpreted on the canonical words."""
    import plonky2_gpu_amd as pg

    desc = bsp.dense_desc(degree_bits)
    assert desc.instrs.shape[0] == 1466 and desc.quotient_degree_bits == 1 and {9, 10} <= set(desc.instrs[:, 0].tolist())  # ACC, ACCR
    n_ext = 1 << (degree_bits + 1)
    rng = np.random.default_rng(1466 + degree_bits)
    alphas = [int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)]
    canonical = None
    if lifted:
        canonical = rep.field_data(rng, (desc.num_columns, n_ext))
        lde, count = rep.lift(canonical, rng, frac=1.0)
        assert count > lde.size // 2 and not (lde[canonical < rep.LIFTABLE] < np.uint64(P)).any()
        alphas[0] = alphas[0] % rep.LIFTABLE
        lifted_alphas = [rep.lift_scalar(a) for a in alphas]
    else:
        lde = rng.integers(0, P, size=(desc.num_columns, n_ext), dtype=np.uint64)
    interpreted = pg.NativeStark(gpu, desc)
    compiled = pg.NativeStark(gpu, desc, compiled=True)
    try:
        assert not interpreted.is_compiled and compiled.is_compiled
        exp = None
        for stride in (n_ext, n_ext + 6):
            t = Strided(gpu, lde, stride)
            got = [ns.quotient_polys(t.ptr, None, stride, lifted_alphas if lifted else alphas, None, []) for ns in (interpreted, compiled)]
            assert (t.polys() == lde).all()  # guards and pads: only read
            t.free()
            exp = got[0] if exp is None else exp
            assert got[0].shape == (2, n_ext) and got[0].all() and rep.all_canonical(got[0])
            assert (got[0] == exp).all(), ("the interpreter at column pitch", stride, "differs from itself at the tight pitch")
            bad = np.argwhere(got[1] != exp)
            assert bad.size == 0, ("column pitch", stride, "first (challenge, coefficient) where compiled differs", bad[0].tolist(), len(bad))
        if lifted:
            t = Strided(gpu, canonical, n_ext)
            assert (interpreted.quotient_polys(t.ptr, None, n_ext, alphas, None, []) == exp).all()
            t.free()
    finally:
        interpreted.close()
        compiled.close()


# ---------------------------------------------------------------- 4. CPU-side pins
@functools.lru_cache(maxsize=None)
def _host_fibonacci(degree_bits):
    """the benchmark's fibonacci with the upload replaced by the host array itself: (description, [4][n] uint64, public inputs)"""
    import plonky2_gpu_amd as pg

    saved = pg.DeviceBuffer.__dict__["from_host"]
    pg.DeviceBuffer.from_host = classmethod(lambda cls, ctx, arr: arr)
    try:
        return bsp.fibonacci(None, degree_bits)
    finally:
        pg.DeviceBuffer.from_host = saved


@functools.lru_cache(maxsize=None)
def _host_fibonacci_proof():
    from oracle import accel

    desc, trace, pis = _host_fibonacci(10)
    with accel.c_backend():
        proof = sr.prove(HASHERS["poseidon"], ss.RefStark(desc), 2, desc.fri_params, [[int(v) for v in col] for col in trace], pis)
    return desc, sr.proof_bytes(HASHERS["poseidon"], proof)


def test_the_adaptor_and_the_verifier_accept_a_reference_made_proof():
    desc, data = _host_fibonacci_proof()
    assert (desc.instrs == si.A.instrs).all() and desc.pairs == si.A.pairs and desc.fri_params["reduction_arity_bits"] == [4]
    assert _verify(desc, data)[0] is True


def test_the_adaptor_and_the_verifier_reject_a_changed_opening():
    """one opened value of the trace at zeta, one of the quotient, one word of a Merkle path's leaf: each is caught"""
    from plonky2_gpu_amd import stark as pstark

    desc, data = _host_fibonacci_proof()
    for where in ("local_values", "quotient_polys"):
        proof = pstark.proof_from_bytes(data, desc)
        x = proof["openings"][where][0]
        proof["openings"][where][0] = ((x[0] + 1) % P, x[1])
        with pytest.raises(AssertionError, match="Mismatch between evaluation and opening"):
            _verify(desc, pstark.proof_to_bytes(proof, desc))
    proof = pstark.proof_from_bytes(data, desc)
    evals = proof["opening_proof"]["query_round_proofs"][83]["initial_trees_proof"][0][0]
    evals[0] = (evals[0] + 1) % P
    with pytest.raises(AssertionError):
        _verify(desc, pstark.proof_to_bytes(proof, desc))


def test_the_batched_keccak_hasher_changes_no_verdict():
    """a reference-made proof of B under Keccak trees at 2^6 rows: KeccakAtOnce answers every Merkle hash of the verification from
    its memo, accepts what the plain hasher accepts, and rejects a changed leaf and a changed sibling as the plain hasher does"""
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    fp = si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2, 2), num_query_rounds=6, proof_of_work_bits=2)
    trace, pis = si.B.make_trace(6, seed=6)
    desc = si.B.desc(6, 1, fp)
    with accel.c_backend():
        data = sr.proof_bytes(HASHERS["keccak"], sr.prove(HASHERS["keccak"], si.B, 1, fp, trace, pis))
        proof = pstark.proof_from_bytes(data, desc, "keccak")
        h = ss.keccak_at_once(si.B, 1, fp, proof)
        assert sr.verify(h, si.B, 1, fp, proof) and sr.verify(HASHERS["keccak"], si.B, 1, fp, proof)
        paths = 6 * (3 + 2)
        assert h.hits == sum(1 + len(mp) for rp in proof["opening_proof"]["query_round_proofs"]
                             for _, mp in rp["initial_trees_proof"] + [(0, st["merkle_proof"]) for st in rp["steps"]]) > paths
        assert _verify(desc, data, "keccak")[0] is True
        for tamper in ("leaf", "sibling"):
            bad = pstark.proof_from_bytes(data, desc, "keccak")
            evals, mp = bad["opening_proof"]["query_round_proofs"][5]["initial_trees_proof"][1]
            if tamper == "leaf":
                evals[0] = (evals[0] + 1) % P
            else:
                mp[2] = bytes([mp[2][0] ^ 1]) + bytes(mp[2][1:])
            for hasher in (ss.keccak_at_once(si.B, 1, fp, bad), HASHERS["keccak"]):
                with pytest.raises(AssertionError, match="initial Merkle proof"):
                    sr.verify(hasher, si.B, 1, fp, bad)


def test_the_counter_trace_satisfies_its_constraints():
    """row by row under stark_ref's interpreter with the consumer's selectors on the subgroup (z_last = 0 on the last row, the
    Lagrange selectors 1 on their row), the pair as multisets, and the reference's own prover and verifier at 2^4 rows"""
    from oracle import accel, pyref

    degree_bits = 4
    n = 1 << degree_bits
    trace, pis = ss.counter_trace(degree_bits)
    stark = ss.RefStark(ss.counter_desc(degree_bits))
    assert (stark.num_columns, stark.num_public_inputs, stark.constraint_degree, stark.pairs) == (4, 1, 2, [[(2, 3)]])
    sr.validate_program(stark.instrs, stark.immediates, 4, 1)
    g = pyref.root_of_unity(degree_bits)
    rows = [[int(v) for v in trace[:, r]] for r in range(n)]
    for r in range(n):
        consumer = sr.Consumer(sr.Base, [1], (pow(g, r, P) - pow(g, n - 1, P)) % P, int(r == 0), int(r == n - 1))
        sr.run_program(sr.Base, stark.instrs, stark.immediates, rows[r], rows[(r + 1) % n], pis, consumer)
        assert len(consumer.emitted) == 3 and not any(consumer.emitted), (r, consumer.emitted)
    assert sorted(trace[2].tolist()) == sorted(trace[3].tolist()) and (trace[2] != trace[3]).all()
    assert (trace[1] == trace[0] * trace[0]).all() and int(trace[0, 0]) == pis[0]
    big = ss.COUNTER_START + (1 << 23)
    assert big * big < P  # the squares of the largest size need no reduction: numpy's product is the field's
    fp = bsp.fast_config_fri_params(degree_bits)
    with accel.c_backend():
        proof = sr.prove(HASHERS["poseidon"], stark, 2, fp, [[int(v) for v in col] for col in trace], pis)
        assert sr.verify(HASHERS["poseidon"], stark, 2, fp, proof)
    wrong = trace.copy()
    wrong[1, 5] += np.uint64(1)
    consumer = sr.Consumer(sr.Base, [1], 1, 0, 0)
    sr.run_program(sr.Base, stark.instrs, stark.immediates, [int(v) for v in wrong[:, 5]], [int(v) for v in wrong[:, 6]], pis, consumer)
    assert any(consumer.emitted)


def test_the_sizes_reach_every_ntt_plan_boundary():
    """rate_bits 1: the LDE of a proof at 2^d rows is an NTT of 2^(d + 1) points. csrc/ntt.hip: one kernel up to 2^12, two passes from
    2^13 to 2^20, the wide-tile plan at 2^21, the special and three-pass plans at 2^22 .. 2^24; gl_stark_create accepts up to 24."""
    assert all(bsp.fast_config_fri_params(d)["rate_bits"] == 1 for _, d in ss.ACCEPTED)
    assert {d + 1 for _, d in ss.ACCEPTED} == {13, 17, 21, 22, 23, 24}
    assert {d + 1 for s, d in ss.ACCEPTED if s == "counter"} == {22, 23, 24} and {d + 1 for s, d in ss.ACCEPTED if s == "wide"} == {13, 17}
    assert ss.COMPILED == [c for c in ss.ACCEPTED if c[0] != "counter"] and len(ss.COMPILED) == 5
    assert {d + 1 for _, d in bsp.CTL_TABLES} == {19, 17, 15}
    assert [len(bsp.fast_config_fri_params(d)["reduction_arity_bits"]) for d in (12, 16, 20, 23)] == [2, 3, 4, 5]
    # the quotient domain (degree_bits + qdb) of every byte-pinned and verifier-pinned case but A at 2^12 rows exceeds 2^12 points
    qdb = {"fibonacci": 0, "wide": 1, "counter": 0, "A": 0, "B": 1}
    assert [s for s, d in ss.ACCEPTED if d + qdb[s] <= 12] == ["fibonacci"] and [c[0] for c in BYTE_PINNED if c[1] + qdb[c[0]] <= 12] == ["A"]
