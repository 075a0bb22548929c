"""Multi-table STARKs with cross-table lookups on the device (gl_stark_tables_create / gl_stark_tables_prove and the two kernels alone)
against tests/ctl_ref.py, bit for bit: there is no tolerance anywhere. The three-table system, its traces and the random
descriptions are tests/ctl_instances.py's; the proved cases and the refused descriptions are shared with tests/test_ctl_ref.py. The
reference runs with oracle.accel.c_backend (its Poseidon, trees and transforms in C): the algebra of the STARKs stays Python."""
import functools
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_instances as ci  # noqa: E402
import ctl_ref as cr  # noqa: E402
import stark_ref as sr  # noqa: E402
import test_ctl_ref as tcr  # noqa: E402  (CASES / _case: the reference proofs; REFUSALS)
from gpu_util import gpu  # noqa: E402,F401
from oracle import fri_ref  # noqa: E402
from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, StarkAsm, StarkDesc, StarkTablesDesc, TableWithColumns  # noqa: E402

P = 0xFFFFFFFF00000001
HASHERS = tcr.HASHERS


def _words(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _any_words(rng, *shape):
    """uniform 64-bit words; only one in 2^32 of those is >= p, so one word in eight is then moved into [p, 2^64)"""
    w = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    high = rng.integers(P, 1 << 64, size=shape, dtype=np.uint64)
    return np.where(rng.random(shape) < 0.125, high, w)


def _pairs(rng, k, words=_words):
    return [(int(a), int(b)) for a, b in words(rng, k, 2)]


# ---------------------------------------------------------------- the CTL Zs
def _zs_desc(degree_bits, num_challenges):
    """table 0 (5 columns, 2^degree_bits rows) looks twice into table 1 through lookup 0 — three CTL columns each: a plain column, a
    combination with a large coefficient and a constant, a constant-only column; filters c3 and 1 - c4 — and once through the
    unfiltered lookup 1: 3 * num_challenges CTL Zs"""
    a = StarkAsm()
    a.emit(a.local(0))
    instrs, imms = a.program()
    fp = dict(rate_bits=1, cap_height=0, proof_of_work_bits=0, num_query_rounds=1, reduction_arity_bits=[], hiding=False)
    tables = [StarkDesc(db, 5, 0, 3, num_challenges, fp, instrs, imms) for db in (degree_bits, 1)]
    cols = lambda: [CtlColumn.single(0), CtlColumn.linear_combination([(1, P - 5), (2, 3)], 1 << 40), CtlColumn.constant(9)]  # noqa: E731
    lookups = [CrossTableLookup([TableWithColumns(0, cols(), CtlColumn.single(3)), TableWithColumns(0, cols(), CtlColumn.linear_combination([(4, P - 1)], 1))],
                                TableWithColumns(1, cols(), CtlColumn.single(3))),
               CrossTableLookup([TableWithColumns(0, [CtlColumn.single(1)])], TableWithColumns(1, [CtlColumn.single(1)]))]
    return StarkTablesDesc(tables, lookups)


def _zs_trace(degree_bits, filters, seed):
    """random words; c3 / c4 binary: all 0, all 1 or mixed. "mixed" also holds words >= p: filter words p + 1 (1 as a field
    element) and p (0), and non-canonical words in the value columns"""
    rng = np.random.default_rng(seed)
    n = 1 << degree_bits
    trace = _words(rng, 5, n)
    if filters == "mixed":
        trace[3], trace[4] = rng.integers(0, 2, size=n, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)
        trace[3, ::3] += np.uint64(P)
        trace[4, 1::2] += np.uint64(P)
        trace[0, 0] = P + 5
        trace[1, -1] = 0xFFFFFFFFFFFFFFFF
    else:
        trace[3] = trace[4] = 0 if filters == "all0" else 1
    return trace


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits,num_challenges,filters", [(1, 1, "mixed"), (3, 2, "all0"), (3, 3, "all1"), (3, 1, "mixed"), (10, 2, "mixed"),
                                                               (11, 1, "mixed"), (13, 3, "mixed")])
def test_ctl_zs_equal_the_reference(gpu, degree_bits, num_challenges, filters):
    """2^10 rows: exactly one scan block, 2^11: two, 2^13: eight; the trace at the tight and at a padded pitch"""
    import plonky2_gpu_amd as pg

    desc = _zs_desc(degree_bits, num_challenges)
    trace = _zs_trace(degree_bits, filters, 50 * degree_bits + num_challenges)
    challenges = _pairs(np.random.default_rng(degree_bits), num_challenges)
    exp = np.array(cr.ctl_z_polys(desc.lookups, num_challenges, 0, trace.tolist(), challenges), dtype=np.uint64)
    n = 1 << degree_bits
    assert exp.shape == (3 * num_challenges, n)
    if filters != "mixed":  # c3 = c4: of the two filters c3 and 1 - c4 one selects every row, the other none
        idle = 0 if filters == "all0" else 1
        assert (exp[idle : 2 * num_challenges : 2] == 1).all() and (exp[1 - idle : 2 * num_challenges : 2, -1] != 1).all()
    nt = pg.NativeStarkTables(gpu, desc)
    try:
        for stride in (n, n + 6):
            got = nt.ctl_zs(0, trace, challenges, trace_stride=stride)
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("trace pitch", stride, "first (Z, row) that differs", bad[0].tolist(), len(bad))
    finally:
        nt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits,row", [(3, 5), (11, 1500)])
def test_a_non_binary_filter_is_refused_by_ctl_zs(gpu, degree_bits, row):
    import plonky2_gpu_amd as pg

    trace = _zs_trace(degree_bits, "mixed", 7)
    nt = pg.NativeStarkTables(gpu, _zs_desc(degree_bits, 2))
    try:
        challenges = [(3, 4), (5, 6)]
        nt.ctl_zs(0, trace, challenges)
        trace[4, row] = 2  # 1 - c4 = -1
        with pytest.raises(pg.Plonky2HipError, match="Non-binary filter") as e:
            nt.ctl_zs(0, trace, challenges)
        assert e.value.code == pg._lib.GL_E_INVALID
        trace[4, row] = P + 1
        nt.ctl_zs(0, trace, challenges)  # and the handle works on
    finally:
        nt.close()


# ---------------------------------------------------------------- the quotient with CTL checks, on random words
def _padded(ctx, cols, stride):
    from plonky2_gpu_amd.device import DeviceBuffer

    host = np.zeros((cols.shape[0], stride), dtype=np.uint64)
    host[:, : cols.shape[1]] = cols
    return DeviceBuffer.from_host(ctx, host)


def _check_ctl_quotient(gpu, system, desc, table, degree_bits, rate_bits, num_challenges, seed, words=_words, nt=None):
    """uniform words in place of the two LDEs (neither side needs low degree), random challenges; `words` draws them all (_words:
    below p; _any_words: any u64 — the reference then gets them reduced); `nt`: a handle of `desc` to use instead of a new one"""
    import plonky2_gpu_amd as pg
    from oracle import accel

    rng = np.random.default_rng(seed)
    stark = system.tables[table]
    n_ext = 1 << (degree_bits + rate_bits)
    trace, zs = words(rng, stark.num_columns, n_ext), words(rng, desc.num_zs(table), n_ext)
    sets = [_pairs(rng, num_challenges, words) for _ in range(sr.quotient_degree_factor(stark))] if stark.pairs else None
    ctl_challenges, alphas = _pairs(rng, num_challenges, words), [int(x) for x in words(rng, num_challenges)]
    reduced = lambda a: (a % np.uint64(P)).T.tolist()  # noqa: E731
    mod = lambda pairs: [(a % P, b % P) for a, b in pairs]  # noqa: E731
    with accel.c_backend():
        exp = np.array(cr.compute_quotient_polys(system, table, num_challenges, degree_bits, rate_bits, reduced(trace), reduced(zs),
                                                 sets and [mod(s) for s in sets], mod(ctl_challenges), [a % P for a in alphas]), dtype=np.uint64)
    own = nt is None
    nt = pg.NativeStarkTables(gpu, desc) if own else nt
    try:
        for stride in (n_ext, n_ext + 2):
            got = nt.quotient_polys(table, _padded(gpu, trace, stride), _padded(gpu, zs, stride), stride, alphas, sets, ctl_challenges)
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("table", table, "column pitch", stride, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad))
    finally:
        if own:
            nt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("num_challenges,degree,rate_bits", [(2, 3, 1), (3, 4, 2)])
@pytest.mark.parametrize("table", [0, 1, 2])
def test_ctl_quotient_of_every_table_of_the_system(gpu, table, num_challenges, degree, rate_bits):
    system = ci.system(degree)
    desc = system.desc(ci.DEGREE_BITS, num_challenges, ci.fri_params(rate_bits=rate_bits))
    _check_ctl_quotient(gpu, system, desc, table, ci.DEGREE_BITS[table], rate_bits, num_challenges, 10 * table + num_challenges)


@functools.lru_cache(maxsize=None)
def _random_system(i):
    return ci.RandomSystem(i, *ci.RANDOM_SHAPES[i])


def test_the_random_descriptions_reach_the_shapes_they_are_meant_to():
    """no GPU: (CTL Zs, permutation Zs, qdf, degree_bits) of table 0 of every random description, and the widths of their TWCs"""
    shapes, widths, filtered = [], set(), set()
    for i in range(len(ci.RANDOM_SHAPES)):
        rs = _random_system(i)
        desc = rs.desc()
        desc.validate()
        shapes.append((desc.num_ctl_zs(0), desc.tables[0].num_zs, desc.tables[0].quotient_degree_factor, rs.degree_bits))
        widths |= set(rs.widths)
        filtered |= {lk.looked_table.filter_column is not None for lk in rs.lookups}
    assert shapes == [(1, 0, 2, 1), (2, 2, 2, 2), (3, 1, 2, 3), (3, 0, 2, 4), (2, 1, 3, 1), (1, 1, 3, 2), (2, 0, 3, 3), (3, 1, 3, 4), (3, 2, 4, 1),
                      (3, 0, 4, 2), (2, 1, 4, 3), (1, 1, 4, 4), (1, 1, 2, 3), (2, 0, 4, 2)]
    assert len(shapes) >= 12 and widths == {1, 2, 3, 4, 5} and filtered == {False, True}
    # zero CTL Zs is gl_stark_quotient_polys itself: test_the_quotient_without_ctl_zs_is_the_single_table_quotient


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ci.RANDOM_SHAPES)))
def test_ctl_quotient_of_random_descriptions(gpu, i):
    rs = _random_system(i)
    _check_ctl_quotient(gpu, rs, rs.desc(), 0, rs.degree_bits, rs.rate_bits, rs.num_challenges, 77 + i)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [1, 8])
def test_the_quotient_without_ctl_zs_is_the_single_table_quotient(gpu, i):
    """table 0 of a random description on its own (gl_stark_quotient_polys) against ctl_ref with no lookups: 0 CTL Zs beside 2
    permutation Zs, the same bytes as tests/stark_ref.py's quotient"""
    import plonky2_gpu_amd as pg
    from oracle import accel

    rs = _random_system(i)
    stark, nch, db, rb = rs.tables[0], rs.num_challenges, rs.degree_bits, rs.rate_bits
    alone = ci.System([stark], [], None)
    rng = np.random.default_rng(i)
    n_ext = 1 << (db + rb)
    trace, zs = _words(rng, stark.num_columns, n_ext), _words(rng, sr.num_zs(stark, nch), n_ext)
    sets, alphas = [_pairs(rng, nch) for _ in range(sr.quotient_degree_factor(stark))], [int(x) for x in _words(rng, nch)]
    with accel.c_backend():
        exp = cr.compute_quotient_polys(alone, 0, nch, db, rb, trace.T.tolist(), zs.T.tolist(), sets, [], alphas)
        assert exp == sr.compute_quotient_polys(stark, nch, db, rb, trace.T.tolist(), zs.T.tolist(), sets, [], alphas)
    ns = pg.NativeStark(gpu, rs.desc().tables[0])
    try:
        got = ns.quotient_polys(_padded(gpu, trace, n_ext), _padded(gpu, zs, n_ext), n_ext, alphas, sets, [])
        assert (got == np.array(exp, dtype=np.uint64)).all()
    finally:
        ns.close()


# ---------------------------------------------------------------- whole proofs
@functools.lru_cache(maxsize=None)
def _reference(i):
    from oracle import accel

    with accel.c_backend():
        system, nch, fp, hasher, proofs = tcr._case(i)
        return system, nch, fp, hasher, cr.proofs_bytes(hasher, proofs)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(tcr.CASES)))
def test_proof_bytes_equal_the_reference_and_verify(gpu, i):
    """Poseidon and Keccak with 1 and 2 challenges; case 3: cap_height 3, all the smallest table's LDE of 8 rows allows. The second
    proof of the handle runs on recycled buffers."""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    system, nch, fp, hasher, exp = _reference(i)
    name = tcr.CASES[i][0]
    desc = system.desc(ci.DEGREE_BITS, nch, fp)
    traces = ci.make_traces(i)
    nt = pg.NativeStarkTables(gpu, desc, name)
    try:
        timing = []
        data = nt.prove_bytes(traces, timing=timing)
        assert data == exp
        assert nt.prove_bytes(traces) == exp
        nt.trim()
        assert nt.prove_bytes(traces) == exp
        assert len(timing) == 3 and all(len(t) == 11 and all(v >= 0 for v in t.values()) for t in timing)
    finally:
        nt.close()
    parsed = pstark.tables_proof_from_bytes(data, desc, name)
    assert pstark.tables_proof_to_bytes(parsed, desc, name) == data
    with accel.c_backend():
        assert cr.verify_tables(hasher, system, nch, fp, parsed)


@pytest.mark.gpu
def test_traces_of_non_canonical_words_give_the_bytes_of_their_canonical_twins(gpu):
    import plonky2_gpu_amd as pg

    system, nch, fp, hasher, exp = _reference(0)
    traces = [np.array(t, dtype=np.uint64) for t in ci.make_traces(0)]
    shifted = 0
    for t in traces:
        small = t < np.uint64((1 << 32) - 1)  # word + p still fits 64 bits: the flags, the bits, the counters
        t[small] += np.uint64(P)
        shifted += int(small.sum())
    assert shifted > 60 and int(traces[0][2].max()) == P + 1  # a filter word p + 1 among them
    nt = pg.NativeStarkTables(gpu, system.desc(ci.DEGREE_BITS, nch, fp))
    try:
        assert nt.prove_bytes(traces) == exp
    finally:
        nt.close()


@pytest.mark.gpu
def test_a_corrupted_looked_row_gives_a_proof_the_verifier_rejects(gpu):
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    system, nch, fp, hasher, _ = _reference(0)
    traces = ci.make_traces(0)
    row = traces[1][2].index(0)
    traces[1][0][row] = (traces[1][0][row] + 1) % P
    desc = system.desc(ci.DEGREE_BITS, nch, fp)
    nt = pg.NativeStarkTables(gpu, desc)
    try:
        data = nt.prove_bytes(traces)
    finally:
        nt.close()
    with accel.c_backend():
        assert data == cr.proofs_bytes(hasher, cr.prove_tables(hasher, system, nch, fp, traces, check=False))
        with pytest.raises(AssertionError, match="cross-table lookup"):
            cr.verify_tables(hasher, system, nch, fp, pstark.tables_proof_from_bytes(data, desc))


@pytest.mark.gpu
def test_a_non_binary_filter_is_refused_by_prove(gpu):
    import plonky2_gpu_amd as pg

    system, nch, fp, hasher, exp = _reference(0)
    nt = pg.NativeStarkTables(gpu, system.desc(ci.DEGREE_BITS, nch, fp))
    try:
        for table, column in ((0, 2), (1, 2)):  # a filter of the first table proved, and of a later one
            traces = ci.make_traces(0)
            traces[table][column][3] = 2
            with pytest.raises(pg.Plonky2HipError, match="Non-binary filter") as e:
                nt.prove_bytes(traces)
            assert e.value.code == pg._lib.GL_E_INVALID
        assert nt.prove_bytes(ci.make_traces(0)) == exp  # the handle works on
    finally:
        nt.close()


# ---------------------------------------------------------------- refusals
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(tcr.REFUSALS))
def test_create_refuses(gpu, name):
    import plonky2_gpu_amd as pg

    desc, hasher = tcr.REFUSALS[name]
    with pytest.raises(pg.Plonky2HipError) as e:
        pg.NativeStarkTables(gpu, desc, hasher).close()
    assert e.value.code == pg._lib.GL_E_INVALID and len(str(e.value)) > 30


@pytest.mark.gpu
def test_create_refuses_bad_arrays_and_bad_programs(gpu):
    """what the Python description cannot express: broken bounds, a filter index out of range, another struct_size; and a table whose
    program gl_stark_create would refuse"""
    import plonky2_gpu_amd as pg

    def refused(desc, **edits):
        flat = desc.flatten()
        for key, (index, value) in edits.items():
            flat[key][index] = value
        with pytest.raises(pg.Plonky2HipError) as e:
            pg.NativeStarkTables(gpu, desc, flat=flat).close()
        assert e.value.code == pg._lib.GL_E_INVALID
        return str(e.value)

    desc = ci.system().desc(ci.DEGREE_BITS, 2, ci.fri_params())
    pg.NativeStarkTables(gpu, desc).close()
    assert "h_lookup_bounds" in refused(desc, lookup_bounds=(0, 1))
    assert "h_lookup_bounds" in refused(desc, lookup_bounds=(3, 8))
    assert "h_twc_column_bounds" in refused(desc, twc_column_bounds=(2, 1))
    assert "h_column_bounds" in refused(desc, column_bounds=(4, 2))
    assert "filter column out of range" in refused(desc, twc_filter=(0, 13))
    assert "table out of range" in refused(desc, twc_table=(6, 3))
    assert "out of range for its table" in refused(desc, term_columns=(0, 7))
    bad = ci.system().desc(ci.DEGREE_BITS, 2, ci.fri_params())
    bad.tables[1].instrs = bad.tables[1].instrs.copy()
    bad.tables[1].instrs[0, 0] = 1  # LOAD_CONST
    assert "LOAD_CONST" in refused(bad)


# ---------------------------------------------------------------- the transcript's compact
@pytest.mark.gpu
@pytest.mark.parametrize("observed", [8, 11, 16, 3])
def test_challenger_compact_equals_the_reference(gpu, observed):
    """the input buffer empty (8, 16 elements observed: compact only drops the outputs) and non-empty (11, 3: it duplexes first), then
    more observations and challenges; the device transcript and the host mirror"""
    from plonky2_gpu_amd.challenger import Challenger, DeviceChallenger
    from plonky2_gpu_amd.device import DeviceBuffer

    rng = np.random.default_rng(observed)
    first, second = _words(rng, observed), _words(rng, 5)
    ref = fri_ref.Challenger()
    ref.observe_elements(int(x) for x in first)
    before = ref.get_n_challenges(2)
    cr.compact(ref)
    exp = ref.get_n_challenges(3)
    ref.observe_elements(int(x) for x in second)
    cr.compact(ref)
    exp += ref.get_n_challenges(9)

    dev = DeviceChallenger(gpu)
    assert dev.step([(DeviceBuffer.from_host(gpu, first), observed)], 2) == before
    got = dev.step([], 3, compact=True)
    got += dev.step([(DeviceBuffer.from_host(gpu, second), 5)], 0)
    got += dev.step([], 9, compact=True)
    assert got == exp

    host = Challenger(gpu)
    host.observe_elements(first)
    assert host.get_n_challenges(2) == before
    host.compact()
    got = host.get_n_challenges(3)
    host.observe_elements(second)
    host.compact()
    assert got + host.get_n_challenges(9) == exp


@pytest.mark.gpu
def test_compact_acts_before_the_step_observes(gpu):
    from plonky2_gpu_amd.challenger import DeviceChallenger
    from plonky2_gpu_amd.device import DeviceBuffer

    words = _words(np.random.default_rng(1), 14)
    ref = fri_ref.Challenger()
    ref.observe_elements(int(x) for x in words[:3])
    cr.compact(ref)
    ref.observe_elements(int(x) for x in words[3:])
    exp = ref.get_n_challenges(4)
    dev = DeviceChallenger(gpu)
    dev.step([(DeviceBuffer.from_host(gpu, words[:3]), 3)], 0)
    assert dev.step([(DeviceBuffer.from_host(gpu, words[3:]), 11)], 4, compact=True) == exp


@pytest.mark.gpu
def test_a_step_whose_output_overlaps_the_transcript_is_refused(gpu):
    """the step stores its outputs before the 32 transcript words: an output inside them is GL_E_INVALID whatever the flags, one
    right behind or right before them is accepted"""
    import ctypes

    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    d = pg.DeviceBuffer.from_host(gpu, np.zeros(80, dtype=np.uint64))
    transcript = d.ptr + 8 * 16  # words 16 .. 47
    for out, n_challenges, flags in ((transcript, 0, 4), (transcript + 8 * 31, 1, 1), (transcript - 8 * 2, 3, 1), (transcript - 8 * 3, 0, 3)):
        with pytest.raises(_lib.Plonky2HipError, match="overlaps") as e:
            _lib.call("gl_challenger_step", transcript, None, 0, n_challenges, out, flags, gpu.ptr)
        assert e.value.code == _lib.GL_E_INVALID
    _lib.call("gl_challenger_step", transcript, None, 0, 3, transcript - 8 * 3, 1, gpu.ptr)
    _lib.call("gl_challenger_step", transcript, None, 0, 2, transcript + 8 * 32, 4, gpu.ptr)
    ref = fri_ref.Challenger()
    exp = ref.get_n_challenges(3)
    cr.compact(ref)
    exp2 = ref.get_n_challenges(2)
    words = d.download()
    assert [int(x) for x in words[13:16]] == exp and [int(x) for x in words[48:50]] == exp2
    d.free()


# ---------------------------------------------------------------- two contexts, two threads
@pytest.mark.gpu
def test_two_proofs_of_one_handle_on_two_contexts_from_two_threads(gpu):
    import plonky2_gpu_amd as pg

    system, nch, fp, hasher, exp = _reference(0)
    all_traces = [ci.make_traces(0), ci.make_traces(5)]
    nt = pg.NativeStarkTables(gpu, system.desc(ci.DEGREE_BITS, nch, fp))
    other = pg.Context(0)
    try:
        alone = [nt.prove_bytes(t) for t in all_traces]
        assert alone[0] == exp != alone[1]
        got, errors = [None, None], []

        def work(k, ctx):
            try:
                for _ in range(3):
                    got[k] = nt.prove_bytes(all_traces[k], ctx=ctx)
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
        nt.close()
        other.close()
