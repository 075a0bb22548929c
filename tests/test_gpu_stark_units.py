"""A STARK's constraints compiled as SEVERAL kernel units (gl_stark_compile_units / gl_stark_tables_compile_units, csrc/stark_jit.hip):
the units run in order and hand the consumer's running sums on through the call's output, so everything here is held bit for bit
against the interpreted handle and the references the interpreter is held against. Small programs at small caps: every unit is a
compile of well under 400 instructions.

1. the quotient of fuzz descriptions of 60 and 400 instructions (tests/stark_fuzz.py) on random non-canonical words at caps 16
   and 100: degree_bits 1 (one partly filled block) and 6 with quotient degree factor 4 (two blocks), at column pitch n and n + 3;
2. a hand-made program with a cut directly behind each kind of EMIT, down to one constraint per unit;
3. whole proofs of the hand-written STARKs B and C and of the three-table system, with the permutation and CTL checks in units of
   their own;
4. the memory table as the looked table of a lookup at cap 40;
5. unit 0 of the Keccak-f table's program at cap 600 as a STARK of its own over the table's 2 430 columns;
6. a cap at the program's length: the single kernel's source;
7. the life cycle: the unit count, compile twice, trim, close, a damaged cache entry of a middle unit, two threads on two contexts.

Every compilation goes to a kernel cache in a temporary directory: the shipped cache is a build product."""
import functools
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_instances as ci  # noqa: E402
import representatives as rep  # noqa: E402
import stark_fuzz as sf  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
import test_gpu_ctl as tgc  # noqa: E402  (_reference: the reference proofs, proved once)
import test_gpu_memory_table as tgm  # noqa: E402  (_Cpu, _ops: the two-table system of the memory lookup)
import test_gpu_stark as tgs  # noqa: E402  (_reference_proof, _trace: the reference proofs, proved once)
import test_gpu_stark_fuzz as tgsf  # noqa: E402  (_desc)
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = sr.P


def _objects(cache):
    return sorted(f for f in os.listdir(cache) if f.startswith("stark_") and f.endswith(".hsaco"))


def _program_units(desc, cap):
    from plonky2_gpu_amd.stark import split_program

    return len(split_program(desc, cap))


def _check_unit_sources(ns):
    """unit 0 starts the sums at 0, every later one loads them; every unit but the last stores them raw, the last runs the tail"""
    sources = ns.unit_sources
    assert len(sources) == ns.num_units >= 1 and ns.kernel_source == sources[0]
    load, store = "sums[c] = p.out[(uint64_t)c * q.size + q.i];", "p.out[(uint64_t)c * q.size + q.i] = sums[c];"
    for k, src in enumerate(sources):
        body = src[src.index('extern "C" __global__'):]
        assert ("sums[c] = 0;" in body) == (k == 0) and (load in body) == (k > 0), k
        assert ("sj::tail(sums, p, q);" in body) == (k == len(sources) - 1) and (store in body) == (k < len(sources) - 1), k


# ---------------------------------------------------------------- 1. quotients on random words
QUOTIENTS = [3, 13]  # 60 and 400 instructions, both with quotient degree factor 4, permutation pairs and 3 public inputs


def test_the_quotient_descriptions_reach_what_the_issue_names():
    cases = [sf.fuzz_case(i) for i in QUOTIENTS]
    assert [sf.LENGTHS[i] for i in QUOTIENTS] == [60, 400]
    assert all(sr.quotient_degree_factor(c["stark"]) == 4 and any(c["stark"].pairs) and c["stark"].num_public_inputs == 3 for c in cases)
    assert [c["num_challenges"] for c in cases] == [4, 2]


@functools.lru_cache(maxsize=None)
def _quotient_case(i, degree_bits):
    """description i at another degree, its inputs as ANY u64 words (half of the liftable ones lifted by p), the reference's answer"""
    case = dict(sf.fuzz_case(i), degree_bits=degree_bits)
    trace, zs, sets, alphas, pis = sf.fuzz_inputs(i, case)
    rng = np.random.default_rng(100 * i + degree_bits)
    small = lambda shape: rng.integers(0, rep.LIFTABLE, size=shape, dtype=np.uint64)  # noqa: E731
    mask = rng.random(trace.shape) < 0.3  # uniform words are almost never liftable: a third become small ones
    trace = np.where(mask, small(trace.shape), trace)
    zs = np.where(rng.random(zs.shape) < 0.3, small(zs.shape), zs)
    exp = sf.reference_quotient(case, trace, zs, sets, alphas, pis)
    trace, lifted = rep.lift(trace, rng)
    zs, more = rep.lift(zs, rng)
    assert lifted and more
    return case, trace, zs, sets, alphas, pis, exp


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits", [1, 6])
@pytest.mark.parametrize("cap", [16, 100])
@pytest.mark.parametrize("i", QUOTIENTS)
def test_quotient_in_units_on_random_words(gpu, i, cap, degree_bits):
    import plonky2_gpu_amd as pg

    case, trace, zs, sets, alphas, pis, exp = _quotient_case(i, degree_bits)
    desc = tgsf._desc(case)
    interpreted = pg.NativeStark(gpu, desc)
    units = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=cap)
    try:
        assert units.is_compiled and not interpreted.is_compiled and interpreted.num_units == 0
        assert units.num_units >= _program_units(desc, cap) and units.num_units > 1
        _check_unit_sources(units)
        n_ext = trace.shape[1]
        for stride in (n_ext, n_ext + 3):
            t, z = Strided(gpu, trace, stride), Strided(gpu, zs, stride)
            got = units.quotient_polys(t.ptr, z.ptr, stride, alphas, sets, pis)
            ref = interpreted.quotient_polys(t.ptr, z.ptr, stride, alphas, sets, pis)
            assert (t.polys() == trace).all() and (z.polys() == zs).all()  # guards and pads: only read
            t.free()
            z.free()
            assert (ref == exp).all()
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("column pitch", stride, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad), units.num_units)
    finally:
        interpreted.close()
        units.close()


# ---------------------------------------------------------------- 2. cuts next to each EMIT kind
def _emit_kinds_case():
    """r9 = column 0 is read by every constraint; a transition, a first-row, a last-row and a plain constraint, twice over"""
    instrs = [(sr.LOAD_WIRE, 9, 0, 0), (sr.LOAD_PI, 8, 0, 0)]
    for k, kind in enumerate((sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW, sr.EMIT) * 2):
        instrs += [(sr.LOAD_NEXT, 1, k % 3, 0), (sr.MUL, 2, 1, 9), (sr.SUB, 2, 2, 8), (kind, 0, 2, 0)]
    stark = sf.FuzzStark(3, 1, 3, [], np.array(instrs, dtype=np.uint16), [])
    return dict(stark=stark, degree_bits=3, rate_bits=1, num_challenges=3)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 5, 10, 11])
def test_cuts_behind_each_kind_of_emit(gpu, cap):
    """cap 1 and 5: every constraint is a unit of its own (its slice has 6 instructions, the two shared loads among them), a cut
    behind every kind; cap 10: two constraints a unit (2 + 4 + 4), the cuts behind the first-row and the plain ones; cap 11 as 10"""
    import plonky2_gpu_amd as pg

    case = _emit_kinds_case()
    trace, zs, sets, alphas, pis = sf.fuzz_inputs(77, case)
    exp = sf.reference_quotient(case, trace, zs, sets, alphas, pis)
    desc = tgsf._desc(case)
    ns = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=cap)
    try:
        assert ns.num_units == _program_units(desc, cap) == {1: 8, 5: 8, 10: 4, 11: 4}[cap]
        _check_unit_sources(ns)
        kinds = ["q.z_last" in s[s.index('extern "C"'):] for s in ns.unit_sources]
        assert any(kinds) and not all(kinds)
        d_t = pg.DeviceBuffer.from_host(gpu, trace)
        assert (ns.quotient_polys(d_t, None, trace.shape[1], alphas, None, pis) == exp).all()
    finally:
        ns.close()


# ---------------------------------------------------------------- 3. whole proofs
PROOFS = [("B", 3, 1, 1, 0, (1, 2), "poseidon"), ("B", 3, 3, 2, 0, (3,), "keccak"), ("C", 3, 2, 2, 0, (1, 2), "poseidon")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,degree_bits,num_challenges,rate_bits,cap_height,arity_bits,hasher", PROOFS)
def test_proof_bytes_in_units_equal_the_interpreted_and_the_reference(gpu, name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher):
    import plonky2_gpu_amd as pg

    assert (name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher) in tgs.PROOFS
    fp = si.fri_params(rate_bits=rate_bits, cap_height=cap_height, arity_bits=arity_bits)
    trace, pis = tgs._trace(name, degree_bits)
    exp = tgs._reference_proof(name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher)
    desc = si.STARKS[name].desc(degree_bits, num_challenges, fp)
    interpreted = pg.NativeStark(gpu, desc, hasher)
    units = pg.NativeStark(gpu, desc, hasher, compiled=True, unit_instrs=6)
    try:
        program_units = _program_units(desc, 6)
        assert program_units > 1 and (units.num_units > program_units if desc.pairs else units.num_units == program_units)
        _check_unit_sources(units)
        assert interpreted.prove_bytes(trace, pis) == exp
        assert units.prove_bytes(trace, pis) == exp
    finally:
        interpreted.close()
        units.close()


@pytest.mark.gpu
def test_tables_in_units_equal_the_interpreted_and_the_reference(gpu):
    """tests/ctl_instances.py under Poseidon with 2 challenges at cap 8: a CTL Z's pair of checks generates more than 8 field
    operations, so every CTL Z is a unit of its own behind the program's"""
    import plonky2_gpu_amd as pg

    system, nch, fp, hasher, exp = tgc._reference(0)
    desc = system.desc(ci.DEGREE_BITS, nch, fp)
    traces = ci.make_traces(0)
    interpreted = pg.NativeStarkTables(gpu, desc, "poseidon")
    units = pg.NativeStarkTables(gpu, desc, "poseidon", compiled=True, unit_instrs=8)
    try:
        assert interpreted.num_units == [0, 0, 0] and interpreted.unit_sources is None
        for k, table in enumerate(desc.tables):
            assert units.num_units[k] >= _program_units(table, 8) + desc.num_ctl_zs(k) and desc.num_ctl_zs(k) > 0, (k, units.num_units)
            ctl = [s for s in units.unit_sources[k] if "p.ctl_beta" in s[s.index('extern "C"'):]]
            assert len(ctl) == desc.num_ctl_zs(k) and units.unit_sources[k][-1] in ctl
        assert interpreted.prove_bytes(traces) == exp
        assert units.prove_bytes(traces) == exp
        units.trim()
        assert units.prove_bytes(traces) == exp
    finally:
        interpreted.close()
        units.close()


# ---------------------------------------------------------------- 4. the memory table
@pytest.mark.gpu
def test_the_memory_table_as_a_looked_table_in_units(gpu):
    """the two-table system of tests/test_gpu_memory_table.py: 23 constraints, two permutation pairs and a filtered lookup over 13
    columns, every table in units of at most 40"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import memory_table as mt
    from plonky2_gpu_amd.stark import CrossTableLookup, CtlColumn, StarkDesc, StarkTablesDesc, TableWithColumns

    w = tgm._ops("provable", 14)
    order = [mt.IS_READ, mt.ADDR_CONTEXT, mt.ADDR_SEGMENT, mt.ADDR_VIRTUAL] + [mt.value_limb(i) for i in range(8)] + [mt.TIMESTAMP]
    cpu_rows = [[int(op[c]) for c in order] + [1] for op in w] + [[0] * 14, [7] * 13 + [0]]
    cpu_trace = [[r[c] for r in cpu_rows] for c in range(14)]
    cpu = tgm._Cpu()
    lookups = [CrossTableLookup([TableWithColumns(0, [CtlColumn.single(c) for c in range(13)], CtlColumn.single(13))],
                                TableWithColumns(1, mt.ctl_data(), mt.ctl_filter()))]
    fps = [si.fri_params(rate_bits=1, cap_height=1, arity_bits=(2,), num_query_rounds=4, proof_of_work_bits=2) for _ in range(2)]
    desc = StarkTablesDesc([StarkDesc(4, 14, 0, 3, 1, fps[0], cpu.instrs, cpu.immediates), mt.stark_desc(5, 1, fps[1])], lookups)
    interpreted = pg.NativeStarkTables(gpu, desc)
    units = pg.NativeStarkTables(gpu, desc, compiled=True, unit_instrs=40)
    try:
        assert units.num_units[1] > _program_units(desc.tables[1], 40) > 1
        exp = interpreted.prove_bytes([cpu_trace, mt.generate_trace(gpu, w)])
        assert units.prove_bytes([cpu_trace, mt.generate_trace(gpu, w)]) == exp
    finally:
        interpreted.close()
        units.close()


# ---------------------------------------------------------------- 5. a unit of the Keccak-f table
@pytest.mark.gpu
def test_a_keccak_unit_as_a_stark_of_its_own(gpu):
    """unit 0 of the table's program at cap 600 over the table's 2 430 columns, cut again at cap 150: compiled = interpreted on
    random words. The whole table compiled in units is what tools/bench_keccak_table.py --compiled proves and verifies."""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import keccak_table as kt
    from plonky2_gpu_amd.stark import StarkDesc, split_program

    instrs, imms, _ = kt.native_program()
    fp = si.fri_params(rate_bits=1)
    unit, (first, last) = split_program(StarkDesc(5, kt.NUM_COLUMNS, 0, 3, 2, fp, instrs, imms), 600)[0]
    assert first == 0 and last > 1 and 150 < len(unit) <= 600
    desc = StarkDesc(5, kt.NUM_COLUMNS, 0, 3, 2, fp, unit, imms)
    rng = np.random.default_rng(600)
    lde = rng.integers(0, 1 << 64, size=(kt.NUM_COLUMNS, 64), dtype=np.uint64)
    alphas = [int(x) for x in rng.integers(0, 1 << 64, size=2, dtype=np.uint64)]
    interpreted = pg.NativeStark(gpu, desc)
    units = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=150)
    try:
        assert units.num_units == _program_units(desc, 150) > 1
        d_t = pg.DeviceBuffer.from_host(gpu, lde)
        exp = interpreted.quotient_polys(d_t, None, 64, alphas, None, [])
        got = units.quotient_polys(d_t, None, 64, alphas, None, [])
        assert exp.shape == (2, 64) and exp.any(axis=1).all() and (exp < np.uint64(P)).all() and (got == exp).all()
    finally:
        interpreted.close()
        units.close()


# ---------------------------------------------------------------- 6. a single unit
@pytest.mark.gpu
def test_a_cap_at_the_program_length_is_the_single_kernel(gpu):
    """C has no permutation pairs: at a cap of its program's length everything is one unit with the source of compile(). B's checks
    do not fit behind its program at that cap; under a cap no description reaches they do."""
    import plonky2_gpu_amd as pg

    for name, cap, units in (("C", None, 1), ("B", None, 2), ("B", 10 ** 6, 1)):
        desc = si.STARKS[name].desc(3, 2, si.fri_params(rate_bits=2))
        cap = len(desc.instrs) if cap is None else cap
        single, cut = pg.NativeStark(gpu, desc, compiled=True), pg.NativeStark(gpu, desc)
        try:
            cut.compile(unit_instrs=cap)
            assert single.num_units == 1 and single.unit_sources == [single.kernel_source]
            assert cut.num_units >= units and (cut.num_units == 1) == (units == 1)
            assert (cut.kernel_source == single.kernel_source) == (units == 1)
        finally:
            single.close()
            cut.close()


# ---------------------------------------------------------------- 7. life cycle
LIFE = ("B", 8, 2, dict(rate_bits=2, cap_height=1, arity_bits=(2, 2)))


@functools.lru_cache(maxsize=None)
def _life_traces():
    return [si.B.make_trace(8, seed=s) for s in (1, 2)]


@pytest.mark.gpu
def test_unit_count_compile_twice_trim_and_close(gpu, kernel_cache):
    import plonky2_gpu_amd as pg

    desc = si.B.desc(LIFE[1], LIFE[2], si.fri_params(**LIFE[3]))
    trace, pis = _life_traces()[0]
    ns = pg.NativeStark(gpu, desc)
    assert ns.num_units == 0 and ns.unit_sources is None and ns.kernel_source is None
    exp = ns.prove_bytes(trace, pis)
    ns.compile(unit_instrs=7)
    sources, objects = ns.unit_sources, _objects(kernel_cache)
    assert ns.num_units == len(sources) > 3
    ns.compile(unit_instrs=3)  # a no-op: the handle is compiled
    ns.compile()
    assert ns.unit_sources == sources and _objects(kernel_cache) == objects
    assert ns.prove_bytes(trace, pis) == exp
    ns.trim()
    assert ns.prove_bytes(trace, pis) == exp
    ns.close()
    ns.close()
    again = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=7)  # out of the cache
    try:
        assert again.unit_sources == sources and _objects(kernel_cache) == objects and again.prove_bytes(trace, pis) == exp
    finally:
        again.close()
    default = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=0)  # the library's cap: far above this program and its checks
    try:
        assert default.num_units == 1 and default.prove_bytes(trace, pis) == exp
    finally:
        default.close()


@pytest.mark.gpu
def test_a_damaged_middle_unit_leaves_the_handle_interpreted(gpu, tmp_path):
    """the cache holds the code object of a middle unit cut short: the library refuses to load it and says which file it was, no
    unit is loaded or launched, and the handle proves interpreted; with the whole file it compiles"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import stark as pstark

    desc = si.C.desc(3, 2, si.fri_params(rate_bits=2, arity_bits=(1, 2)))
    trace, pis = tgs._trace("C", 3)
    exp = tgs._reference_proof("C", 3, 2, 2, 0, (1, 2), "poseidon")
    saved = os.environ["PLONKY2_HIP_KERNEL_CACHE"]
    os.environ["PLONKY2_HIP_KERNEL_CACHE"] = str(tmp_path)
    try:
        pstark.precompile(desc, unit_instrs=6)
        probe = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=6)
        sources = probe.unit_sources
        probe.close()
        assert len(sources) >= 3 and len(_objects(str(tmp_path))) == len(sources)
        by_source = {open(os.path.join(str(tmp_path), f)).read(): f[:-4] + ".hsaco" for f in os.listdir(str(tmp_path)) if f.endswith(".hip")}
        name = by_source[sources[1]]  # the second of at least three
        assert name in _objects(str(tmp_path))
        path = os.path.join(str(tmp_path), name)
        whole = open(path, "rb").read()
        with open(path, "wb") as f:
            f.write(whole[: len(whole) // 2])
        ns = pg.NativeStark(gpu, desc)
        try:
            with pytest.raises(pg.Plonky2HipError) as e:
                ns.compile(unit_instrs=6)
            assert e.value.code == pg.GL_E_INVALID and name in str(e.value)
            assert not ns.is_compiled and ns.num_units == 0 and ns.unit_sources is None
            assert ns.prove_bytes(trace, pis) == exp
            with open(path, "wb") as f:
                f.write(whole)
            ns.compile(unit_instrs=6)
            assert ns.num_units == len(sources) and ns.prove_bytes(trace, pis) == exp
        finally:
            ns.close()
    finally:
        os.environ["PLONKY2_HIP_KERNEL_CACHE"] = saved


@pytest.mark.gpu
def test_one_handle_in_units_on_two_contexts_from_two_threads(gpu):
    import plonky2_gpu_amd as pg

    desc = si.B.desc(LIFE[1], LIFE[2], si.fri_params(**LIFE[3]))
    traces = _life_traces()
    ns = pg.NativeStark(gpu, desc, compiled=True, unit_instrs=7)
    other = pg.Context(0)
    try:
        assert ns.num_units > 3
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
