"""The compiled STARK quotient kernels (gl_stark_compile / gl_stark_tables_compile, csrc/stark_jit.hip) against the references the
interpreter is held against, bit for bit: there is no tolerance anywhere. A compiled handle replaces the interpreter's kernel by one
generated from the description, so everything here runs the shapes at which that generator can go wrong — the small ones that
exist already:

1. every description of tests/stark_fuzz.py (the parametrisation of tests/test_gpu_stark_fuzz.py) through quotient_polys;
2. three of them with every liftable word of the trace, the Zs, the alphas, the challenges and the public inputs lifted by p;
3. whole proofs of the hand-written STARKs of tests/stark_instances.py: compiled = interpreted = tests/stark_ref.py;
4. the system of tests/ctl_instances.py and the systems 0, 1, 2, 4, 5, 11 and 13 of tests/ctl_fuzz.py: every table's quotient on
   random words against tests/ctl_ref.py and the compiled proof against the interpreted one. What those systems reach is asserted
   on the CPU. The chains of 8 to 17 tables (systems 7 - 10), and the systems 3, 6, 12 and 14, are left out for COMPILE TIME only:
   every table is a hiprtc compilation of two to three seconds and the chains add nothing the generator sees differently;
5. the life cycle: compile twice, trim, destroy and create again (a cache hit), two host threads on two contexts, and a handle
   whose compile failed.

Every compilation goes to a kernel cache in a temporary directory: the shipped cache is a build product."""
import functools
import os
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_fuzz as cf  # noqa: E402
import ctl_instances as ci  # noqa: E402
import ctl_ref as cr  # noqa: E402
import representatives as rep  # noqa: E402
import stark_fuzz as sf  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
import test_ctl_fuzz as tcf  # noqa: E402  (cf.coverage is pinned there)
import test_gpu_ctl as tgc  # noqa: E402  (_check_ctl_quotient, _reference: the reference proofs, proved once)
import test_gpu_stark as tgs  # noqa: E402  (_reference_proof, _trace: the reference proofs, proved once)
import test_gpu_stark_fuzz as tgsf  # noqa: E402  (_desc)
from gpu_util import gpu, kernel_cache  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = sr.P


def _objects(cache):
    return sorted(f for f in os.listdir(cache) if f.startswith("stark_") and f.endswith(".hsaco"))


def _compiled_stark(gpu, desc, hasher="poseidon"):
    import plonky2_gpu_amd as pg

    ns = pg.NativeStark(gpu, desc, hasher)
    assert not ns.is_compiled and ns.kernel_source is None
    ns.close()
    ns = pg.NativeStark(gpu, desc, hasher, compiled=True)
    assert ns.is_compiled and "stark_quotient_kernel" in ns.kernel_source
    return ns


# ---------------------------------------------------------------- 1. every description of stark_fuzz.CASES
def _check_fuzz_case(gpu, i, lifted=False):
    case = sf.fuzz_case(i)
    s = case["stark"]
    trace, zs, sets, alphas, pis = sf.fuzz_inputs(i, case)
    exp = sf.reference_quotient(case, trace, zs, sets, alphas, pis)
    shape = dict(seed=sf.SEED + i, columns=s.num_columns, public_inputs=s.num_public_inputs, constraint_degree=s.constraint_degree,
                 challenges=case["num_challenges"], degree_bits=case["degree_bits"], rate_bits=case["rate_bits"], instructions=len(s.instrs),
                 pairs=s.pairs, lifted=lifted)
    if lifted:  # every word that has a second representative word + p is that one
        rng = np.random.default_rng(i)
        trace, count = rep.lift(trace, rng, frac=1.0)
        if zs is not None:
            zs, more = rep.lift(zs, rng, frac=1.0)
            count += more
            sets = [[(rep.lift_scalar(b), rep.lift_scalar(g)) for b, g in one] for one in sets]
        alphas, pis = [rep.lift_scalar(a) for a in alphas], [rep.lift_scalar(x) for x in pis]
        shape["lifted"] = count
    t0 = time.perf_counter()
    ns = _compiled_stark(gpu, tgsf._desc(case))
    print("compile of %d instructions (and an interpreted handle): %.1f s" % (len(s.instrs), time.perf_counter() - t0))
    try:
        n_ext = trace.shape[1]
        for stride in (n_ext, n_ext + 6):
            t = Strided(gpu, trace, stride)
            z = Strided(gpu, zs, stride) if zs is not None else None
            got = ns.quotient_polys(t.ptr, z.ptr if z else None, stride, alphas, sets, pis)
            assert (t.polys() == trace).all() and (z is None or (z.polys() == zs).all())  # guards and pads: only read
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("column pitch", stride, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad), shape)
            t.free()
            if z:
                z.free()
    finally:
        ns.close()


LONG = [i for i in sf.CASES if sf.LENGTHS[i] >= 1000]


@pytest.mark.gpu
@pytest.mark.parametrize("i", [i for i in sf.CASES if i not in LONG])
def test_compiled_quotient_of_a_random_program_on_random_words(gpu, i):
    _check_fuzz_case(gpu, i)


@pytest.mark.gpu
def test_compiled_quotient_of_the_4000_instruction_program(gpu):
    """the one slow test: hiprtc takes 22 s on the GPU host (80 s on an eight-core build container) for 4 000 instructions under
    four challenges — its instruction selection over one long basic block"""
    assert LONG == [11] and sf.LENGTHS[11] == 4000
    _check_fuzz_case(gpu, 11)


# ---------------------------------------------------------------- 2. non-canonical words
LIFTED = [0, 5, 7]


def test_the_lifted_descriptions_have_1_2_and_4_challenges_and_one_has_pairs():
    cases = [sf.fuzz_case(i) for i in LIFTED]
    assert sorted(c["num_challenges"] for c in cases) == [1, 2, 4]
    assert any(any(pair for pair in c["stark"].pairs) for c in cases)
    assert all(sf.LENGTHS[i] <= 400 for i in LIFTED)


@pytest.mark.gpu
@pytest.mark.parametrize("i", LIFTED)
def test_compiled_quotient_on_non_canonical_words(gpu, i):
    _check_fuzz_case(gpu, i, lifted=True)


# ---------------------------------------------------------------- 3. whole proofs
# the hand-written STARKs where tests/test_gpu_stark.py proves them, under both hashers where it uses both; one D(d) with qdf 16 and
# 4 challenges; a trace of two rows
PROOFS = [p for p in tgs.PROOFS if (p[0] in ("A", "B", "C") and p[1] == 3)] + [("D17", 3, 4, 4, 0, (1, 2), "poseidon"), ("A", 1, 2, 1, 0, (), "poseidon")]


def test_the_proved_starks_are_the_hand_written_ones_under_both_hashers():
    assert {p[0] for p in PROOFS} == {"A", "B", "C", "D17"} and all(p in tgs.PROOFS for p in PROOFS)
    assert {(p[0], p[6]) for p in PROOFS} >= {("A", "poseidon"), ("B", "poseidon"), ("B", "keccak"), ("C", "poseidon"), ("C", "keccak")}
    assert sr.quotient_degree_factor(si.STARKS["D17"]) == 16 and ("D17", 3, 4, 4, 0, (1, 2), "poseidon") in PROOFS and ("A", 1, 2, 1, 0, (), "poseidon") in PROOFS


@pytest.mark.gpu
@pytest.mark.parametrize("name,degree_bits,num_challenges,rate_bits,cap_height,arity_bits,hasher", PROOFS)
def test_compiled_proof_bytes_equal_the_interpreted_and_the_reference(gpu, name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher):
    import plonky2_gpu_amd as pg

    stark = si.STARKS[name]
    fp = si.fri_params(rate_bits=rate_bits, cap_height=cap_height, arity_bits=arity_bits)
    trace, pis = tgs._trace(name, degree_bits)
    exp = tgs._reference_proof(name, degree_bits, num_challenges, rate_bits, cap_height, arity_bits, hasher)
    desc = stark.desc(degree_bits, num_challenges, fp)
    interpreted = pg.NativeStark(gpu, desc, hasher)
    compiled = _compiled_stark(gpu, desc, hasher)
    try:
        assert not interpreted.is_compiled
        assert interpreted.prove_bytes(trace, pis) == exp
        assert compiled.prove_bytes(trace, pis) == exp
    finally:
        interpreted.close()
        compiled.close()


# ---------------------------------------------------------------- 4. tables
SYSTEMS = [0, 1, 2, 4, 5, 11, 13]


def test_the_systems_reach_what_the_ctl_generator_can_get_wrong():
    """from Case.filters, Case.general and ctl_fuzz.coverage(): a changed generator of systems fails here, on the CPU"""
    cases = {i: cf.fuzz_system(i) for i in SYSTEMS}
    cov = cf.coverage()
    among = lambda key: sorted(set(cov[key]) & set(SYSTEMS))  # noqa: E731
    assert {c.hasher for c in cases.values()} == {"poseidon", "keccak"}
    assert {c.num_challenges for c in cases.values()} == {1, 2, 3, 4}
    assert all(2 <= len(c.system.tables) <= 3 for c in cases.values()) and sum(len(c.system.tables) for c in cases.values()) == 17
    assert among("self_lookup") and among("repeated_looking") and among("mixed_roles")  # both sides of a lookup; twice on one side
    assert 4 in among("pair_two_ctl_zs_qdf_3")
    assert 2 in among("qdf_4_rate_bits_2")
    assert 11 in among("two_rows_beside_2_11")
    assert among("filter_selects_no_row") and among("filter_selects_every_row")
    assert 13 in among("unfiltered_with_default") and 13 in among("unfiltered_without_default")
    filters = [v for c in cases.values() for v in c.filters.values()]
    assert any(count == 0 for _, count, n in filters) and any(count == n for _, count, n in filters)
    assert {kind for kind, _, _ in filters} == {"single", "not", "sum"}
    assert {g for c in cases.values() for g in c.general} == {"looked", "looking"}
    assert "default" in cases[13].kinds and "plain" in cases[13].kinds and not cases[13].filters


def _compiled_tables(gpu, desc, hasher):
    import plonky2_gpu_amd as pg

    nt = pg.NativeStarkTables(gpu, desc, hasher)
    assert not nt.is_compiled and nt.kernel_source is None
    nt.compile()
    sources = nt.kernel_source
    assert nt.is_compiled and len(sources) == len(desc.tables) and all("stark_quotient_kernel" in s and "p.ctl_beta" in s for s in sources)
    return nt


@pytest.mark.gpu
@pytest.mark.parametrize("i", SYSTEMS)
def test_compiled_tables_of_a_random_system(gpu, i):
    """every table's quotient on any u64 (as tests/test_gpu_ctl_fuzz.py), then the compiled proof against the interpreted one and
    the reference's bytes"""
    import plonky2_gpu_amd as pg

    case = cf.fuzz_system(i)
    rate_bits = case.fri_params[0]["rate_bits"]
    assert all(db + rate_bits <= 13 for db in case.degree_bits)  # the quotient's reference is Python
    desc = case.desc()
    interpreted = pg.NativeStarkTables(gpu, desc, case.hasher)
    compiled = _compiled_tables(gpu, desc, case.hasher)
    try:
        for k in range(len(desc.tables)):
            tgc._check_ctl_quotient(gpu, case.system, desc, k, case.degree_bits[k], rate_bits, case.num_challenges, 1000 * i + k, words=tgc._any_words,
                                    nt=compiled)
        exp = interpreted.prove_bytes(case.traces)
        assert not interpreted.is_compiled and compiled.prove_bytes(case.traces) == exp
        _, proofs = tcf.reference(i)
        assert exp == cr.proofs_bytes(tgc.HASHERS[case.hasher], proofs)
    finally:
        interpreted.close()
        compiled.close()


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 2])
def test_compiled_tables_of_the_hand_written_system(gpu, i):
    """tests/ctl_instances.py under Poseidon with 2 challenges and under Keccak with 2 challenges at degree 4"""
    import plonky2_gpu_amd as pg

    system, nch, fp, hasher, exp = tgc._reference(i)
    name, rate_bits = tgc.tcr.CASES[i][0], tgc.tcr.CASES[i][3]
    desc = system.desc(ci.DEGREE_BITS, nch, fp)
    traces = ci.make_traces(i)
    interpreted = pg.NativeStarkTables(gpu, desc, name)
    compiled = _compiled_tables(gpu, desc, name)
    try:
        for k in range(3):
            tgc._check_ctl_quotient(gpu, system, desc, k, ci.DEGREE_BITS[k], rate_bits, nch, 50 * i + k, words=tgc._any_words, nt=compiled)
        assert interpreted.prove_bytes(traces) == exp
        assert compiled.prove_bytes(traces) == exp
    finally:
        interpreted.close()
        compiled.close()


# ---------------------------------------------------------------- 5. life cycle
LIFE = ("B", 8, 2, dict(rate_bits=2, cap_height=1, arity_bits=(2, 2)))


@functools.lru_cache(maxsize=None)
def _life_traces():
    return [si.B.make_trace(8, seed=s) for s in (1, 2)]


@pytest.mark.gpu
def test_compile_twice_trim_and_a_cache_hit(gpu, kernel_cache):
    import plonky2_gpu_amd as pg

    desc = si.B.desc(LIFE[1], LIFE[2], si.fri_params(**LIFE[3]))
    trace, pis = _life_traces()[0]
    interpreted = pg.NativeStark(gpu, desc)
    exp = interpreted.prove_bytes(trace, pis)
    interpreted.close()
    ns = pg.NativeStark(gpu, desc)
    ns.compile()
    objects = _objects(kernel_cache)
    stamps = [os.stat(os.path.join(kernel_cache, f)).st_mtime_ns for f in objects]
    source = ns.kernel_source
    ns.compile()  # a no-op
    assert ns.is_compiled and ns.kernel_source == source
    assert ns.prove_bytes(trace, pis) == exp
    ns.trim()
    assert ns.prove_bytes(trace, pis) == exp
    ns.close()
    again = pg.NativeStark(gpu, desc, compiled=True)  # the same description: its kernel comes out of the cache
    try:
        assert again.kernel_source == source
        assert _objects(kernel_cache) == objects and [os.stat(os.path.join(kernel_cache, f)).st_mtime_ns for f in objects] == stamps
        assert again.prove_bytes(trace, pis) == exp
    finally:
        again.close()


@pytest.mark.gpu
def test_one_compiled_handle_on_two_contexts_from_two_threads(gpu):
    import plonky2_gpu_amd as pg

    desc = si.B.desc(LIFE[1], LIFE[2], si.fri_params(**LIFE[3]))
    traces = _life_traces()
    ns = pg.NativeStark(gpu, desc, compiled=True)
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


@pytest.mark.gpu
def test_a_handle_whose_compile_failed_proves_interpreted(gpu, tmp_path):
    """the cache holds a code object cut short under the kernel's own name: the library refuses to load it, says which file it was,
    and the handle stays interpreted and usable; no kernel is launched from the damaged file"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import stark as pstark

    desc = si.C.desc(3, 2, si.fri_params(rate_bits=2, arity_bits=(1, 2)))
    trace, pis = tgs._trace("C", 3)
    exp = tgs._reference_proof("C", 3, 2, 2, 0, (1, 2), "poseidon")
    saved = os.environ["PLONKY2_HIP_KERNEL_CACHE"]
    os.environ["PLONKY2_HIP_KERNEL_CACHE"] = str(tmp_path)
    try:
        pstark.precompile(desc)
        (name,) = _objects(str(tmp_path))
        path = os.path.join(str(tmp_path), name)
        whole = open(path, "rb").read()
        with open(path, "wb") as f:
            f.write(whole[: len(whole) // 2])
        ns = pg.NativeStark(gpu, desc)
        try:
            with pytest.raises(pg.Plonky2HipError) as e:
                ns.compile()
            assert e.value.code == pg.GL_E_INVALID and name in str(e.value)
            assert not ns.is_compiled and ns.kernel_source is None
            assert ns.prove_bytes(trace, pis) == exp
            with open(path, "wb") as f:
                f.write(whole)
            ns.compile()  # and with the whole file it compiles
            assert ns.is_compiled and ns.prove_bytes(trace, pis) == exp
        finally:
            ns.close()
    finally:
        os.environ["PLONKY2_HIP_KERNEL_CACHE"] = saved
