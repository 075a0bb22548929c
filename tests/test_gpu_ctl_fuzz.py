"""gl_stark_tables_create / gl_stark_tables_prove, gl_stark_tables_ctl_zs and gl_stark_tables_quotient_polys on the random multi-table
systems of tests/ctl_fuzz.py against tests/ctl_ref.py, bit for bit: there is no tolerance anywhere. What the list of systems reaches
— 2 to 17 tables (the trace caps are observed in steps of eight), 1 to 4 challenges, 2 to 2^12 rows in one proof, a table on both
sides of one lookup, Zs oracles of 1 to 36 polynomials, filters that select no row or every row — is asserted on the CPU
(tests/test_ctl_fuzz.py). Here also: words >= p in the traces, the challenges, the LDEs and the description's coefficients."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctl_fuzz as cf  # noqa: E402
import ctl_ref as cr  # noqa: E402
import representatives as rep  # noqa: E402
import test_ctl_fuzz as tcf  # noqa: E402  (reference: the reference proofs, proved once)
import test_gpu_ctl as tgc  # noqa: E402  (_check_ctl_quotient, _any_words)
from gpu_util import gpu  # noqa: E402,F401
from test_ctl_ref import HASHERS  # noqa: E402

P = cf.P
ALL = range(len(cf.CASES))
MAX_POINTS_BITS = 13  # the quotient's reference is Python: at most 2^13 points of the LDE per call


@functools.lru_cache(maxsize=None)
def _reference_bytes(i):
    case, proofs = tcf.reference(i)
    return case, cr.proofs_bytes(HASHERS[case.hasher], proofs)


# ---------------------------------------------------------------- a. whole proofs
@pytest.mark.gpu
@pytest.mark.parametrize("i", ALL)
def test_proof_bytes_equal_the_reference_and_verify(gpu, i):
    """the second proof runs on the recycled pools, the third after trim()"""
    import plonky2_gpu_amd as pg
    from oracle import accel
    from plonky2_gpu_amd import stark as pstark

    case, exp = _reference_bytes(i)
    desc = case.desc()
    nt = pg.NativeStarkTables(gpu, desc, case.hasher)
    try:
        data = nt.prove_bytes(case.traces)
        assert data == exp
        assert nt.prove_bytes(case.traces) == exp
        nt.trim()
        assert nt.prove_bytes(case.traces) == exp
    finally:
        nt.close()
    parsed = pstark.tables_proof_from_bytes(data, desc, case.hasher)
    assert pstark.tables_proof_to_bytes(parsed, desc, case.hasher) == data
    with accel.c_backend():
        assert cr.verify_tables(HASHERS[case.hasher], case.system, case.num_challenges, case.fri_params, parsed)


# ---------------------------------------------------------------- b. the CTL Zs
@pytest.mark.gpu
@pytest.mark.parametrize("i", ALL)
def test_ctl_zs_of_every_table_equal_the_reference(gpu, i):
    """the canonical trace and the trace in which every word that has a second representative word + p is that one (the flags, the
    counters, the small words of the free columns); the challenges as c + p where that fits; tight and padded pitch"""
    import plonky2_gpu_amd as pg

    case = cf.fuzz_system(i)
    nch = case.num_challenges
    rng = np.random.default_rng(600 + i)
    canonical = [(int(b), int(g)) for b, g in rep.field_data(rng, (nch, 2))]
    challenges = [(rep.lift_scalar(b), rep.lift_scalar(g)) for b, g in canonical]
    assert any(w >= P for bg in challenges for w in bg) or nch == 1
    nt = pg.NativeStarkTables(gpu, case.desc(), case.hasher)
    try:
        lifted_words = 0
        for k, trace in enumerate(case.traces):
            n = 1 << case.degree_bits[k]
            assert n <= 1 << 12
            exp = np.array(cr.ctl_z_polys(case.system.lookups, nch, k, trace, canonical), dtype=np.uint64)
            assert exp.shape == (case.desc().num_ctl_zs(k), n)
            lifted, count = rep.lift(trace, rng, frac=1.0)
            lifted_words += count
            for name, words in (("canonical", np.array(trace, dtype=np.uint64)), ("lifted", lifted)):
                for stride in (n, n + 6):
                    got = nt.ctl_zs(k, words, challenges, trace_stride=stride)
                    bad = np.argwhere(got != exp)
                    assert bad.size == 0, ("table", k, name, "trace pitch", stride, "first (Z, row) that differs", bad[0].tolist(), len(bad))
        assert lifted_words >= sum(1 << db for db in case.degree_bits)  # at least every counter
    finally:
        nt.close()


# ---------------------------------------------------------------- c. the quotient on any u64
@pytest.mark.gpu
@pytest.mark.parametrize("i", ALL)
def test_ctl_quotient_of_every_table_on_any_u64(gpu, i):
    """uniform 64-bit words, one in eight of them moved to [p, 2^64), for both LDEs, the alphas, the permutation and the CTL
    challenges (the reference gets all of them reduced); a table whose LDE has more than 2^13
    points is described again with fewer rows (the same program, pairs and lookups: the quotient needs nothing to hold)"""
    import plonky2_gpu_amd as pg

    case = cf.fuzz_system(i)
    rate_bits = case.fri_params[0]["rate_bits"]
    degree_bits = [min(db, MAX_POINTS_BITS - rate_bits) for db in case.degree_bits]
    desc = case.desc(degree_bits)
    for t, db in zip(desc.tables, case.degree_bits):
        if t.degree_bits != db:
            t.fri_params["reduction_arity_bits"] = []
    desc.validate(case.hasher)
    nt = pg.NativeStarkTables(gpu, desc, case.hasher)
    try:
        for k in range(len(desc.tables)):
            tgc._check_ctl_quotient(gpu, case.system, desc, k, degree_bits[k], rate_bits, case.num_challenges, 1000 * i + k, words=tgc._any_words, nt=nt)
    finally:
        nt.close()


def test_the_words_of_the_quotient_test_reach_beyond_p():
    """no GPU: what test_gpu_ctl._any_words draws"""
    w = tgc._any_words(np.random.default_rng(0), 3, 1 << 12)
    assert w.dtype == np.uint64 and w.shape == (3, 1 << 12) and 0.08 < float((w >= np.uint64(P)).mean()) < 0.17 and int(w.min()) < 1 << 54
    assert [int(x) for x in np.array([P, P + 5, (1 << 64) - 1], dtype=np.uint64) % np.uint64(P)] == [0, 5, (1 << 32) - 2]


# ---------------------------------------------------------------- d. a description of non-canonical words
@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 1])
def test_a_description_of_non_canonical_words_proves_the_same_bytes(gpu, i):
    """every coefficient and constant w < 2^64 - p of the flattened description as w + p (lifted behind flatten(): the library must
    reduce them, not the Python layer); one case per hasher"""
    import plonky2_gpu_amd as pg

    case, exp = _reference_bytes(i)
    assert case.hasher == ("poseidon", "keccak")[i]
    desc = case.desc()
    flat = desc.flatten()
    lifted = 0
    for key in ("term_coeffs", "column_constants"):
        small = flat[key] < np.uint64(rep.LIFTABLE)
        flat[key][small] += np.uint64(P)
        lifted += int(small.sum())
        assert flat[key].dtype == np.uint64 and (flat[key][small] >= np.uint64(P)).all()
    assert lifted >= 10 and int(flat["term_coeffs"].min()) > 1  # every coefficient 1 (the single columns, the filters) among them
    nt = pg.NativeStarkTables(gpu, desc, case.hasher, flat=flat)
    try:
        assert nt.prove_bytes(case.traces) == exp
    finally:
        nt.close()


# ---------------------------------------------------------------- e. a non-binary filter in the ninth table
@pytest.mark.gpu
def test_a_non_binary_filter_in_the_ninth_table_is_refused_by_prove(gpu):
    """table 8 is proved in the second step of the trace caps' observation; its CTL Zs are the last the flag is raised by"""
    import copy

    import plonky2_gpu_amd as pg

    i = [k for k, spec in enumerate(cf.CASES) if spec.get("chain") == 9][0]
    case, exp = _reference_bytes(i)
    assert len(case.traces) == 9
    flags = [c for lk in case.system.lookups for t in lk.twcs if t.table == 8 and t.filter_column is not None for c, _ in t.filter_column.terms]
    assert flags, "table 8 has no filter"
    traces = copy.deepcopy(case.traces)
    assert traces[8][flags[0]][1] in (0, 1)
    traces[8][flags[0]][1] = 2
    nt = pg.NativeStarkTables(gpu, case.desc(), case.hasher)
    try:
        with pytest.raises(pg.Plonky2HipError, match="Non-binary filter") as e:
            nt.prove_bytes(traces)
        assert e.value.code == pg._lib.GL_E_INVALID
        assert nt.prove_bytes(case.traces) == exp  # the handle works on
    finally:
        nt.close()
