"""tests/stark_fuzz.py pinned on the CPU: every generated program is valid, the fixed list of descriptions the device test runs
(stark_fuzz.CASES) reaches what the generator exists for — a CONDITION on the generator and its seeds, asserted here, not a
measurement — and the interpreter of tests/stark_ref.py runs the programs alike over the base field and over the extension."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stark_fuzz as sf  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402

P = sr.P


def _cases():
    return [sf.fuzz_case(i) for i in sf.CASES]


def test_every_generated_program_is_valid():
    for i, case in enumerate(_cases()):
        s = case["stark"]
        assert s.instrs.shape == (sf.LENGTHS[i], 4) and s.instrs.dtype == np.uint16
        sr.validate_program(s.instrs, s.immediates, s.num_columns, s.num_public_inputs)
        assert int(s.instrs[-1, 0]) in sf.EMITS
    rng = np.random.default_rng(1)
    for length in (2, 3, 5, 8, 17, 60):  # other shapes than the fixed list's
        for cols, pis in ((1, 0), (2, 1), (70, 3)):
            instrs, imms = sf.gen_program(rng, cols, pis, length)
            assert len(instrs) == length
            sr.validate_program(instrs, imms, cols, pis)


def test_the_generator_is_deterministic():
    a, b = sf.fuzz_case(5), sf.fuzz_case(5)
    assert (a["stark"].instrs == b["stark"].instrs).all() and a["stark"].immediates == b["stark"].immediates
    assert a["stark"].pairs == b["stark"].pairs and a["degree_bits"] == b["degree_bits"]


def test_the_fixed_list_reaches_what_the_generator_is_for():
    cases = _cases()
    cov = [sf.coverage(c["stark"].instrs, c["stark"].immediates) for c in cases]
    count = lambda f: sum(1 for c in cov if f(c))  # noqa: E731
    for op in set(range(15)) - {sr.LOAD_CONST}:
        assert 2 * count(lambda c: op in c["ops"]) >= len(cases), ("opcode in fewer than half of the programs", op)
    assert count(lambda c: c["dst63"]) >= 3
    for q in range(4):
        assert count(lambda c: q in c["accs"]) >= 3, q
    assert count(lambda c: 0 in c["shifts"]) >= 3 and count(lambda c: 63 in c["shifts"]) >= 3 and count(lambda c: 32 in c["shifts"]) >= 3
    assert count(lambda c: c["high_bound"]) >= 3
    assert count(lambda c: c["own_source"]) >= 3
    # immediates: p - 1, 2^32 and 2^32 - 1 are loaded somewhere, and the largest single ACC weight is used
    loaded = {c["stark"].immediates[int(r[2])] for c in cases for r in c["stark"].instrs if int(r[0]) == sr.LOAD_IMM}
    assert {P - 1, 1 << 32, (1 << 32) - 1} <= loaded and any(v not in sf.IMMEDIATES for v in loaded)
    weights = {c["stark"].immediates[int(r[3])] for c in cases for r in c["stark"].instrs if int(r[0]) == sr.ACC}
    assert weights == set(sf.ACC_WEIGHTS) - {(1 << 32) - 1}  # (2^32 - 1)^2 > 2^63: never taken
    # the shapes
    shape = lambda f: {f(c) for c in cases}  # noqa: E731
    assert shape(lambda c: c["stark"].num_columns) == {1, 5, 70} and shape(lambda c: c["stark"].num_public_inputs) == {0, 1, 3}
    assert shape(lambda c: c["num_challenges"]) == {1, 2, 3, 4} and shape(lambda c: c["degree_bits"]) == {1, 2, 3, 4}
    assert shape(lambda c: sr.quotient_degree_factor(c["stark"])) == set(sf.QDFS)
    assert shape(lambda c: c["stark"].constraint_degree) >= {1, 2, 17}
    assert any(sr.quotient_degree_factor(c["stark"]) == 16 and c["num_challenges"] == 4 and c["stark"].pairs for c in cases)
    steps = shape(lambda c: c["rate_bits"] - (sr.quotient_degree_factor(c["stark"]) - 1).bit_length())
    assert steps >= {0, 1}  # the quotient domain is the LDE's, or every second point of it
    assert all(c["rate_bits"] >= 1 for c in cases)
    assert shape(lambda c: len(c["stark"].pairs)) == {0, 1, 2, 3}
    assert sum(1 for c in cases if any(len(pair) == 0 for pair in c["stark"].pairs)) >= 2  # a pair with no column pairs
    assert sorted(set(sf.LENGTHS)) == [8, 60, 400, 4000] and sf.LENGTHS.count(4000) == 1
    # a single short batch: fewer instances than the batch size
    assert any(0 < len(c["stark"].pairs) * c["num_challenges"] < sr.quotient_degree_factor(c["stark"]) for c in cases)


@pytest.mark.parametrize("i", [0, 1, 4, 9])
def test_base_and_extension_interpreters_agree_on_generated_programs(i):
    """the base field embeds in the extension: on rows (x, 0) the interpreter over Ext gives (the interpreter over Base, 0),
    constraint by constraint and in the accumulators"""
    s = sf.fuzz_case(i)["stark"]
    rng = np.random.default_rng(50 + i)
    rand = lambda k: [int(x) for x in rng.integers(0, P, size=k, dtype=np.uint64)]  # noqa: E731
    for _ in range(3):
        local, nxt, pis, alphas = rand(s.num_columns), rand(s.num_columns), rand(s.num_public_inputs), rand(3)
        z_last, l_first, l_last = rand(3)
        base = sr.Consumer(sr.Base, alphas, z_last, l_first, l_last)
        ext = sr.Consumer(sr.Ext, alphas, (z_last, 0), (l_first, 0), (l_last, 0))
        emb = lambda v: [(x, 0) for x in v]  # noqa: E731
        sr.run_program(sr.Base, s.instrs, s.immediates, local, nxt, pis, base)
        sr.run_program(sr.Ext, s.instrs, s.immediates, emb(local), emb(nxt), emb(pis), ext)
        assert [tuple(e) for e in ext.emitted] == [(b, 0) for b in base.emitted] and len(base.emitted) >= 1
        assert [tuple(a) for a in ext.accs] == [(a, 0) for a in base.accs]
        assert any(b != 0 for b in base.emitted)


def test_the_batch_inversion_zs_equal_the_reference_zs():
    """2^13 rows of B with 3 challenges (5 Zs, batches of 2 and 1) and of A"""
    for stark, nch in ((si.B, 3), (si.A, 1)):
        trace, _ = stark.make_trace(13, seed=13)
        rng = np.random.default_rng(13)
        sets = [[(int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64))) for _ in range(nch)]
                for _ in range(sr.quotient_degree_factor(stark))]
        assert sf.fast_permutation_z_polys(stark, nch, trace, sets) == sr.compute_permutation_z_polys(stark, nch, trace, sets)
