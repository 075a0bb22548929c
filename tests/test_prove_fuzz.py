"""tests/fuzz_prove.py and tests/fuzz_prove_c.py pinned on the CPU: the fixed lists of cases that tests/test_gpu_prove_fuzz.py runs
on the device reach what the campaigns exist for — a CONDITION on the generators and their seeds, asserted here and computed from
the lists, not a measurement. A change of a generator or of a seed that loses one of these fails here; the remedy is a longer list
or another seed, never a dropped assertion."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_prove as fp  # noqa: E402
import fuzz_prove_c as fpc  # noqa: E402


def _python_cases():
    return [fp.fuzz_case(i) for i in range(len(fp.CASES))]


def _c_cases():
    return [fpc.fuzz_case(i) for i in range(len(fpc.CASES))]


def _fri_shapes():
    """(degree_bits, rate_bits, cap_height, arity_bits, pow_bits, num_queries) of every case of both lists"""
    out = [(c["shape"]["degree_bits"], c["shape"]["rate_bits"], c["shape"]["cap_height"], c["shape"]["arity_bits"], c["shape"]["pow_bits"],
            c["shape"]["num_queries"]) for c in _python_cases()]
    out += [(c["degree_bits"], fpc.RATE_BITS, c["kw"]["cap_height"], c["kw"]["arity_bits"], c["kw"]["pow_bits"], c["kw"]["num_queries"])
            for c in _c_cases()]
    return out


def test_the_lists_are_deterministic_and_a_prefix_of_their_campaigns():
    assert _python_cases() == _python_cases() and _c_cases() == _c_cases()
    assert fp.cases(40, fp.SEED)[: len(fp.CASES)] == _python_cases()
    assert fpc.cases(40, fpc.SEED, fpc.MAX_DEGREE_BITS)[: len(fpc.CASES)] == _c_cases()
    assert [c["index"] for c in _python_cases()] == fp.CASES and [c["index"] for c in _c_cases()] == fpc.CASES
    assert 20 <= len(fp.CASES) + len(fpc.CASES) <= 28  # about 24 proofs: the suite runs them for every later change


def test_the_sizes_stay_within_what_the_references_prove_in_seconds():
    assert max(c["shape"]["degree_bits"] for c in _python_cases()) <= 6   # the Python prover
    assert max(c["degree_bits"] for c in _c_cases()) <= fpc.MAX_DEGREE_BITS == 10  # the C prover
    assert max(c["degree_bits"] for c in fpc.cases(200, 1)) == 12  # the command line still goes further


def test_the_circuits_the_lists_reach():
    py, c = _python_cases(), _c_cases()
    assert {k["family"] for k in c} == {"mini", "full", "recursion"}
    groups = {k["shape"]["two_groups"] for k in py} | {k["kw"]["two_groups"] for k in c if k["family"] == "mini"}
    assert groups == {False, True}
    assert {k["shape"]["two_groups"] for k in py} == {False, True}  # and both against the Python prover alone
    challenges = {k["shape"]["num_challenges"] for k in py} | {k["kw"]["num_challenges"] for k in c if k["family"] == "mini"}
    assert challenges == {1, 2, 3} == {k["shape"]["num_challenges"] for k in py}  # and all three against the Python prover alone
    qdfs = {k["shape"]["quotient_degree_factor"] for k in py}
    assert any(q & (q - 1) for q in qdfs), qdfs  # a quotient degree factor that is not a power of two
    assert all(q <= 1 << k["shape"]["rate_bits"] for k in py for q in [k["shape"]["quotient_degree_factor"]])  # prover.rs:807-811
    # the rates a proof of these circuits can have: their constraints need a quotient degree factor of at least 4 (two selector
    # groups) or 5 (one), and it must not exceed 2^rate_bits, so a rate of 1 bit is out of a plonk proof's reach. random_shape draws
    # it all the same and falls back to 3; rate bits 0 and 1 are reached one level below, by the commits of tests/fuzz_commit.py
    # (tests/test_commit_fuzz.py asserts that)
    assert {k["shape"]["rate_bits"] for k in py} == {2, 3}
    assert all(k["shape"]["two_groups"] for k in py if k["shape"]["rate_bits"] == 2)
    # compiled and interpreted gates, against either prover and for every family
    assert min(sum(1 for k in py if k["compile_gates"] == flag) for flag in (False, True)) >= 3
    for family in ("mini", "full", "recursion"):
        assert {k["compile_gates"] for k in c if k["family"] == family} == {False, True}, family
    # blinding: some case draws its salts from all of u64, some from the field, most proofs are not blinded
    assert any(k["blinded"] and k["raw_salts"] for k in c) and any(k["blinded"] and not k["raw_salts"] for k in c)
    assert not any(k["raw_salts"] and not k["blinded"] for k in c) and sum(1 for k in c if not k["blinded"]) >= len(c) // 2
    assert min(k["degree_bits"] for k in c) <= 4 and max(k["degree_bits"] for k in c) >= 9  # both ends of the C prover's sizes


def test_the_fri_shapes_the_lists_reach():
    shapes = _fri_shapes()
    assert {s[2] for s in shapes} == {0, 1, 2, 3, 4}  # cap heights
    # every layer of every shape is at least as large as the cap (reduction_strategies.rs:38-48) ...
    for degree_bits, rate_bits, cap_height, arity, _, _ in shapes:
        bits = degree_bits + rate_bits
        for ab in arity:
            bits -= ab
            assert bits >= cap_height, (degree_bits, rate_bits, cap_height, arity)
    # ... and somewhere the cap IS the whole last layer: its tree has no digests below the cap
    assert any(arity and degree_bits + rate_bits - sum(arity) == cap_height for degree_bits, rate_bits, cap_height, arity, _, _ in shapes)
    assert any(arity == () for _, _, _, arity, _, _ in shapes)  # no reduction at all
    assert {ab for _, _, _, arity, _, _ in shapes for ab in arity} == {1, 2, 3, 4}
    assert any(len(arity) >= 3 for _, _, _, arity, _, _ in shapes)
    assert {s[4] for s in shapes} >= {0, 9}   # proof-of-work bits: none, and the most the campaigns draw
    assert {s[5] for s in shapes} >= {1, 28}  # query rounds
