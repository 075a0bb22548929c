"""tests/fuzz_commit.py pinned on the CPU: the fixed list of cases that tests/test_gpu_commit_fuzz.py runs on the device reaches
what the campaign exists for — a CONDITION on the generator and its seed, asserted here and computed from the list, not a
measurement. A change that loses one of these fails here; the remedy is a longer list or another seed, never a dropped assertion."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_commit as fc  # noqa: E402


def _cases():
    return [fc.fuzz_case(i) for i in range(len(fc.CASES))]


def test_the_list_is_deterministic_and_a_prefix_of_its_campaign():
    assert _cases() == _cases() and fc.cases(60, fc.SEED)[: len(fc.CASES)] == _cases()
    assert [c["index"] for c in _cases()] == fc.CASES and 24 <= len(fc.CASES) <= 36  # about 30
    a, b = fc.values(fc.fuzz_case(4)), fc.values(fc.fuzz_case(4))
    assert (a == b).all() and a.dtype == np.uint64
    assert len({fc.values(c).tobytes() for c in _cases() if c["log_n"] >= 2}) == sum(1 for c in _cases() if c["log_n"] >= 2)


def test_the_list_stays_in_the_small_branch():
    assert max(c["log_n"] for c in _cases()) <= 13
    assert min(c["log_n"] for c in fc.cases(10, fc.SEED, large=True)) >= 13  # the large branch stays a command-line option


def test_what_the_list_reaches():
    cases = _cases()
    polys = {c["n_polys"] for c in cases}
    # leaves of at most 4 elements are not hashed (hash_or_noop), 8 elements fill one sponge block
    assert min(polys) < 4 < max(polys) and any(p <= 4 for p in polys) and any(4 < p < 8 for p in polys) and any(p > 8 for p in polys)
    assert {4, 8} & polys and any(p >= 17 for p in polys)  # a boundary itself, and leaves of several blocks
    logs = {c["log_n"] for c in cases}
    assert {0, 1} <= logs and max(logs) >= 12
    assert {c["rate_bits"] for c in cases} == {0, 1, 2, 3}
    assert any(c["log_n"] == 0 and c["rate_bits"] == 0 for c in cases) or any(c["log_n"] + c["rate_bits"] <= 1 for c in cases)  # a tree of one or two leaves
    for c in cases:
        assert 0 <= c["cap_height"] <= c["log_n"] + c["rate_bits"]
        assert all(0 <= i < 1 << (c["log_n"] + c["rate_bits"]) for i in c["opened"]) and len(c["opened"]) == 3
    assert any(c["cap_height"] == c["log_n"] + c["rate_bits"] and c["cap_height"] > 0 for c in cases)  # the cap is the leaf layer: no digests
    assert any(c["cap_height"] == 0 and c["log_n"] + c["rate_bits"] > 0 for c in cases)                # the cap is the root
    assert any(0 < c["cap_height"] < c["log_n"] + c["rate_bits"] for c in cases)
    for flag in ("non_canonical", "from_values", "leaf_major"):
        assert {c[flag] for c in cases} == {False, True}, flag
    # the flags in combination: a non-canonical case really holds words >= p; both constructors with and without the leaf-major copy
    assert any(c["non_canonical"] and (fc.values(c) >= np.uint64(fc.P)).any() for c in cases)
    assert all((fc.values(c) < np.uint64(fc.P)).all() for c in cases if not c["non_canonical"])
    assert {(c["from_values"], c["leaf_major"]) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
