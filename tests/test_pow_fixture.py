"""tests/golden/pow_witnesses.json re-checked on the CPU, and the C search (oracle/gl_oracle.c glo_pow_search) held against the
Python model. The rows are smallest proof-of-work witnesses that the device search (tests/test_gpu_fri.py) finds only after its
first batch; which batch is derived here from the schedule written out in tests/pow_instance.py.

What is re-checked: every witness qualifies, under both permutations of the C oracle and under the Python model; for the four rows
below 2^22 NO smaller candidate qualifies (all of [0, witness) is scanned). For the two 26-bit rows only the 2^20 candidates just
below the witness and the first 2^20 from 0 are scanned here: their full minimality is proven by the generator
(tests/golden/gen_pow_witnesses.py), which scans everything, and not by this test."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pow_instance as pi  # noqa: E402
from oracle import accel, fri_ref, pyref  # noqa: E402
from oracle import oracle as o  # noqa: E402

ROWS = pi.load()


def test_the_rows_are_the_instances_of_the_list():
    assert [(r["seed"], r["bits"]) for r in ROWS] == pi.ROWS
    for r in ROWS:
        assert (r["batch"], r["batch_lo"], r["batch_size"]) == pi.batch_of(r["witness"])
        assert r["batch_lo"] <= r["witness"] < r["batch_lo"] + r["batch_size"]


def test_the_batch_schedule_written_out_here():
    """2^17, doubling, capped at 2^24: batch k starts at 2^17 (2^(k-1) - 1) up to the first capped one"""
    assert pi.batch_of(0) == (1, 0, 1 << 17) and pi.batch_of((1 << 17) - 1)[0] == 1
    assert pi.batch_of(1 << 17) == (2, 1 << 17, 1 << 18)
    assert pi.batch_of((1 << 17) + (1 << 18)) == (3, 3 << 17, 1 << 19)
    assert pi.FIRST_CAPPED == 8
    assert pi.batch_of((1 << 24) - (1 << 17) - 1) == (7, 63 << 17, 1 << 23)
    assert pi.batch_of((1 << 24) - (1 << 17)) == (8, (1 << 24) - (1 << 17), 1 << 24)
    assert pi.batch_of((1 << 25) - (1 << 17)) == (9, (1 << 25) - (1 << 17), 1 << 24)  # no more doubling
    assert pi.batch_of((1 << 25) - (1 << 17) + (1 << 24)) == (10, (1 << 25) - (1 << 17) + (1 << 24), 1 << 24)


def test_the_rows_cover_the_batches_beyond_the_first():
    """batches 2, 3, 4 and 5 (the base advance and three doublings), the first batch of the capped size, and a later capped one.
    If the device search's schedule changes, this is the assertion to revisit: new rows are needed, not a weaker test."""
    batches = [r["batch"] for r in ROWS]
    assert set(batches[:5]) == {2, 3, 4, 5, pi.FIRST_CAPPED}
    assert batches[5] > pi.FIRST_CAPPED + 1  # several batches of 2^24 in a row
    assert all(r["batch_size"] == pi.LARGEST_BATCH for r in ROWS[4:])


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "seed%d-%dbits" % (r["seed"], r["bits"]))
def test_each_witness_qualifies_and_nothing_scanned_below_it_does(row):
    st, min_lz, w = pi.state(row["seed"]), pi.min_leading_zeros(row["bits"]), row["witness"]
    s = list(st)
    s[pi.POS] = w
    resp = int(o.canon(o.poseidon(s))[7])
    assert resp == row["response"] == int(o.canon(o.poseidon(s, naive=True))[7]) == pyref.poseidon(s)[7]
    assert 64 - resp.bit_length() >= min_lz
    assert o.pow_search(st, pi.POS, min_lz, w, w + 1) == w
    if w < 1 << 22:
        assert o.pow_search(st, pi.POS, min_lz, 0, w) is None  # all of [0, witness)
    else:  # a part only: the generator scanned the rest
        assert o.pow_search(st, pi.POS, min_lz, w - (1 << 20), w) is None
        assert o.pow_search(st, pi.POS, min_lz, 0, 1 << 20) is None


def test_the_c_search_equals_the_python_model():
    """one permutation at a time in Python against the sliced, threaded C search: every position, ranges that start anywhere, a range
    without a witness, one thread and several, a state word >= p taken as given"""
    for pos in (0, 3, 11):
        for bits in (0, 7):
            st = pi.state(200 + pos)
            want = pyref.pow_search(st, pos, bits)
            for threads in (1, 3):
                assert o.pow_search(st, pos, bits, 0, pi.P, threads=threads) == want
            assert o.pow_search(st, pos, bits, 0, want) is None
            assert o.pow_search(st, pos, bits, want, want) is None  # an empty range
            nxt = o.pow_search(st, pos, bits, want + 1, pi.P)
            assert nxt > want
            s = list(st)
            s[pos] = nxt
            assert 64 - pyref.poseidon(s)[7].bit_length() >= bits
            assert all(64 - pyref.poseidon(s[:pos] + [c] + s[pos + 1:])[7].bit_length() < bits for c in range(want + 1, min(nxt, want + 60)))
    st = pi.state(300)
    lifted = list(st)
    lifted[5] += pi.P
    assert o.pow_search(lifted, 3, 7, 0, pi.P) == pyref.pow_search(st, 3, 7)
    # more candidates than one slice of the search holds, on a thread count that does not divide it
    assert o.pow_search(st, 3, 64, 0, 100_000, threads=3) is None


def test_the_reference_prover_searches_in_c_under_the_c_backend():
    """fri_ref.fri_proof_of_work: the same witness and the same transcript with and without accel.c_backend()"""
    out = []
    for backend in (False, True):
        ch = fri_ref.Challenger()
        ch.observe_elements(list(range(50, 61)))  # three elements left in the input buffer
        assert len(ch.input_buffer) == 3
        if backend:
            with accel.c_backend():
                assert pyref.pow_search is not _python_search
                w = fri_ref.fri_proof_of_work(ch, dict(proof_of_work_bits=10))
        else:
            w = fri_ref.fri_proof_of_work(ch, dict(proof_of_work_bits=10))
        out.append((w, ch.get_n_challenges(4)))
    assert out[0] == out[1] and pyref.pow_search is _python_search


_python_search = pyref.pow_search
