"""Proof-of-work instances whose smallest witness lies beyond the first batch of the device search (TEST INFRASTRUCTURE ONLY).

The device search scans candidates in batches: 2^17 first, doubling while nothing is found, capped at 2^24. That schedule is WRITTEN
OUT here, not read from the library: if the library's schedule changes, tests/test_pow_fixture.py's coverage assertion is what has to
be revisited. The rows themselves are tests/golden/pow_witnesses.json (tests/golden/gen_pow_witnesses.py)."""
import json
import os

P = 0xFFFFFFFF00000001
POS = 3                                   # where the candidate goes into the state
ROWS = [(100, 18), (104, 18), (100, 22), (104, 22), (102, 26), (101, 26)]   # (seed, proof-of-work bits)
FIRST_BATCH, LARGEST_BATCH = 1 << 17, 1 << 24
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pow_witnesses.json")


def state(seed):
    return [seed + k for k in range(12)]


def min_leading_zeros(bits):
    return bits + (64 - P.bit_length())   # F::order() has 64 bits: the response's leading zeros as a u64


def batch_of(witness):
    """(index from 1, lo, size) of the batch that scans `witness`: sizes 2^17, 2^18, .. doubling up to 2^24, then 2^24 for ever"""
    lo, size, index = 0, FIRST_BATCH, 1
    while witness >= lo + size:
        lo, size, index = lo + size, min(2 * size, LARGEST_BATCH), index + 1
    return index, lo, size


FIRST_CAPPED = 1 + (LARGEST_BATCH // FIRST_BATCH).bit_length() - 1   # sizes double seven times: batch 8 is the first of 2^24


def load():
    with open(FIXTURE) as f:
        return json.load(f)["rows"]
