#!/usr/bin/env python3
"""Generate tests/golden/pow_witnesses.json: for each (seed, bits) of tests/pow_instance.ROWS the smallest proof-of-work witness of
the state [seed, seed + 1, .., seed + 11] with the candidate at position 3, and its response (word 7 of the permuted state), found
with the C search of oracle/gl_oracle.c (glo_pow_search over glo_poseidon). Minimality is PROVEN here: all of [0, witness) is
scanned and holds no qualifying candidate; the witness's response is recomputed with both permutations of the C oracle and with the
Python model. The in-suite re-check (tests/test_pow_fixture.py) scans the four rows below 2^22 in full and only parts of the two
26-bit rows. The largest row is about 9 * 10^7 permutations: a minute or two on a few cores.
Run:  python tests/golden/gen_pow_witnesses.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as o, pyref  # noqa: E402
import pow_instance as pi  # noqa: E402


def main():
    rows = []
    for seed, bits in pi.ROWS:
        t0 = time.time()
        st, min_lz = pi.state(seed), pi.min_leading_zeros(bits)
        w = o.pow_search(st, pi.POS, min_lz, 0, pi.P)
        assert w is not None
        assert o.pow_search(st, pi.POS, min_lz, 0, w) is None, "a smaller candidate qualifies"
        s = list(st)
        s[pi.POS] = w
        resp = pyref.poseidon(s)[7]
        assert resp == int(o.canon(o.poseidon(s))[7]) == int(o.canon(o.poseidon(s, naive=True))[7])
        assert 64 - resp.bit_length() >= min_lz
        index, lo, size = pi.batch_of(w)
        rows.append(dict(seed=seed, bits=bits, witness=w, response=resp, batch=index, batch_lo=lo, batch_size=size))
        print(rows[-1], "%.1f s" % (time.time() - t0), flush=True)
    with open(pi.FIXTURE, "w") as f:
        json.dump(dict(pos=pi.POS, state="[seed, seed + 1, .., seed + 11]", response="word 7 of the permuted state, canonical",
                       minimality="all of [0, witness) scanned by the generator", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
