"""Differential campaign one level below fuzz_prove.py: randomly shaped NTTs, coset LDEs and
PolynomialBatch commits on the device against the C oracle (oracle/gl_oracle.c).

fuzz_case(i) is case i of the fixed list CASES (seed SEED, the small branch) that tests/test_gpu_commit_fuzz.py runs on the device;
tests/test_commit_fuzz.py asserts on the CPU what that list reaches. The same functions behind a command line, for longer campaigns
on a GPU box:
    python tests/fuzz_commit.py [cases=60] [seed=1] [large]
`large`: 2^13..2^22 rows (every two-pass decomposition, wide and narrow tiles, ragged tiles, the split columns of 2^21, three passes at 2^22),
1..5 polynomials, rate 0..1.
Shapes: 1..48 polynomials (crossing the 8-element sponge block and the <=4 `not hashed` rule), 2^0..2^13
rows, rate 0..3 bits, every legal cap height, values that are NOT canonical (>= p) in a tenth of the
cases, from_values and from_coeffs, with and without the leaf-major copy; forward / inverse NTT with
natural and bit-reversed output. Exits non-zero on the first mismatch."""
import json
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import oracle as o  # noqa: E402

P = 0xFFFFFFFF00000001
SEED = 176
CASES = list(range(30))


def raw_words(nprng, shape):
    """any u64 is a legal representative at the boundary (goldilocks_field.rs:26). Of uniform 64-bit words only one in 2^32 is >= p,
    so a quarter of the words are drawn from [p, 2^64) outright"""
    words = nprng.integers(0, 2**64, size=shape, dtype=np.uint64)
    high = np.uint64(P) + nprng.integers(0, 2**32 - 1, size=shape, dtype=np.uint64)
    return np.where(nprng.random(size=shape) < 0.25, high, words)


def rand_values(nprng, shape, non_canonical):
    return raw_words(nprng, shape) if non_canonical else nprng.integers(0, P, size=shape, dtype=np.uint64)


def bitrev_perm(n):
    bits = n.bit_length() - 1
    idx = np.arange(n, dtype=np.int64)
    out = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        out |= ((idx >> b) & 1) << (bits - 1 - b)
    return out


def cases(count, seed, large=False):
    """the first `count` cases of the campaign with this seed: dict(index, value_seed, log_n, n_polys, rate_bits, cap_height,
    non_canonical, from_values, leaf_major, opened = three leaf indices)"""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        if large:
            log_n = rng.choice([13, 14, 15, 16, 17, 18, 19, 20, 21, 22])
            n_polys = rng.choice([1, 2, 3, 5])
            rate_bits = rng.choice([0, 1]) if log_n < 21 else 0  # the LDE of 2^21 and 2^22 rows is in test_gpu_ntt.py
            cap_height = rng.randrange(0, 6)
        else:
            log_n = rng.choice([0, 1, 2, 3, 5, 7, 9, 10, 11, 12, 13])
            n_polys = rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 31, 48])
            rate_bits = rng.choice([0, 1, 2, 3])
            cap_height = rng.randrange(0, log_n + rate_bits + 1)
        non_canonical = rng.random() < 0.1
        from_values = rng.random() < 0.5
        leaf_major = rng.random() < 0.5
        opened = [rng.randrange(1 << (log_n + rate_bits)) for _ in range(3)]
        out.append(dict(index=k, value_seed=(seed, k), log_n=log_n, n_polys=n_polys, rate_bits=rate_bits, cap_height=cap_height,
                        non_canonical=non_canonical, from_values=from_values, leaf_major=leaf_major, opened=opened))
    return out


def fuzz_case(i):
    return cases(len(CASES), SEED)[CASES[i]]


def describe(case):
    return str({k: v for k, v in case.items() if k not in ("index", "value_seed", "opened")})


def values(case):
    return rand_values(np.random.default_rng(case["value_seed"]), (case["n_polys"], 1 << case["log_n"]), case["non_canonical"])


def check(ctx, case):
    """None when everything the device computes for the case equals the C oracle's, else the name of the first thing that differs"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    log_n, n_polys, rate_bits, cap_height = case["log_n"], case["n_polys"], case["rate_bits"], case["cap_height"]
    vals = values(case)
    # ---- commit
    if case["from_values"]:
        b = pg.PolynomialBatch.from_values(ctx, vals, rate_bits, False, cap_height, leaf_major=case["leaf_major"])
        exp = o.commit_from_values(vals, rate_bits, cap_height, threads=4)
    else:
        b = pg.PolynomialBatch.from_coeffs(ctx, vals, rate_bits, False, cap_height, leaf_major=case["leaf_major"])
        exp = o.commit_from_coeffs(vals, rate_bits, cap_height, threads=4)
    if not (b.merkle_tree.cap == o.canon(exp["cap"])).all():
        return "the Merkle cap"
    if not (b.merkle_tree.digests == o.canon(exp["digests"]).reshape(-1, 4)).all():
        return "the digests"
    if case["from_values"] and not (b.polynomials == o.canon(exp["coeffs"])).all():
        return "the coefficients"
    leaves = o.canon(exp["leaves"])
    if not (b.lde_column_major() == leaves.T).all():
        return "the LDE, column-major"
    if case["leaf_major"] and not (b.merkle_tree.d_leaves.download().reshape(leaves.shape) == leaves).all():
        return "the leaf-major copy"
    lv, sib = b.merkle_tree.open_batch(case["opened"])
    for q, i in enumerate(case["opened"]):
        if not (lv[q] == leaves[i]).all():
            return f"the opened leaf {i}"
        if not o.merkle_verify(leaves[i], i, exp["cap"], sib[q]):
            return f"the Merkle path of leaf {i}"
    # ---- NTT on the same data: forward natural, forward bit-reversed, inverse round trip
    x = vals.copy()
    nat = pg.fft_with_options(ctx, x)
    want = o.canon(o.fft_batch(x.copy(), threads=4))
    if not (nat == want).all():
        return "the forward NTT, natural order"
    buf = pg.DeviceBuffer.from_host(ctx, x)
    n = 1 << log_n
    _lib.call("gl_ntt_batch", buf.ptr, n_polys, log_n, n, 0, 1, ctx.ptr)  # bit-reversed output
    if not (buf.download().reshape(n_polys, n) == want[:, bitrev_perm(n)]).all():
        return "the forward NTT, bit-reversed order"
    buf.upload(want)
    _lib.call("gl_ntt_batch", buf.ptr, n_polys, log_n, n, 1, 0, ctx.ptr)  # inverse, natural
    if not (buf.download().reshape(n_polys, n) == o.canon(x)).all():
        return "the inverse NTT"
    return None


def main():
    import plonky2_gpu_amd as pg

    count = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    large = len(sys.argv) > 3 and sys.argv[3] == "large"
    ctx = pg.Context(0)
    t0 = time.time()
    for case in cases(count, seed, large):
        diff = check(ctx, case)
        print(f"case {case['index']:3d} {'FAIL' if diff else 'ok  '} {describe(case)}", flush=True)
        if diff:
            print(json.dumps(dict(failed_case=case["index"], seed=seed, difference=diff,
                                  **{k: v for k, v in case.items() if k not in ("index", "value_seed", "opened")})))
            sys.exit(1)
    print(json.dumps(dict(cases=count, seed=seed, all_equal=True, seconds=round(time.time() - t0, 1))))


if __name__ == "__main__":
    main()
