"""Differential campaign: randomly shaped small circuits through gl_prove (native prover), each proof
compared byte for byte with the oracle's (oracle/prove_ref.py). Shapes vary in degree, selector
grouping, FRI arities, rate, cap height, proof-of-work bits, query count, quotient degree factor,
number of challenges and gate compilation.

fuzz_case(i) is case i of the fixed list CASES (seed SEED) that tests/test_gpu_prove_fuzz.py runs on the device;
tests/test_prove_fuzz.py asserts on the CPU what that list reaches. The same functions behind a command line, for longer campaigns
on a GPU box:
    python tests/fuzz_prove.py [cases=40] [seed=1]
Prints one line per case and a JSON summary; exits non-zero on the first mismatch."""
import json
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import prove_ref, serialize_ref  # noqa: E402
from plonk_instance import make_circuit  # noqa: E402

SEED = 9
CASES = list(range(12))


def random_shape(rng):
    degree_bits = rng.choice([3, 4, 4, 5, 5, 6])
    two_groups = rng.random() < 0.5
    rate_bits = rng.choice([1, 2, 3, 3])
    qdf_min = 4 if two_groups else 5
    qdf = rng.choice([q for q in (4, 5, 6, 7, 8) if qdf_min <= q <= (1 << rate_bits)] or [None])
    if qdf is None:  # the quotient degree must fit the rate (prover.rs:807-811)
        rate_bits, qdf = 3, rng.choice([q for q in (5, 6, 7, 8) if q >= qdf_min])
    # reduction arities: keep every layer at least as large as the cap (reduction_strategies.rs:38-48)
    cap_height = rng.choice([0, 1, 2])
    arity, bits = [], degree_bits
    while bits > 0 and rng.random() < 0.75:
        ab = rng.choice([1, 1, 2, 3, 4])
        if ab > bits or bits + rate_bits - ab < cap_height:
            break
        arity.append(ab)
        bits -= ab
    return dict(degree_bits=degree_bits, two_groups=two_groups, rate_bits=rate_bits, cap_height=cap_height, arity_bits=tuple(arity),
                pow_bits=rng.choice([0, 1, 3, 6]), num_queries=rng.choice([1, 2, 4]), quotient_degree_factor=qdf,
                num_challenges=rng.choice([1, 2, 2, 3]))


def cases(count, seed):
    """the first `count` cases of the campaign with this seed: dict(index, circuit_seed, shape, compile_gates)"""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        shape = random_shape(rng)
        out.append(dict(index=k, circuit_seed=1000 * seed + k, shape=shape, compile_gates=rng.random() < 0.5))
    return out


def fuzz_case(i):
    return cases(len(CASES), SEED)[CASES[i]]


def describe(case):
    return f"compile={int(case['compile_gates'])} {case['shape']}"


def check(ctx, case):
    """None when the device's proof equals the oracle's byte for byte, else the first difference; case["bytes"] = the proof's length"""
    import plonky2_gpu_amd as pg

    circuit, wires, pis = make_circuit(seed=case["circuit_seed"], **case["shape"])
    exp = serialize_ref.proof_bytes(prove_ref.prove(circuit, wires, pis))
    nc = pg.NativeCircuit(ctx, dict(circuit, circuit_digest=None), compile_gates=case["compile_gates"])
    try:
        got = nc.prove_bytes(wires, pis)
    finally:
        nc.close()
    case["bytes"] = len(got)
    return first_difference(got, exp)


def first_difference(got, exp):
    if got == exp:
        return None
    if len(got) != len(exp):
        return f"{len(got)} bytes, the oracle's proof has {len(exp)}"
    at = next(k for k in range(len(exp)) if got[k] != exp[k])
    return f"byte {at} of {len(exp)}: {got[at]:#04x}, the oracle has {exp[at]:#04x}"


def main():
    import plonky2_gpu_amd as pg

    count = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    ctx = pg.Context(0)
    t0 = time.time()
    for case in cases(count, seed):
        diff = check(ctx, case)
        print(f"case {case['index']:3d} {'FAIL' if diff else 'ok  '} {case['bytes']:6d} B {describe(case)}", flush=True)
        if diff:
            print(json.dumps(dict(failed_case=case["index"], seed=seed, shape=case["shape"], compile_gates=case["compile_gates"], difference=diff)))
            sys.exit(1)
    print(json.dumps(dict(cases=count, seed=seed, all_equal=True, seconds=round(time.time() - t0, 1))))


if __name__ == "__main__":
    main()
