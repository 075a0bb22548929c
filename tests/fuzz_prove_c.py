"""Differential campaign against the C prover (oracle/prove_oracle.c), which is fast enough for larger and wider cases than
fuzz_prove.py's Python oracle: randomly shaped circuits of three families — the four basic gates (12 wires), every gate kind of the
ed25519 list (135 wires), the recursion-shaped circuit with the eight upstream gate kinds (135 wires) — at 2^3 .. 2^12 rows, random
FRI shapes, rate, cap height, proof-of-work bits, query counts, compiled or interpreted gates, and blinded (gl_prove_zk with random
salts, a tenth of them raw 64-bit words, a quarter of those >= p) in a third of the cases. Every proof byte for byte.

fuzz_case(i) is case i of the fixed list CASES (seed SEED, at most 2^MAX_DEGREE_BITS rows) that tests/test_gpu_prove_fuzz.py runs on
the device; tests/test_prove_fuzz.py asserts on the CPU what that list reaches. The same functions behind a command line, for longer
campaigns on a GPU box:
    python tests/fuzz_prove_c.py [cases=40] [seed=1]"""
import json
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from fuzz_commit import raw_words  # noqa: E402
from fuzz_prove import first_difference  # noqa: E402
from oracle import accel, prove_c  # noqa: E402
from plonk_instance import make_circuit, make_full_circuit, make_recursion_circuit  # noqa: E402

P = 0xFFFFFFFF00000001
RATE_BITS = 3
SEED = 281
CASES = list(range(12))
MAX_DEGREE_BITS = 10  # of the fixed list; the command line goes to 2^12


def fri_shape(rng, degree_bits, rate_bits):
    cap_height = rng.choice([0, 1, 2, 3, 4])
    cap_height = min(cap_height, degree_bits + rate_bits)
    arity, bits = [], degree_bits
    while bits > 0 and rng.random() < 0.8:
        ab = rng.choice([1, 2, 3, 4, 4])
        if ab > bits or bits + rate_bits - ab < cap_height:
            break
        arity.append(ab)
        bits -= ab
    return cap_height, tuple(arity)


def cases(count, seed, max_degree_bits=12):
    """the first `count` cases of the campaign with this seed: dict(index, circuit_seed, family, degree_bits, kw = the arguments of
    the family's make_*circuit, blinded, raw_salts, salt_seed, compile_gates)"""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        family = rng.choice(["mini", "mini", "full", "recursion"])
        sizes = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12] if family == "mini" else [4, 5, 6, 7, 8, 9, 10]
        degree_bits = rng.choice([b for b in sizes if b <= max_degree_bits])
        cap_height, arity = fri_shape(rng, degree_bits, RATE_BITS)
        kw = dict(arity_bits=arity, cap_height=cap_height, pow_bits=rng.choice([0, 2, 5, 9]), num_queries=rng.choice([1, 3, 7, 28]))
        if family == "mini":
            kw.update(two_groups=rng.random() < 0.5, num_challenges=rng.choice([1, 2, 2, 3]))
        blinded = rng.random() < 0.33
        raw_salts = blinded and rng.random() < 0.3
        out.append(dict(index=k, circuit_seed=7000 * seed + k, family=family, degree_bits=degree_bits, kw=kw, blinded=blinded,
                        raw_salts=raw_salts, salt_seed=seed * 100003 + k, compile_gates=rng.random() < 0.5))
    return out


def fuzz_case(i):
    return cases(len(CASES), SEED, MAX_DEGREE_BITS)[CASES[i]]


def describe(case):
    return (f"{case['family']:9s} 2^{case['degree_bits']:<2d} compile={int(case['compile_gates'])} blinded={int(case['blinded'])} "
            f"raw_salts={int(case['raw_salts'])} {case['kw']}")


def build(case):
    """(circuit, wires, public inputs, salts or None) of a case"""
    make = dict(mini=make_circuit, full=make_full_circuit, recursion=make_recursion_circuit)[case["family"]]
    with accel.c_backend():
        circuit, wires, pis = make(case["degree_bits"], seed=case["circuit_seed"], **case["kw"])
    salts = None
    if case["blinded"]:
        circuit = dict(circuit, fri_params=dict(circuit["fri_params"], hiding=True))
        n_ext = 1 << (case["degree_bits"] + RATE_BITS)
        nprng = np.random.default_rng(case["salt_seed"])
        salts = raw_words(nprng, (3, 4, n_ext)) if case["raw_salts"] else nprng.integers(0, P, size=(3, 4, n_ext), dtype=np.uint64)
    return circuit, wires, pis, salts


def check(ctx, case):
    """None when the device's proof equals the C prover's byte for byte, else the first difference; case["bytes"] = the proof's length"""
    import plonky2_gpu_amd as pg

    circuit, wires, pis, salts = build(case)
    exp = prove_c.prove(circuit, wires, pis, salts=salts)
    nc = pg.NativeCircuit(ctx, dict(circuit, circuit_digest=None), compile_gates=case["compile_gates"])
    try:
        got = nc.prove_bytes(wires, pis, salts=salts)
    finally:
        nc.close()
    case["bytes"] = len(got)
    return first_difference(got, exp)


def main():
    import plonky2_gpu_amd as pg

    count = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    ctx = pg.Context(0)
    t0 = time.time()
    for case in cases(count, seed):
        diff = check(ctx, case)
        print(f"case {case['index']:3d} {'FAIL' if diff else 'ok  '} {case['bytes']:7d} B {describe(case)}", flush=True)
        if diff:
            print(json.dumps(dict(failed_case=case["index"], seed=seed, family=case["family"], degree_bits=case["degree_bits"],
                                  compile_gates=case["compile_gates"], blinded=case["blinded"], difference=diff)))
            sys.exit(1)
    print(json.dumps(dict(cases=count, seed=seed, all_equal=True, oracle="oracle/prove_oracle.c", seconds=round(time.time() - t0, 1))))


if __name__ == "__main__":
    main()
