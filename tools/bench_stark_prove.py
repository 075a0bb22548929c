#!/usr/bin/env python3
"""Whole STARK proofs (gl_stark_create / gl_stark_prove) of two shapes under starky's standard_fast_config (2 challenges, rate_bits 1,
cap_height 4, 16 proof-of-work bits, ConstantArityBits(4, 5), 84 query rounds; starky/src/config.rs:17-29):

  fibonacci  the reference's FibonacciStark: 4 columns, degree 2, one permutation pair
  wide       100 columns, degree 3: a counter and 33 triples (a, b, c) with c = a * b * counter on every row, two permutation-free
             transition / boundary constraints on the counter: 35 constraints, quotient_degree_factor 2

at 2^16 .. 2^20 rows, trace resident in HBM. Per shape and size: the handle is created and warmed (two proofs), then `--reps` proofs
are timed by the wall clock around gl_stark_prove (it ends synchronised); median, min and max, and the h_stage_ms breakdown of one
further proof. Oracle-free: every proof must equal the first one and round-trip through the wire format. One JSON line on stdout
(and --out, by default profiles/stark_prove.json).

  python tools/bench_stark_prove.py [--min-bits 16] [--max-bits 20] [--reps 7] [--out profiles/stark_prove.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import plonky2_gpu_amd as pg
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd import stark as pstark

P = 0xFFFFFFFF00000001
WIDE_TRIPLES = 33


def fast_config_fri_params(degree_bits):
    """FriConfig::fri_params of standard_fast_config (plonky2/src/fri/reduction_strategies.rs:38-49)"""
    rate_bits, cap_height, arity, final_poly_bits = 1, 4, 4, 5
    arities, db = [], degree_bits
    while db > final_poly_bits and db + rate_bits - arity >= cap_height:
        arities.append(arity)
        db -= arity
    return dict(rate_bits=rate_bits, cap_height=cap_height, proof_of_work_bits=16, num_query_rounds=84, reduction_arity_bits=arities, hiding=False)


def fibonacci(ctx, degree_bits):
    """(description, trace in HBM, public inputs) of FibonacciStark (starky/src/fibonacci_stark.rs)"""
    a = pstark.StarkAsm()
    a.emit_first_row(a.sub(a.local(0), a.pi(0)))
    a.emit_first_row(a.sub(a.local(1), a.pi(1)))
    a.emit_last_row(a.sub(a.local(1), a.pi(2)))
    a.release()
    a.emit_transition(a.sub(a.next(0), a.local(1)))
    a.emit_transition(a.sub(a.sub(a.next(1), a.local(0)), a.local(1)))
    instrs, imms = a.program()
    n = 1 << degree_bits
    trace = np.zeros((4, n), dtype=np.uint64)
    x0, x1 = 0, 1
    for r in range(n):
        trace[0, r], trace[1, r] = x0, x1
        x0, x1 = x1, (x0 + x1) % P
    trace[2] = np.arange(n, dtype=np.uint64)
    trace[3] = np.arange(1, n + 1, dtype=np.uint64)
    trace[3, n - 1] = 0
    desc = pstark.StarkDesc(degree_bits, 4, 3, 2, 2, fast_config_fri_params(degree_bits), instrs, imms, [[(2, 3)]])
    return desc, pg.DeviceBuffer.from_host(ctx, trace), [0, 1, int(trace[1, n - 1])]


def wide(ctx, degree_bits):
    """(description, trace in HBM, public inputs) of the 100-column degree-3 STARK; the products are formed on the device"""
    cols = 1 + 3 * WIDE_TRIPLES
    a = pstark.StarkAsm()
    a.emit_first_row(a.sub(a.local(0), a.pi(0)))
    a.emit_transition(a.sub(a.next(0), a.add(a.local(0), a.imm(1))))
    for j in range(WIDE_TRIPLES):
        a.release()
        c0 = a.local(0)
        a.emit(a.sub(a.local(3 + 3 * j), a.mul(a.mul(a.local(1 + 3 * j), a.local(2 + 3 * j)), c0)))
    instrs, imms = a.program()
    n = 1 << degree_bits
    rng = np.random.default_rng(degree_bits)
    trace = rng.integers(0, P, size=(cols, n), dtype=np.uint64)
    trace[0] = np.arange(5, n + 5, dtype=np.uint64)
    d_trace = pg.DeviceBuffer.from_host(ctx, trace)
    for j in range(WIDE_TRIPLES):  # c = (a * b) * counter, element-wise on the device (op 2: multiplication)
        out = d_trace.at((3 + 3 * j) * n)
        _lib.call("gl_debug_field_op", 2, d_trace.at((1 + 3 * j) * n), d_trace.at((2 + 3 * j) * n), out, n, ctx.ptr)
        _lib.call("gl_debug_field_op", 2, out, d_trace.at(0), out, n, ctx.ptr)
    ctx.synchronize()
    desc = pstark.StarkDesc(degree_bits, cols, 1, 3, 2, fast_config_fri_params(degree_bits), instrs, imms, [])
    return desc, d_trace, [5]


def measure(ctx, make, degree_bits, reps, hasher="poseidon"):
    """Poseidon trees: with 2 challenges both shapes have 4-element leaves somewhere (the Fibonacci trace, the wide quotient), which
    KeccakHash<25> cannot hash"""
    desc, d_trace, pis = make(ctx, degree_bits)
    ns = pg.NativeStark(ctx, desc, hasher)

    def prove(timing=None):
        t0 = time.perf_counter()
        data = ns.prove_bytes(d_trace, pis, timing)
        return (time.perf_counter() - t0) * 1e3, data

    first = prove()[1]
    prove()
    ms = []
    for _ in range(reps):
        t, data = prove()
        if data != first:
            raise SystemExit("bench_stark_prove: the proof is not deterministic")
        ms.append(t)
    timing = {}
    prove(timing)
    if pstark.proof_to_bytes(pstark.proof_from_bytes(first, desc, hasher), desc, hasher) != first:
        raise SystemExit("bench_stark_prove: the proof does not round-trip through the wire format")
    ns.close()
    d_trace.free()
    stages = {k: round(v, 3) for k, v in timing.items()}
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "proof_bytes": len(first),
            "columns": desc.num_columns, "stage_ms": stages, "largest_stage": max(stages, key=stages.get)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-bits", type=int, default=16)
    ap.add_argument("--max-bits", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="fibonacci,wide")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_prove.json"))
    a = ap.parse_args()
    if a.reps < 1 or not 6 <= a.min_bits <= a.max_bits <= 22:
        ap.error("--reps >= 1 and 6 <= --min-bits <= --max-bits <= 22")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_stark_prove.py", "library": _lib.load().gl_version().decode(), "hasher": "poseidon", "reps": a.reps,
           "config": "standard_fast_config: 2 challenges, rate_bits 1, cap_height 4, 16 PoW bits, arity 4 down to 2^5, 84 queries; trace resident"}
    makers = {"fibonacci": fibonacci, "wide": wide}
    for shape in a.shapes.split(","):
        res[shape] = {}
        for bits in range(a.min_bits, a.max_bits + 1):
            res[shape]["2^%d" % bits] = measure(ctx, makers[shape], bits, a.reps)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
