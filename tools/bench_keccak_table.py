#!/usr/bin/env python3
"""The Keccak-f table (plonky2_gpu_amd/keccak_table.py, csrc/keccak_table.hip): its trace built on the device, against the store
floor of its 2430 columns and against a host route, and whole interpreted proofs of it. Per size:

  trace       gl_keccak_table_trace of floor(n / 24) random inputs into a resident buffer, timed by events on the context's stream,
              warm, median of --reps runs: milliseconds, 2430 * 8 * n bytes / time, and that as a fraction of the 8 TB/s
              specification. Next to it gl_memset_zero of the same buffer: the rate a pure store stream of the runtime reaches.
  numpy       the same inputs through tests/keccak_table_ref.py's generate_trace_rows (numpy over all permutations at once) on
              the host, at the sizes where that takes under a minute; its rows must equal the device's.
  prove       gl_stark_prove of the device-built trace, interpreted, under starky's standard_fast_config, with its stage times
              (sizes --prove-bits, default 12 and 14)

Oracle-free; the reference verifier accepts the proofs of `prove` at 2^12 and 2^14 rows in tests/test_gpu_stark_scale.py, which takes
inputs_for and the parameters from here. One JSON line on stdout and in --out (default profiles/keccak_table.json).

  python tools/bench_keccak_table.py [--bits 14 16 18 20] [--prove-bits 12 14] [--reps 7] [--device LABEL] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import plonky2_gpu_amd as pg
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd import keccak_table as kt

SPEC_BYTES_PER_S = 8e12  # the 8 TB/s of the MI355X's specification


def fast_config_fri_params(degree_bits):
    """FriConfig::fri_params of standard_fast_config (plonky2/src/fri/reduction_strategies.rs:38-49)"""
    rate_bits, cap_height, arity, final_poly_bits = 1, 4, 4, 5
    arities, db = [], degree_bits
    while db > final_poly_bits and db + rate_bits - arity >= cap_height:
        arities.append(arity)
        db -= arity
    return dict(rate_bits=rate_bits, cap_height=cap_height, proof_of_work_bits=16, num_query_rounds=84, reduction_arity_bits=arities, hiding=False)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def inputs_for(bits):
    n = 1 << bits
    return np.random.default_rng(bits).integers(0, 1 << 64, size=(n // 24, 25), dtype=np.uint64)


def timed(ctx, reps, call):
    e0, e1 = pg.Event(), pg.Event()
    ms = []
    for rep in range(reps + 2):  # two warm-up calls
        ctx.synchronize()
        e0.record(ctx)
        call()
        e1.record(ctx)
        ctx.synchronize()
        if rep >= 2:
            ms.append(e1.elapsed_ms_since(e0))
    return ms


def measure_trace(ctx, bits, reps, numpy_budget_s):
    n = 1 << bits
    inputs = inputs_for(bits)
    d_in = pg.DeviceBuffer.from_host(ctx, inputs)
    d_trace = pg.DeviceBuffer(ctx, kt.NUM_COLUMNS * n)
    nbytes = kt.NUM_COLUMNS * 8 * n
    ms = timed(ctx, reps, lambda: _lib.call("gl_keccak_table_trace", d_in.ptr, inputs.shape[0], bits, d_trace.ptr, n, ctx.ptr))
    memset = timed(ctx, reps, lambda: _lib.call("gl_memset_zero", d_trace.ptr, nbytes, ctx.ptr))
    med = float(np.median(ms))
    res = {"rows": n, "inputs": int(inputs.shape[0]), "bytes": nbytes, "trace": stats(ms), "trace_tb_per_s": round(nbytes / med / 1e9, 3),
           "fraction_of_8_tb_per_s": round(nbytes / (med * 1e-3) / SPEC_BYTES_PER_S, 4), "memset_same_buffer": stats(memset),
           "memset_tb_per_s": round(nbytes / float(np.median(memset)) / 1e9, 3)}
    if numpy_budget_s is not None:
        import keccak_table_ref as kr

        t0 = time.perf_counter()
        rows = kr.generate_trace_rows(inputs, n)
        res["numpy_host_s"] = round(time.perf_counter() - t0, 3)
        _lib.call("gl_keccak_table_trace", d_in.ptr, inputs.shape[0], bits, d_trace.ptr, n, ctx.ptr)
        for c0 in range(0, kt.NUM_COLUMNS, 270):  # compared in slabs of 270 columns
            got = d_trace.download(c0 * n, 270 * n).reshape(270, n)
            if not (got == rows[:, c0 : c0 + 270].T).all():
                raise SystemExit("bench_keccak_table: the device's trace differs from the host's at 2^%d rows" % bits)
        res["equals_numpy"] = True
        res["numpy_over_device"] = round(res["numpy_host_s"] * 1e3 / med, 1)
    d_in.free(), d_trace.free()
    return res


def measure_prove(ctx, bits, reps):
    n = 1 << bits
    desc = kt.stark_desc(bits, 2, fast_config_fri_params(bits))
    d_trace = kt.generate_trace(ctx, inputs_for(bits), bits)
    ns = pg.NativeStark(ctx, desc)
    first = ns.prove_bytes(d_trace, [])
    ns.prove_bytes(d_trace, [])
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        data = ns.prove_bytes(d_trace, [])
        ms.append((time.perf_counter() - t0) * 1e3)
        if data != first:
            raise SystemExit("bench_keccak_table: the proof is not deterministic")
    timing = {}
    ns.prove_bytes(d_trace, [], timing)
    ns.close()
    d_trace.free()
    return dict(stats(ms), rows=n, proof_bytes=len(first), program_instructions=int(desc.instrs.shape[0]), stage_ms={k: round(v, 3) for k, v in timing.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[14, 16, 18, 20])
    ap.add_argument("--prove-bits", type=int, nargs="*", default=[12, 14])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--numpy-max-seconds", type=float, default=60.0, help="the host trace is timed while the next size is expected to stay below this")
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keccak_table.json"))
    a = ap.parse_args()
    if a.reps < 5 or not all(5 <= b <= 20 for b in a.bits + a.prove_bits):
        ap.error("--reps >= 5; sizes in 2^5 .. 2^20 rows (a trace at 2^20 rows is 20.4 GB)")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_keccak_table.py", "device": a.device, "library": _lib.load().gl_version().decode(), "reps": a.reps,
           "columns": kt.NUM_COLUMNS, "store_floor": "2430 * 8 * n bytes against 8 TB/s",
           "prove_config": "KeccakStark: 2430 columns, degree 3, interpreted program, Poseidon, standard_fast_config (2 challenges, rate_bits 1, "
                           "cap_height 4, 16 PoW bits, arity 4 down to 2^5, 84 queries); trace built on the device and resident",
           "trace": {}, "prove": {}}
    expected_numpy_s = 0.0
    for bits in sorted(a.bits):
        budget = a.numpy_max_seconds if expected_numpy_s < a.numpy_max_seconds and bits <= 18 else None
        entry = measure_trace(ctx, bits, a.reps, budget)
        if "numpy_host_s" in entry:
            expected_numpy_s = entry["numpy_host_s"] * 4.5  # the next size listed is usually four times this one
        res["trace"]["2^%d" % bits] = entry
    for bits in a.prove_bits:
        res["prove"]["2^%d" % bits] = measure_prove(ctx, bits, a.reps)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
