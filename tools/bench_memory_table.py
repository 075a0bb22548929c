#!/usr/bin/env python3
"""The memory table (plonky2_gpu_amd/memory_table.py, csrc/memory_table.hip): its trace built on the device from the unsorted
operation list, stage by stage, against the upload of a finished trace, and whole proofs of it. Per number of operations:

  stages      gl_debug_memory_table_stage_ms: the call with an event between its stages — the sort (four rounds of the radix sort
              over field << 32 | position), the gaps (dummies per pair, their prefix sums, the decision), the rows (one thread per
              row of the trace: 14 columns from the operation, the zeros, COUNTER), the flags (first-change flags and RANGE_CHECK
              from rows r and r + 1), the lookup columns (permuted_cols of RANGE_CHECK against COUNTER) — warm, median of --reps
  call        gl_memory_table_trace and the wait for the stream, by the wall clock: the stages plus the host's one wait for the count
  upload      a finished 26-column trace of the same height from pageable host memory into the same buffer, by the wall clock:
              what the host route pays after it has generated the trace
  prove       gl_stark_prove of the device-built trace, interpreted, under starky's standard_fast_config, with its stage times
              (--prove-bits; the trace of such a list need not satisfy the constraints: the prover does the same work, and with
              quotient_degree_factor 2 it cannot fail)

The lists are shaped like an execution: five contexts of unequal weight, segments below 32, addresses in 64 clusters of 1024 words,
timestamps rising in list order, seven reads in ten operations. Oracle-free. One JSON line on stdout and in --out (default
profiles/memory_table.json).

  python tools/bench_memory_table.py [--bits 16 18 20 22] [--prove-bits 16 18 20] [--reps 7] [--device LABEL] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import plonky2_gpu_amd as pg
from bench_common import fast_config_fri_params, stats
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd import memory_table as mt

STAGES = ("sort", "gaps", "rows", "flags", "lookup_columns")


def ops_for(bits):
    """[2^bits][14] operations in the order an execution issues them"""
    num_ops = 1 << bits
    rng = np.random.default_rng(bits)
    w = np.zeros((num_ops, mt.OP_WORDS), dtype=np.uint64)
    w[:, mt.FILTER] = 1
    w[:, mt.TIMESTAMP] = np.arange(num_ops)  # clock * NUM_CHANNELS + channel with every channel in use
    w[:, mt.IS_READ] = rng.random(num_ops) < 0.7
    w[:, mt.ADDR_CONTEXT] = rng.choice(5, size=num_ops, p=[0.5, 0.2, 0.15, 0.1, 0.05])
    w[:, mt.ADDR_SEGMENT] = np.minimum(rng.geometric(0.25, size=num_ops) - 1, 31)
    bases = rng.integers(0, 1 << 24, size=64, dtype=np.uint64)
    w[:, mt.ADDR_VIRTUAL] = bases[rng.integers(0, 64, size=num_ops)] + rng.integers(0, 1024, size=num_ops, dtype=np.uint64)
    w[:, mt.VALUE_START :] = rng.integers(0, 1 << 32, size=(num_ops, mt.VALUE_LIMBS), dtype=np.uint64)
    return w


def wall(ctx, reps, call):
    ms = []
    for rep in range(reps + 2):  # two warm-up calls
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        if rep >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def measure_trace(ctx, bits, reps):
    w = ops_for(bits)
    num_ops = w.shape[0]
    d_ops = pg.DeviceBuffer.from_host(ctx, w)
    rows = mt.rows(ctx, d_ops)
    degree_bits = (rows - 1).bit_length()
    n = 1 << degree_bits
    scratch = pg.DeviceBuffer(ctx, _lib.load().gl_memory_table_scratch_bytes(num_ops, degree_bits) // 8)
    d_trace = pg.DeviceBuffer(ctx, mt.NUM_COLUMNS * n)
    stage_ms = np.zeros((reps + 2, len(STAGES)), dtype=np.float32)
    for rep in range(reps + 2):
        _lib.call("gl_debug_memory_table_stage_ms", d_ops.ptr, num_ops, degree_bits, d_trace.ptr, n, scratch.ptr, stage_ms[rep].ctypes.data, ctx.ptr)
    stage_ms = stage_ms[2:]
    count = ctypes.c_uint64()
    call_ms = wall(ctx, reps, lambda: _lib.call("gl_memory_table_trace", d_ops.ptr, num_ops, degree_bits, d_trace.ptr, n, scratch.ptr,
                                                ctypes.byref(count), ctx.ptr))
    count_ms = wall(ctx, reps, lambda: _lib.call("gl_memory_table_trace", d_ops.ptr, num_ops, degree_bits, None, 0, scratch.ptr, ctypes.byref(count), ctx.ptr))
    finished = d_trace.download()  # pageable host memory holding a finished trace
    upload_ms = wall(ctx, reps, lambda: d_trace.upload(finished))
    ops_upload_ms = wall(ctx, reps, lambda: d_ops.upload(w))
    medians = {name: round(float(np.median(stage_ms[:, k])), 4) for k, name in enumerate(STAGES)}
    res = {"operations": num_ops, "rows": rows, "degree_bits": degree_bits, "trace_bytes": mt.NUM_COLUMNS * 8 * n, "ops_bytes": int(w.nbytes),
           "stage_median_ms": medians, "gaps_and_rows_median_ms": round(medians["gaps"] + medians["rows"], 4),
           "stages_sum_median_ms": round(float(np.median(stage_ms.sum(axis=1))), 4), "dominant_stage": max(medians, key=medians.get),
           "call": stats(call_ms), "count_only_call": stats(count_ms), "upload_finished_trace": stats(upload_ms), "upload_operations": stats(ops_upload_ms)}
    res["upload_over_call"] = round(res["upload_finished_trace"]["median_ms"] / res["call"]["median_ms"], 2)
    for b in (d_ops, scratch, d_trace):
        b.free()
    return res


def measure_prove(ctx, bits, reps):
    d_ops = pg.DeviceBuffer.from_host(ctx, ops_for(bits))
    d_trace = mt.generate_trace(ctx, d_ops)
    degree_bits = (d_trace.n // mt.NUM_COLUMNS).bit_length() - 1
    desc = mt.stark_desc(degree_bits, 2, fast_config_fri_params(degree_bits))
    ns = pg.NativeStark(ctx, desc)
    first = ns.prove_bytes(d_trace, [])
    ns.prove_bytes(d_trace, [])
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        data = ns.prove_bytes(d_trace, [])
        ms.append((time.perf_counter() - t0) * 1e3)
        if data != first:
            raise SystemExit("bench_memory_table: the proof is not deterministic")
    timing = {}
    ns.prove_bytes(d_trace, [], timing)
    ns.close()
    d_trace.free(), d_ops.free()
    return dict(stats(ms), operations=1 << bits, rows=d_trace.rows, degree_bits=degree_bits, proof_bytes=len(first),
                stage_ms={k: round(v, 3) for k, v in timing.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[16, 18, 20, 22])
    ap.add_argument("--prove-bits", type=int, nargs="*", default=[16, 18, 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memory_table.json"))
    a = ap.parse_args()
    if a.reps < 5 or not all(4 <= b <= 22 for b in a.bits + a.prove_bits):
        ap.error("--reps >= 5; 2^4 .. 2^22 operations (the trace of 2^22 operations has 2^23 rows, the most a STARK of rate 2 takes)")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_memory_table.py", "device": a.device, "library": _lib.load().gl_version().decode(), "reps": a.reps,
           "columns": mt.NUM_COLUMNS, "operations_shape": "5 contexts, segments < 32, 64 address clusters of 1024 words, timestamps rising in list order",
           "prove_config": "MemoryStark: 26 columns, degree 3, 2 permutation pairs, interpreted program, Poseidon, standard_fast_config (2 challenges, "
                           "rate_bits 1, cap_height 4, 16 PoW bits, arity 4 down to 2^5, 84 queries); trace built on the device and resident",
           "trace": {}, "prove": {}}
    for bits in sorted(a.bits):
        res["trace"]["2^%d" % bits] = measure_trace(ctx, bits, a.reps)
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
