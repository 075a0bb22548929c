#!/usr/bin/env python3
"""The logic table (plonky2_gpu_amd/logic_table.py, csrc/logic_table.hip): its trace built on the device, against the store floor
of its 523 columns, against the Keccak-f table's trace kernel and against the upload it replaces, and whole proofs of it. Per size:

  rows        gl_debug_logic_table_fill at both store widths — one row per thread (8 bytes per lane and column store) and two
              adjacent rows per thread (16 bytes per lane) —, the calls of the two alternating, timed by events on the context's
              stream, warm, median of --reps runs: milliseconds, 523 * 8 * n bytes / time, that as a fraction of the 8 TB/s
              specification and as a fraction of gl_memset_zero of the same buffer. The two widths' traces must be equal (compared up to
              --upload-max-bits). Beside them the same kernels with no operation at all (every row padding: the stores alone, no
              record is loaded): the difference is what the strided record loads cost.
  call        gl_logic_table_trace by the wall clock with the wait for the stream: validation, its one host wait, the rows
  keccak      gl_keccak_table_trace at the nearest equal byte count (2430 * 8 * n / 4 bytes against 523 * 8 * n: 1.16 times as
              many) with the memset of ITS buffer, in the same run: the yardstick is its fraction of the memset rate
  upload      a finished 523-column trace of the same height from pageable host memory into the same buffer, by the wall clock:
              what the host route pays after it has generated the trace (up to --upload-max-bits)
  prove       gl_stark_prove of the device-built trace under starky's standard_fast_config, interpreted against compiled in
              units (gl_stark_compile_units at the library's cap), the calls of the two handles alternating; the bytes must be
              equal, and the reference verifier of tests/stark_verify.py must accept them at the smallest size

n rows hold n operations of all three operators on random words (no padding: every row loads its record). One JSON line on stdout
and in --out (default profiles/logic_table.json).

  python tools/bench_logic_table.py [--bits 14 16 18 20] [--prove-bits 12 14 16] [--reps 7] [--device LABEL] [--out FILE]"""
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
from bench_common import TemporaryKernelCache, fast_config_fri_params, stats
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd import keccak_table as kt
from plonky2_gpu_amd import logic_table as lt

SPEC_BYTES_PER_S = 8e12  # the 8 TB/s of the MI355X's specification


def ops_for(bits):
    """[2^bits][17] records: all three operators on random 256-bit words"""
    n = 1 << bits
    rng = np.random.default_rng(bits)
    w = rng.integers(0, 1 << 32, size=(n, lt.OP_WORDS), dtype=np.uint64)
    w[:, 0] = rng.integers(0, 3, n)
    return w


def timed_alternating(ctx, reps, calls):
    """{name: [ms]} of the calls in `calls`, one after the other in every round, two warm-up rounds first"""
    e0, e1 = pg.Event(), pg.Event()
    ms = {k: [] for k in calls}
    for rep in range(reps + 2):
        for k, call in calls.items():
            ctx.synchronize()
            e0.record(ctx)
            call()
            e1.record(ctx)
            ctx.synchronize()
            if rep >= 2:
                ms[k].append(e1.elapsed_ms_since(e0))
    return ms


def rate(nbytes, ms, memset_ms):
    med = float(np.median(ms))
    return dict(stats(ms), tb_per_s=round(nbytes / med / 1e9, 3), fraction_of_8_tb_per_s=round(nbytes / (med * 1e-3) / SPEC_BYTES_PER_S, 4),
                fraction_of_memset=round(float(np.median(memset_ms)) / med, 4))


def measure_trace(ctx, bits, reps, upload):
    n = 1 << bits
    w = ops_for(bits)
    d_ops = pg.DeviceBuffer.from_host(ctx, w)
    d_trace = pg.DeviceBuffer(ctx, lt.NUM_COLUMNS * n)
    scratch = pg.DeviceBuffer(ctx, 2)
    nbytes = lt.NUM_COLUMNS * 8 * n
    fill = lambda width: _lib.call("gl_debug_logic_table_fill", d_ops.ptr, n, bits, d_trace.ptr, n, width, ctx.ptr)  # noqa: E731
    no_loads = lambda width: _lib.call("gl_debug_logic_table_fill", None, 0, bits, d_trace.ptr, n, width, ctx.ptr)  # noqa: E731
    ms = timed_alternating(ctx, reps, {"8": lambda: fill(1), "16": lambda: fill(2), "8 padding": lambda: no_loads(1), "16 padding": lambda: no_loads(2),
                                       "memset": lambda: _lib.call("gl_memset_zero", d_trace.ptr, nbytes, ctx.ptr)})
    res = {"rows": n, "bytes": nbytes, "memset_same_buffer": dict(stats(ms["memset"]), tb_per_s=round(nbytes / float(np.median(ms["memset"])) / 1e9, 3)),
           "rows_8_bytes_per_lane": rate(nbytes, ms["8"], ms["memset"]), "rows_16_bytes_per_lane": rate(nbytes, ms["16"], ms["memset"]),
           "all_padding_8_bytes_per_lane": rate(nbytes, ms["8 padding"], ms["memset"]),
           "all_padding_16_bytes_per_lane": rate(nbytes, ms["16 padding"], ms["memset"])}
    res["record_loads_share_of_8_byte_rows"] = round(1 - res["all_padding_8_bytes_per_lane"]["median_ms"] / res["rows_8_bytes_per_lane"]["median_ms"], 4)
    res["16_over_8"] = round(res["rows_8_bytes_per_lane"]["median_ms"] / res["rows_16_bytes_per_lane"]["median_ms"], 4)
    if upload:  # the two widths write the same trace (compared in slabs of columns, on the host; at the sizes the upload is timed at)
        slab = max(1, (1 << 24) // n)
        other = pg.DeviceBuffer(ctx, lt.NUM_COLUMNS * n)
        fill(1)
        _lib.call("gl_debug_logic_table_fill", d_ops.ptr, n, bits, other.ptr, n, 2, ctx.ptr)
        ctx.synchronize()
        for c0 in range(0, lt.NUM_COLUMNS, slab):
            count = min(slab, lt.NUM_COLUMNS - c0) * n
            if not (d_trace.download(c0 * n, count) == other.download(c0 * n, count)).all():
                raise SystemExit("bench_logic_table: the two store widths differ at 2^%d rows" % bits)
        other.free()
        res["widths_equal"] = True
    # the product call, by the wall clock: validation, the host's wait, the rows
    wall = []
    for rep in range(reps + 2):
        ctx.synchronize()
        t0 = time.perf_counter()
        _lib.call("gl_logic_table_trace", d_ops.ptr, n, bits, d_trace.ptr, n, scratch.ptr, ctx.ptr)
        ctx.synchronize()
        if rep >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
    res["call_wall"] = stats(wall)
    # the Keccak-f table's kernel at the nearest equal byte count, with the memset of its buffer
    kbits = bits - 2
    kn, kbytes = 1 << kbits, kt.NUM_COLUMNS * 8 << kbits
    inputs = np.random.default_rng(kbits).integers(0, 1 << 64, size=(kn // 24, 25), dtype=np.uint64)
    d_in, d_kt = pg.DeviceBuffer.from_host(ctx, inputs), pg.DeviceBuffer(ctx, kt.NUM_COLUMNS * kn)
    kms = timed_alternating(ctx, reps, {"keccak": lambda: _lib.call("gl_keccak_table_trace", d_in.ptr, inputs.shape[0], kbits, d_kt.ptr, kn, ctx.ptr),
                                        "memset": lambda: _lib.call("gl_memset_zero", d_kt.ptr, kbytes, ctx.ptr)})
    res["keccak_table_kernel"] = dict(rate(kbytes, kms["keccak"], kms["memset"]), rows=kn, bytes=kbytes, bytes_over_logic=round(kbytes / nbytes, 3),
                                      memset_tb_per_s=round(kbytes / float(np.median(kms["memset"])) / 1e9, 3))
    d_in.free(), d_kt.free()
    for key in ("rows_8_bytes_per_lane", "rows_16_bytes_per_lane"):
        res[key]["points_of_memset_above_keccak_kernel"] = round(100 * (res[key]["fraction_of_memset"] - res["keccak_table_kernel"]["fraction_of_memset"]), 2)
    if upload:
        host = d_trace.download()  # a finished trace, in pageable host memory
        up = []
        for rep in range(5):
            ctx.synchronize()
            t0 = time.perf_counter()
            d_trace.upload(host)
            ctx.synchronize()
            if rep >= 2:
                up.append((time.perf_counter() - t0) * 1e3)
        res["upload_of_the_finished_trace"] = dict(stats(up), gb_per_s=round(nbytes / float(np.median(up)) / 1e6, 2),
                                                   over_call=round(float(np.median(up)) / float(np.median(wall)), 1))
        del host
    d_ops.free(), d_trace.free(), scratch.free()
    return res


def measure_prove(ctx, bits, reps, verify):
    """interpreted against compiled in units, alternating, inside a TemporaryKernelCache: the first size carries the cold compile"""
    desc = lt.stark_desc(bits, 2, fast_config_fri_params(bits))
    d_trace = lt.generate_trace(ctx, ops_for(bits), bits)
    interpreted, compiled = pg.NativeStark(ctx, desc), pg.NativeStark(ctx, desc)
    t0 = time.perf_counter()
    compiled.compile(unit_instrs=0)
    compile_ms = round((time.perf_counter() - t0) * 1e3, 1)
    handles = {"interpreted": interpreted, "compiled": compiled}
    first = interpreted.prove_bytes(d_trace, [])
    if compiled.prove_bytes(d_trace, []) != first:
        raise SystemExit("bench_logic_table: at 2^%d rows the proof compiled in units differs from the interpreted one" % bits)
    ms, quotient, stages = {k: [] for k in handles}, {k: [] for k in handles}, {}
    for _ in range(reps):
        for k, ns in handles.items():
            timing = {}
            t0 = time.perf_counter()
            data = ns.prove_bytes(d_trace, [], timing)
            ms[k].append((time.perf_counter() - t0) * 1e3)
            quotient[k].append(timing["quotient polys"])
            stages[k] = {name: round(v, 3) for name, v in timing.items()}
            if data != first:
                raise SystemExit("bench_logic_table: the bytes changed between two calls")
    res = {"rows": 1 << bits, "units": compiled.num_units, "compile_ms": compile_ms, "proof_bytes": len(first), "bytes_equal": True,
           "program_instructions": int(desc.instrs.shape[0])}
    for k in handles:
        res[k] = {"proof": stats(ms[k]), "quotient_stage": stats(quotient[k]), "stage_ms": stages[k]}
    res["quotient_interpreted_over_compiled"] = round(res["interpreted"]["quotient_stage"]["median_ms"] / res["compiled"]["quotient_stage"]["median_ms"], 3)
    res["proof_interpreted_over_compiled"] = round(res["interpreted"]["proof"]["median_ms"] / res["compiled"]["proof"]["median_ms"], 3)
    for ns in handles.values():
        ns.close()
    d_trace.free()
    if verify:
        import stark_verify

        if not stark_verify.accepts(desc, first):
            raise SystemExit("bench_logic_table: the reference verifier rejects the proof at 2^%d rows" % bits)
        res["reference_verifier_accepts"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="*", default=[14, 16, 18, 20])
    ap.add_argument("--prove-bits", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--upload-max-bits", type=int, default=18, help="the upload is timed up to this size (2^18 rows are 1.1 GB of host memory)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logic_table.json"))
    a = ap.parse_args()
    if a.reps < 5 or not all(5 <= b <= 20 for b in a.bits + a.prove_bits):
        ap.error("--reps >= 5; sizes in 2^5 .. 2^20 rows (a trace at 2^20 rows is 4.4 GB)")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_logic_table.py", "device": a.device, "library": _lib.load().gl_version().decode(), "reps": a.reps,
           "columns": lt.NUM_COLUMNS, "store_floor": "523 * 8 * n bytes against 8 TB/s",
           "yardstick": "the Keccak-f table's trace kernel at the nearest equal byte count in the same run: its fraction of the memset rate of "
                        "its buffer, less 5 points",
           "prove_config": "LogicStark: 523 columns, 520 constraints of degree 3, Poseidon, standard_fast_config (2 challenges, rate_bits 1, "
                           "cap_height 4, 16 PoW bits, arity 4 down to 2^5, 84 queries); trace built on the device and resident; compiled in units "
                           "at the library's cap",
           "trace": {}, "prove": {}}
    for bits in sorted(a.bits):
        res["trace"]["2^%d" % bits] = measure_trace(ctx, bits, a.reps, bits <= a.upload_max_bits)
        print("2^%d" % bits, json.dumps(res["trace"]["2^%d" % bits]), file=sys.stderr, flush=True)
    with TemporaryKernelCache("logic_table"):
        for k, bits in enumerate(sorted(a.prove_bits)):
            res["prove"]["2^%d" % bits] = measure_prove(ctx, bits, a.reps, verify=k == 0)
            print("prove 2^%d" % bits, json.dumps(res["prove"]["2^%d" % bits]), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
