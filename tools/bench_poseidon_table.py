#!/usr/bin/env python3
"""The Poseidon table (plonky2_gpu_amd/poseidon_table.py, csrc/poseidon_table.hip): its trace built on the device, against a memset
of the same bytes, against gl_poseidon_permute_batch on as many states and against the upload it replaces, and whole proofs of
it. Nobody had measured this kernel — 1 992 bytes of stores per row against a whole permutation of arithmetic — so there is no
target figure: the yardsticks are the memset rate and the permutation rate measured in the same rounds. Per size and per list:

  stages      gl_debug_poseidon_table_stage_ms: the validation, the serial pass (not run for a list without an ABSORB) and the
              rows kernel, by events on the context's stream, warm, median of --reps runs
  memset      gl_memset_zero of the same 249 * 8 * n bytes, by events, in the same rounds: rows.fraction_of_memset
  permute     gl_poseidon_permute_batch on n states in place, by events, in the same rounds: rows.fraction_of_permute_rate
  call        gl_poseidon_table_trace by the wall clock with the wait for the stream: validation, its one host wait, the fill
  upload      a finished 249-column trace of the same height from pageable host memory into the same buffer, by the wall clock:
              what the host route pays AFTER it has generated the trace
  mds         the rows kernel with its MDS layers on the matrix cores and on the vector ALU, on the all-START list, alternating

The lists fill all n rows: "starts" n STARTs; "leaves135" runs of 17 rows, the sponge of a 135-element leaf; "one_run" one run as
long as the list — as far as --max-run-seconds allows: a run is walked by ONE lane, its time is linear in its length, and a
kernel that runs for many seconds does not belong on a machine others use. The tool measures a run of 2^12 rows first and cuts
longer runs to the largest power of two whose projected time stays within the limit (the list is then several such runs, which
lanes walk side by side); serial_us_per_row and the projection for a run of n rows are recorded either way.
`prove`: gl_stark_prove of the device-built leaves135 trace under starky's standard_fast_config, interpreted against compiled in
units, the calls of the two handles alternating; the bytes must be equal, and tests/stark_verify.py must accept them at the
smallest size. One JSON line on stdout and in --out (default profiles/poseidon_table.json).

  python tools/bench_poseidon_table.py [--bits 16 18 20] [--prove-bits 12 16] [--reps 7] [--max-run-seconds 1.5] [--device LABEL] [--out FILE]"""
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
from plonky2_gpu_amd import poseidon_table as pt

LISTS = ("starts", "leaves135", "one_run")
MDS = {"matrix_cores": 1, "vector_alu": 2}
P = 0xFFFFFFFF00000001
# the whole program as ONE unit: the permutation's state runs through all 237 constraints, every unit re-derives it from the
# columns, and at the library's cap split_program makes 58 units of up to 3 800 instructions whose cold compile takes minutes
UNIT_INSTRS = 8192


def ops_for(bits, name, run_rows=None):
    """[2^bits][13] records: random canonical elements; the kinds make STARTs, 17-row runs (16 ABSORBs, the last of 7 elements)
    or runs of run_rows rows (ABSORBs of 8)"""
    n = 1 << bits
    w = np.random.default_rng(bits).integers(0, P, size=(n, pt.OP_WORDS), dtype=np.uint64)
    at = np.arange(n)
    if name == "starts":
        w[:, 0] = 0
    elif name == "leaves135":
        w[:, 0] = np.where(at % 17 == 0, 0, np.where(at % 17 == 16, 7, 8))
    else:
        w[:, 0] = np.where(at % run_rows == 0, 0, 8)
    return w


def stage_ms(ctx, d_ops, n_ops, bits, d_trace, scratch, mds=0):
    ms = np.zeros(3, dtype=np.float32)
    _lib.call("gl_debug_poseidon_table_stage_ms", d_ops.ptr, n_ops, bits, d_trace.ptr, 1 << bits, scratch.ptr, mds, ms.ctypes.data, ctx.ptr)
    return [float(v) for v in ms]


def serial_us_per_row(ctx):
    """the serial pass on one run of 2^12 rows: what one lane takes per row of a run"""
    bits = 12
    d_ops = pg.DeviceBuffer.from_host(ctx, ops_for(bits, "one_run", 1 << bits))
    d_trace, scratch = pg.DeviceBuffer(ctx, pt.NUM_COLUMNS << bits), pg.DeviceBuffer(ctx, 2)
    ms = [stage_ms(ctx, d_ops, 1 << bits, bits, d_trace, scratch)[1] for _ in range(4)][1:]
    d_ops.free(), d_trace.free(), scratch.free()
    return float(np.median(ms)) * 1e3 / ((1 << bits) - 1)


def measure_trace(ctx, bits, name, reps, run_rows):
    n = 1 << bits
    w = ops_for(bits, name, run_rows)
    d_ops = pg.DeviceBuffer.from_host(ctx, w)
    d_trace = pg.DeviceBuffer(ctx, pt.NUM_COLUMNS * n)
    d_states = pg.DeviceBuffer.from_host(ctx, np.ascontiguousarray(w[:, 1:]))
    scratch = pg.DeviceBuffer(ctx, 2)
    nbytes = pt.NUM_COLUMNS * 8 * n
    e0, e1, e2 = pg.Event(), pg.Event(), pg.Event()
    stages, memset_ms, permute_ms, wall = [], [], [], []
    for rep in range(reps + 2):
        stage = stage_ms(ctx, d_ops, n, bits, d_trace, scratch)
        ctx.synchronize()
        e0.record(ctx)
        _lib.call("gl_memset_zero", d_trace.ptr, nbytes, ctx.ptr)
        e1.record(ctx)
        _lib.call("gl_poseidon_permute_batch", d_states.ptr, n, ctx.ptr)
        e2.record(ctx)
        ctx.synchronize()
        t0 = time.perf_counter()
        _lib.call("gl_poseidon_table_trace", d_ops.ptr, n, bits, d_trace.ptr, n, scratch.ptr, ctx.ptr)
        ctx.synchronize()
        if rep >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(stage), memset_ms.append(e1.elapsed_ms_since(e0)), permute_ms.append(e2.elapsed_ms_since(e1))
    validation, serial, rows = ([s[k] for s in stages] for k in range(3))
    rows_ms, ms0, perm = float(np.median(rows)), float(np.median(memset_ms)), float(np.median(permute_ms))
    res = {"rows": n, "bytes": nbytes, "validation": stats(validation),
           "serial_pass": dict(stats(serial), us_per_row=round(float(np.median(serial)) * 1e3 / n, 4)) if min(serial) >= 0 else "not run",
           "rows_kernel": dict(stats(rows), tb_per_s=round(nbytes / rows_ms / 1e9, 3), g_rows_per_s=round(n / rows_ms / 1e6, 3),
                               fraction_of_memset=round(ms0 / rows_ms, 4), fraction_of_permute_rate=round(perm / rows_ms, 4)),
           "memset_same_bytes": dict(stats(memset_ms), tb_per_s=round(nbytes / ms0 / 1e9, 3)),
           "permute_batch_as_many_states": dict(stats(permute_ms), g_permutations_per_s=round(n / perm / 1e6, 3)), "call_wall": stats(wall)}
    if name == "one_run":
        res["run_rows"] = run_rows
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
    for b in (d_ops, d_trace, d_states, scratch):
        b.free()
    return res


def measure_mds(ctx, bits, reps):
    """the rows kernel of the all-START list with either MDS layer, alternating"""
    n = 1 << bits
    d_ops = pg.DeviceBuffer.from_host(ctx, ops_for(bits, "starts"))
    d_trace, scratch = pg.DeviceBuffer(ctx, pt.NUM_COLUMNS * n), pg.DeviceBuffer(ctx, 2)
    ms = {k: [] for k in MDS}
    for rep in range(reps + 2):
        for k, variant in MDS.items():
            rows = stage_ms(ctx, d_ops, n, bits, d_trace, scratch, variant)[2]
            if rep >= 2:
                ms[k].append(rows)
    d_ops.free(), d_trace.free(), scratch.free()
    res = {k: stats(v) for k, v in ms.items()}
    res["vector_alu_over_matrix_cores"] = round(res["vector_alu"]["median_ms"] / res["matrix_cores"]["median_ms"], 4)
    return res


def measure_prove(ctx, bits, reps, verify):
    """interpreted against compiled in units, alternating, inside a TemporaryKernelCache: the first size carries the cold compile"""
    desc = pt.stark_desc(bits, 2, fast_config_fri_params(bits))
    d_trace = pt.generate_trace(ctx, ops_for(bits, "leaves135"), bits)
    interpreted, compiled = pg.NativeStark(ctx, desc), pg.NativeStark(ctx, desc)
    t0 = time.perf_counter()
    compiled.compile(unit_instrs=UNIT_INSTRS)
    compile_ms = round((time.perf_counter() - t0) * 1e3, 1)
    handles = {"interpreted": interpreted, "compiled": compiled}
    first = interpreted.prove_bytes(d_trace, [])
    if compiled.prove_bytes(d_trace, []) != first:
        raise SystemExit("bench_poseidon_table: at 2^%d rows the proof compiled in units differs from the interpreted one" % bits)
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
                raise SystemExit("bench_poseidon_table: the bytes changed between two calls")
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
            raise SystemExit("bench_poseidon_table: the reference verifier rejects the proof at 2^%d rows" % bits)
        res["reference_verifier_accepts"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="*", default=[16, 18, 20])
    ap.add_argument("--prove-bits", type=int, nargs="*", default=[12, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-run-seconds", type=float, default=1.5, help="the longest serial pass the one_run list may take")
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_table.json"))
    a = ap.parse_args()
    if a.reps < 5 or not all(5 <= b <= 22 for b in a.bits + a.prove_bits) or not 0 < a.max_run_seconds <= 5:
        ap.error("--reps >= 5; sizes in 2^5 .. 2^22 rows; --max-run-seconds in (0, 5]")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_poseidon_table.py", "device": a.device, "library": _lib.load().gl_version().decode(), "reps": a.reps,
           "columns": pt.NUM_COLUMNS, "row_bytes": pt.NUM_COLUMNS * 8,
           "yardsticks": "rows_kernel.fraction_of_memset = memset time / rows kernel time, rows_kernel.fraction_of_permute_rate = "
                         "gl_poseidon_permute_batch time on as many states / rows kernel time, all three measured in the same rounds",
           "prove_config": "the permutation unit: 249 columns, 237 constraints, degree 3, Poseidon, standard_fast_config (2 challenges, "
                           "rate_bits 1, cap_height 4, 16 PoW bits, arity 4 down to 2^5, 84 queries); the leaves135 trace built on the "
                           "device and resident; compiled as one unit (unit_instrs 8192)",
           "trace": {}, "mds": {}, "prove": {}}
    per_row = serial_us_per_row(ctx)
    longest = 1 << int(np.floor(np.log2(a.max_run_seconds * 1e6 / per_row)))
    res["serial_pass_one_lane"] = {"us_per_row": round(per_row, 3), "measured_on_a_run_of_rows": 1 << 12, "max_run_seconds": a.max_run_seconds,
                                   "longest_run_measured": longest,
                                   "projected_ms_for_one_run_of": {"2^%d" % b: round(per_row * (1 << b) / 1e3, 1) for b in sorted(a.bits)}}
    print("serial", json.dumps(res["serial_pass_one_lane"]), file=sys.stderr, flush=True)
    for bits in sorted(a.bits):
        key = "2^%d" % bits
        res["trace"][key] = {name: measure_trace(ctx, bits, name, a.reps, min(1 << bits, longest)) for name in LISTS}
        res["mds"][key] = measure_mds(ctx, bits, a.reps)
        print(key, json.dumps(res["trace"][key]), json.dumps(res["mds"][key]), file=sys.stderr, flush=True)
    with TemporaryKernelCache("poseidon_table"):
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
