#!/usr/bin/env python3
"""The arithmetic table (plonky2_gpu_amd/arithmetic_table.py, csrc/arithmetic_table.hip): its trace built on the device, against a
memset of the same bytes and against the upload it replaces, and whole proofs of it. Per size and per mix of operators:

  stages      gl_debug_arithmetic_table_stage_ms: the counting pass (validation, row counts, their scan) and the fill (one lane
              per operation, one lane per zero row), by events on the context's stream, warm, median of --reps runs
  memset      gl_memset_zero of the same 92 * 8 * n bytes, by events, in the same rounds; the fill's share of its rate stands beside
              the logic table's share at the same height (profiles/logic_table.json, rows_8_bytes_per_lane)
  call        gl_arithmetic_table_trace by the wall clock with the wait for the stream: count, its one host wait, the fill
  upload      a finished 92-column trace of the same height from pageable host memory into the same buffer, by the wall clock:
              what the host route pays AFTER it has generated the trace. THE CONDITION: the call is faster, at every size and mix.

The mixes fill the n rows as far as their row counts allow: "add" n ADDs; "mulmod" n / 2 MULMODs (a 512-by-256-bit division each);
"mixed" all ten operators in turn, 2 n / 3 operations. Operands are random 256-bit words. mulmod_over_add_per_operation says what
the modular path costs. `prove`: gl_stark_prove of the device-built mixed trace at constraint_degree 5 under starky's
standard_fast_config with rate_bits 2, interpreted against compiled in units, the calls of the two handles alternating; the bytes
must be equal, and tests/stark_verify.py must accept them at the smallest size. One JSON line on stdout and in --out (default
profiles/arithmetic_table.json).

  python tools/bench_arithmetic_table.py [--bits 16 18 20] [--prove-bits 12 16] [--reps 7] [--device LABEL] [--out FILE]"""
import argparse
import ctypes
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
from plonky2_gpu_amd import arithmetic_table as at

MIXES = ("add", "mulmod", "mixed")
ORDER = (at.OP_ADD, at.OP_MULMOD, at.OP_LT, at.OP_DIV, at.OP_MUL, at.OP_SUBMOD, at.OP_SUB, at.OP_MOD, at.OP_GT, at.OP_ADDMOD)


def ops_for(bits, mix):
    """[num_ops][25] records that fill 2^bits rows as far as the mix's row counts allow"""
    n = 1 << bits
    num_ops = {"add": n, "mulmod": n // 2, "mixed": (2 * n // 3) // 10 * 10}[mix]
    rng = np.random.default_rng(bits)
    w = rng.integers(0, 1 << 32, size=(num_ops, at.OP_WORDS), dtype=np.uint64)
    op = {"add": np.full(num_ops, at.OP_ADD), "mulmod": np.full(num_ops, at.OP_MULMOD), "mixed": np.array(ORDER)[np.arange(num_ops) % 10]}[mix]
    w[:, 0] = op
    w[np.isin(op, at.ONE_ROW_OPS), 17:25] = 0
    w[np.isin(op, (at.OP_DIV, at.OP_MOD)), 9:17] = 0
    return w


def measure_trace(ctx, bits, mix, reps, logic_share):
    n = 1 << bits
    w = ops_for(bits, mix)
    num_ops = w.shape[0]
    d_ops = pg.DeviceBuffer.from_host(ctx, w)
    d_trace = pg.DeviceBuffer(ctx, at.NUM_COLUMNS * n)
    scratch = pg.DeviceBuffer(ctx, _lib.load().gl_arithmetic_table_scratch_bytes(num_ops, bits) // 8)
    nbytes = at.NUM_COLUMNS * 8 * n
    e0, e1 = pg.Event(), pg.Event()
    stage = np.zeros(2, dtype=np.float32)
    count_ms, fill_ms, memset_ms, wall = [], [], [], []
    rows = ctypes.c_uint64()
    for rep in range(reps + 2):
        _lib.call("gl_debug_arithmetic_table_stage_ms", d_ops.ptr, num_ops, bits, d_trace.ptr, n, scratch.ptr, stage.ctypes.data, ctx.ptr)
        ctx.synchronize()
        e0.record(ctx)
        _lib.call("gl_memset_zero", d_trace.ptr, nbytes, ctx.ptr)
        e1.record(ctx)
        ctx.synchronize()
        memset = e1.elapsed_ms_since(e0)
        t0 = time.perf_counter()
        _lib.call("gl_arithmetic_table_trace", d_ops.ptr, num_ops, bits, d_trace.ptr, n, scratch.ptr, ctypes.byref(rows), ctx.ptr)
        ctx.synchronize()
        if rep >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
            count_ms.append(float(stage[0])), fill_ms.append(float(stage[1])), memset_ms.append(memset)
    fill, ms0 = float(np.median(fill_ms)), float(np.median(memset_ms))
    res = {"rows": n, "operations": num_ops, "rows_taken": int(rows.value), "bytes": nbytes, "count_stage": stats(count_ms),
           "fill": dict(stats(fill_ms), tb_per_s=round(nbytes / fill / 1e9, 3), fraction_of_memset=round(ms0 / fill, 4),
                        ns_per_operation=round(fill * 1e6 / num_ops, 3)),
           "memset_same_bytes": dict(stats(memset_ms), tb_per_s=round(nbytes / ms0 / 1e9, 3)), "call_wall": stats(wall)}
    if logic_share is not None:
        res["fill"]["logic_table_fraction_of_memset_at_this_height"] = logic_share
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
    res["call_faster_than_upload"] = bool(np.median(wall) < np.median(up))
    del host
    d_ops.free(), d_trace.free(), scratch.free()
    return res


def measure_prove(ctx, bits, reps, verify):
    """interpreted against compiled in units, alternating, inside a TemporaryKernelCache: the first size carries the cold compile"""
    desc = at.stark_desc(bits, 2, dict(fast_config_fri_params(bits), rate_bits=2))
    d_trace = at.generate_trace(ctx, ops_for(bits, "mixed"), bits)
    interpreted, compiled = pg.NativeStark(ctx, desc), pg.NativeStark(ctx, desc)
    t0 = time.perf_counter()
    compiled.compile(unit_instrs=0)
    compile_ms = round((time.perf_counter() - t0) * 1e3, 1)
    handles = {"interpreted": interpreted, "compiled": compiled}
    first = interpreted.prove_bytes(d_trace, [])
    if compiled.prove_bytes(d_trace, []) != first:
        raise SystemExit("bench_arithmetic_table: at 2^%d rows the proof compiled in units differs from the interpreted one" % bits)
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
                raise SystemExit("bench_arithmetic_table: the bytes changed between two calls")
    res = {"rows": 1 << bits, "rows_taken": d_trace.rows, "units": compiled.num_units, "compile_ms": compile_ms, "proof_bytes": len(first),
           "bytes_equal": True, "program_instructions": int(desc.instrs.shape[0])}
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
            raise SystemExit("bench_arithmetic_table: the reference verifier rejects the proof at 2^%d rows" % bits)
        res["reference_verifier_accepts"] = True
    return res


def logic_shares():
    """{bits: the logic table's fill as a fraction of the memset rate} from profiles/logic_table.json, where it is there"""
    try:
        with open(os.path.join(ROOT, "profiles", "logic_table.json")) as f:
            trace = json.load(f)["trace"]
        return {int(k[2:]): v["rows_8_bytes_per_lane"]["fraction_of_memset"] for k, v in trace.items()}
    except (OSError, KeyError, ValueError):
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="*", default=[16, 18, 20])
    ap.add_argument("--prove-bits", type=int, nargs="*", default=[12, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arithmetic_table.json"))
    a = ap.parse_args()
    if a.reps < 5 or not all(5 <= b <= 22 for b in a.bits + a.prove_bits):
        ap.error("--reps >= 5; sizes in 2^5 .. 2^22 rows")
    ctx = pg.Context(0)
    shares = logic_shares()
    res = {"tool": "tools/bench_arithmetic_table.py", "device": a.device, "library": _lib.load().gl_version().decode(), "reps": a.reps,
           "columns": at.NUM_COLUMNS, "condition": "call_wall median below upload_of_the_finished_trace median at every size and mix",
           "prove_config": "ArithmeticStark: 92 columns, 246 constraints, declared degree 5, Poseidon, standard_fast_config with rate_bits 2 "
                           "(2 challenges, cap_height 4, 16 PoW bits, arity 4 down to 2^5, 84 queries); the mixed trace built on the device and "
                           "resident; compiled in units at the library's cap",
           "trace": {}, "prove": {}}
    for bits in sorted(a.bits):
        per_mix = {mix: measure_trace(ctx, bits, mix, a.reps, shares.get(bits)) for mix in MIXES}
        per_mix["mulmod_over_add_per_operation"] = round(per_mix["mulmod"]["fill"]["ns_per_operation"] / per_mix["add"]["fill"]["ns_per_operation"], 2)
        res["trace"]["2^%d" % bits] = per_mix
        print("2^%d" % bits, json.dumps(per_mix), file=sys.stderr, flush=True)
    res["condition_met"] = all(res["trace"][k][mix]["call_faster_than_upload"] for k in res["trace"] for mix in MIXES)
    with TemporaryKernelCache("arithmetic_table"):
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
