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

--compiled proves the table INTERPRETED and COMPILED IN UNITS (gl_stark_compile_units, csrc/stark_jit.hip) in one run, the calls of
the two handles alternating, at the sizes of --prove-bits: per size the quotient stage and the whole proof of both with median and
min - max, the number of units, and the cold (empty temporary kernel cache) and warm compile wall time. It exits non-zero unless
the compiled proof's bytes equal the interpreted one's at every size and the reference verifier of tests/stark_ref.py accepts
them. --caps adds, per cap, the cold compile time and the quotient stage at every size (the curves the library's default cap
was read from); --precompile-caps measures only the cold gl_stark_precompile_units per cap, each in a process of its own, and
needs no device (--precompile-program fuzz4000: of the 4 000-instruction program of tests/stark_fuzz.py, cap -1 its single kernel). Both write
--compiled-out (default profiles/keccak_table_compiled.json), --precompile-caps under the key the --host label names.

Without --compiled oracle-free; the reference verifier accepts the proofs of `prove` at 2^12 and 2^14 rows in tests/test_gpu_stark_scale.py, which takes
inputs_for and the parameters from here. One JSON line on stdout and in --out (default profiles/keccak_table.json).

  python tools/bench_keccak_table.py [--bits 14 16 18 20] [--prove-bits 12 14] [--reps 7] [--device LABEL] [--out FILE]
  python tools/bench_keccak_table.py --compiled [--unit-instrs N] [--caps 250 500 1000 2000 4000] [--prove-bits 12 14]
  python tools/bench_keccak_table.py --precompile-caps 250 500 1000 2000 4000 --host LABEL
  python tools/bench_keccak_table.py --precompile-program fuzz4000 --precompile-caps -1 0 --host LABEL"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import plonky2_gpu_amd as pg
from bench_common import TemporaryKernelCache, fast_config_fri_params, stats
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd import keccak_table as kt

SPEC_BYTES_PER_S = 8e12  # the 8 TB/s of the MI355X's specification


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


def _precompile_desc(which):
    if which == "keccak":
        return kt.stark_desc(12, 2, fast_config_fri_params(12))
    import bench_stark_prove as bsp  # the 4 000-instruction program of tests/stark_fuzz.py

    return bsp.fuzz4000_desc(12)


def precompile_child(which, cap):
    """in a process of its own: one cold precompile (cap < 0: the single kernel) into an empty kernel cache; prints one JSON line"""
    from plonky2_gpu_amd import stark as pstark

    desc = _precompile_desc(which)
    cache = os.environ["PLONKY2_HIP_KERNEL_CACHE"]
    t0 = time.perf_counter()
    pstark.precompile(desc, unit_instrs=None if cap < 0 else cap)
    print(json.dumps({"cold_s": round(time.perf_counter() - t0, 2), "units": len([f for f in os.listdir(cache) if f.endswith(".hsaco")]),
                      "instructions": int(desc.instrs.shape[0])}))


def measure_precompile(which, caps):
    """Cold gl_stark_precompile_units per cap (-1: gl_stark_precompile, the single kernel): wall seconds and the code objects
    written. Every cap in a fresh process with an empty kernel cache and an empty cache directory of the compiler library's own —
    units that two caps have in common would otherwise come back from it."""
    out = {}
    for cap in caps:
        name = "single kernel" if cap < 0 else str(cap)
        with TemporaryKernelCache("keccak_table", {"AMD_COMGR_CACHE": "0"}), tempfile.TemporaryDirectory(prefix="comgr_cache_") as comgr:
            env = dict(os.environ, AMD_COMGR_CACHE_DIR=comgr)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--precompile-child", which, str(cap)], env=env, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit("bench_keccak_table: the precompile at cap %d failed: %s" % (cap, r.stderr[-2000:]))
            out[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print("precompile of", which, "at cap", cap, json.dumps(out[name]), file=sys.stderr, flush=True)
    return out


def _verified(desc, data):
    """the reference verifier of tests/stark_ref.py on the parsed bytes (tests/stark_verify.py)"""
    import stark_verify

    return stark_verify.accepts(desc, data)


def measure_compiled(ctx, bits, reps, unit_instrs, verify=True):
    """interpreted against compiled in units, alternating, inside a TemporaryKernelCache: the first size measured in it carries the
    cold compile time (the units' sources do not depend on the number of rows), every size the warm one"""
    desc = kt.stark_desc(bits, 2, fast_config_fri_params(bits))
    d_trace = kt.generate_trace(ctx, inputs_for(bits), bits)
    cold = not os.listdir(os.environ["PLONKY2_HIP_KERNEL_CACHE"])
    compile_ms = []
    for _ in range(2):  # cold (or warm), then warm: another handle with the cache the first one filled
        ns = pg.NativeStark(ctx, desc)
        t0 = time.perf_counter()
        ns.compile(unit_instrs=unit_instrs)
        compile_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        compiled = ns if len(compile_ms) == 2 else ns.close()
    interpreted = pg.NativeStark(ctx, desc)
    handles = {"interpreted": interpreted, "compiled": compiled}
    first = interpreted.prove_bytes(d_trace, [])
    if compiled.prove_bytes(d_trace, []) != first:
        raise SystemExit("bench_keccak_table: at 2^%d rows the proof compiled in units differs from the interpreted one" % bits)
    for ns in handles.values():
        ns.prove_bytes(d_trace, [])
    ms = {k: [] for k in handles}
    quotient = {k: [] for k in handles}
    for _ in range(reps):
        for k, ns in handles.items():
            timing = {}
            t0 = time.perf_counter()
            data = ns.prove_bytes(d_trace, [], timing)
            ms[k].append((time.perf_counter() - t0) * 1e3)
            quotient[k].append(timing["quotient polys"])
            if data != first:
                raise SystemExit("bench_keccak_table: the bytes changed between two calls")
    res = {"rows": 1 << bits, "units": compiled.num_units, "unit_instrs": unit_instrs,
           "compile_ms": {"cold": compile_ms[0] if cold else None, "warm": compile_ms[1]}, "proof_bytes": len(first)}
    for k in handles:
        res[k] = {"proof": stats(ms[k]), "quotient_stage": stats(quotient[k])}
    res["quotient_interpreted_over_compiled"] = round(res["interpreted"]["quotient_stage"]["median_ms"] / res["compiled"]["quotient_stage"]["median_ms"], 3)
    for ns in handles.values():
        ns.close()
    d_trace.free()
    if verify:
        if not _verified(desc, first):
            raise SystemExit("bench_keccak_table: the reference verifier rejects the proof at 2^%d rows" % bits)
        res["reference_verifier_accepts"] = True
    return res


def _merge_out(path, update):
    """the file's JSON object with `update`'s keys replaced"""
    res = {}
    if os.path.exists(path):
        with open(path) as f:
            res = json.loads(f.read() or "{}")
    res.update(update)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")
    return res


def main_compiled(a):
    head = {"tool": "tools/bench_keccak_table.py --compiled", "library": _lib.load().gl_version().decode(), "program_instructions": 47227}
    if a.precompile_caps:
        key = "precompile_cold%s: %s" % ("" if a.precompile_program == "keccak" else " of " + a.precompile_program, a.host)
        print(json.dumps(_merge_out(a.compiled_out, dict(head, **{key: measure_precompile(a.precompile_program, a.precompile_caps)}))))
        return
    ctx = pg.Context(0)
    res = dict(head, device=a.device, reps=a.reps, prove={}, caps={},
               yardstick="the interpreter (stark_quotient_values_kernel) in the same run: calls of the two handles alternate",
               prove_config="KeccakStark: 2430 columns, degree 3, Poseidon, standard_fast_config; trace built on the device and resident")
    for cap in a.caps or []:
        with TemporaryKernelCache("keccak_table", {"AMD_COMGR_CACHE": "0"}):
            res["caps"][str(cap)] = {"2^%d" % bits: measure_compiled(ctx, bits, a.reps, cap, verify=False) for bits in a.prove_bits}
        print("cap", cap, json.dumps(res["caps"][str(cap)]), file=sys.stderr, flush=True)
    with TemporaryKernelCache("keccak_table", {"AMD_COMGR_CACHE": "0"}):
        for bits in a.prove_bits:
            res["prove"]["2^%d" % bits] = measure_compiled(ctx, bits, a.reps, a.unit_instrs)
            print("2^%d" % bits, json.dumps(res["prove"]["2^%d" % bits]), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(_merge_out(a.compiled_out, res)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compiled", action="store_true", help="interpreted against compiled in units, in one run")
    ap.add_argument("--unit-instrs", type=int, default=0, help="the cap of --compiled; 0: the library's default")
    ap.add_argument("--caps", type=int, nargs="*", help="with --compiled: also measure each of these caps")
    ap.add_argument("--precompile-caps", type=int, nargs="*", help="device-free: cold gl_stark_precompile_units per cap")
    ap.add_argument("--precompile-program", choices=["keccak", "fuzz4000"], default="keccak",
                    help="what --precompile-caps compiles: the table, or the 4 000-instruction program of tests/stark_fuzz.py (cap -1: as one kernel)")
    ap.add_argument("--precompile-child", nargs=2, help=argparse.SUPPRESS)
    ap.add_argument("--host", default="this host", help="label of the machine --precompile-caps ran on, recorded as given")
    ap.add_argument("--compiled-out", default=os.path.join(ROOT, "profiles", "keccak_table_compiled.json"))
    ap.add_argument("--bits", type=int, nargs="+", default=[14, 16, 18, 20])
    ap.add_argument("--prove-bits", type=int, nargs="*", default=[12, 14])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--numpy-max-seconds", type=float, default=60.0, help="the host trace is timed while the next size is expected to stay below this")
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keccak_table.json"))
    a = ap.parse_args()
    if a.precompile_child:
        return precompile_child(a.precompile_child[0], int(a.precompile_child[1]))
    if a.reps < 5 or not all(5 <= b <= 20 for b in a.bits + a.prove_bits):
        ap.error("--reps >= 5; sizes in 2^5 .. 2^20 rows (a trace at 2^20 rows is 20.4 GB)")
    if a.compiled or a.precompile_caps:
        return main_compiled(a)
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
