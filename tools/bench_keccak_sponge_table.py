#!/usr/bin/env python3
"""The Keccak sponge table (plonky2_gpu_amd/keccak_sponge_table.py, csrc/keccak_sponge_table.hip): its two fill kernels against their
yardsticks, the whole call against the upload it replaces, and whole proofs of it, all in one run. Per size:

  rows        keccak_sponge_rows_kernel (one lane per row, 314 of the 414 columns, 34 read back) from the stage times of
              gl_debug_keccak_sponge_table_stage_ms, warm, median of --reps runs: milliseconds, 314 * 8 * n bytes stored / time and
              that as a fraction of gl_memset_zero over the same number of bytes; beside it logic_table_rows_kernel
              (gl_debug_logic_table_fill, one row per thread) with the memset of ITS bytes, in the same run. The yardstick is the logic
              kernel's fraction of the memset rate less 5 points.
  chain       keccak_sponge_chain_kernel (one lane per operation) on n one-block operations: permutations per second, beside the
              Keccak leaf kernel (gl_keccak_hash_no_pad_batch, 16 words per leaf: one block, one permutation per lane, 32 bytes
              stored) on n leaves. The chain kernel also stores 100 columns, 800 bytes, per row. Then the same number of blocks as
              operations of 64 blocks and as ONE operation that holds all blocks: what the serial chain and divergence cost.
  call        gl_keccak_sponge_table_trace by the wall clock with the wait for the stream (count, its one host wait, map, chain,
              rows), gl_keccak_sponge_table_ops with all three outputs the same way, and the upload of the finished 414-column trace
              from pageable host memory into the same buffer: what the host route pays after it has generated the trace.
  prove       gl_stark_prove of the device-built trace under starky's standard_fast_config, interpreted against compiled in
              units, the calls of the two handles alternating; the bytes must be equal, and the reference verifier of
              tests/stark_verify.py must accept them at the smallest size.

n rows hold n operations of 100 bytes each unless said otherwise (no padding rows). One JSON line on stdout and in --out (default
profiles/keccak_sponge_table.json).

  python tools/bench_keccak_sponge_table.py [--bits 14 16 18 20] [--chain-bits 16 20] [--prove-bits 12 16] [--reps 7] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import plonky2_gpu_amd as pg
from bench_common import TemporaryKernelCache, fast_config_fri_params, stats
from bench_logic_table import ops_for, timed_alternating
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd import keccak_sponge_table as ks
from plonky2_gpu_amd import logic_table as lt

ROWS_KERNEL_COLUMNS = ks.NUM_COLUMNS - 2 * ks.KECCAK_WIDTH_U32S  # everything but the state before and behind the permutation
STAGES = ("count", "map", "chain", "rows")
ONE_BLOCK_LEN = 100


def operations(num_ops, length):
    """[num_ops][5] records of `length` bytes each at consecutive addresses, and the random bytes"""
    w = np.zeros((num_ops, ks.OP_WORDS), dtype=np.uint64)
    w[:, 0] = np.arange(num_ops) % 7
    w[:, 2] = (np.arange(num_ops, dtype=np.uint64) * np.uint64(length)) % np.uint64(1 << 31)
    w[:, 3] = np.arange(num_ops)
    w[:, 4] = length
    return w, np.random.default_rng(num_ops).integers(0, 256, size=num_ops * length, dtype=np.uint8)


class Trace:
    """the buffers of one gl_keccak_sponge_table_trace at 2^bits rows"""

    def __init__(self, ctx, bits, words, data):
        self.ctx, self.bits, self.n, self.num_ops = ctx, bits, 1 << bits, len(words)
        self.d_ops = pg.DeviceBuffer.from_host(ctx, words)
        self.d_bytes, self.bytes_ptr = ks.upload_bytes(ctx, data)
        self.d_trace = pg.DeviceBuffer(ctx, ks.NUM_COLUMNS * self.n)
        self.scratch = pg.DeviceBuffer(ctx, _lib.load().gl_keccak_sponge_table_scratch_bytes(self.num_ops, bits) // 8)

    def stage_ms(self, reps, warm=2):
        """{stage: [ms]}, `warm` calls first"""
        ms, out = np.zeros(4, dtype=np.float32), {k: [] for k in STAGES}
        for rep in range(reps + warm):
            _lib.call("gl_debug_keccak_sponge_table_stage_ms", self.d_ops.ptr, self.num_ops, self.bytes_ptr, self.bits, self.d_trace.ptr, self.n,
                      self.scratch.ptr, ms, self.ctx.ptr)
            if rep >= warm:
                for k, v in zip(STAGES, ms):
                    out[k].append(float(v))
        return out

    def count(self):
        rows = ctypes.c_uint64()
        _lib.call("gl_keccak_sponge_table_trace", self.d_ops.ptr, self.num_ops, None, self.bits, None, 0, self.scratch.ptr, ctypes.byref(rows), self.ctx.ptr)
        return int(rows.value)

    def call(self):
        rows = ctypes.c_uint64()
        _lib.call("gl_keccak_sponge_table_trace", self.d_ops.ptr, self.num_ops, self.bytes_ptr, self.bits, self.d_trace.ptr, self.n, self.scratch.ptr,
                  ctypes.byref(rows), self.ctx.ptr)
        return int(rows.value)

    def free(self):
        for b in (self.d_ops, self.d_bytes, self.d_trace, self.scratch):
            b.free()


def wall(ctx, reps, call):
    out = []
    for rep in range(reps + 2):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        if rep >= 2:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def measure_rows_and_call(ctx, bits, reps, upload):
    n = 1 << bits
    t = Trace(ctx, bits, *operations(n, ONE_BLOCK_LEN))
    stage = t.stage_ms(reps)
    stored = ROWS_KERNEL_COLUMNS * 8 * n
    memset = timed_alternating(ctx, reps, {"memset": lambda: _lib.call("gl_memset_zero", t.d_trace.ptr, stored, ctx.ptr)})["memset"]
    med = float(np.median(stage["rows"]))
    res = {"rows": n, "operations": n, "bytes_stored_by_the_rows_kernel": stored, "bytes_read_back": ks.KECCAK_RATE_U32S * 8 * n + ONE_BLOCK_LEN * n,
           "stage_ms": {k: stats(v) for k, v in stage.items()},
           "memset_same_bytes": dict(stats(memset), tb_per_s=round(stored / float(np.median(memset)) / 1e9, 3)),
           "rows_kernel": dict(stats(stage["rows"]), tb_per_s=round(stored / med / 1e9, 3), fraction_of_memset=round(float(np.median(memset)) / med, 4))}
    # logic_table_rows_kernel and the memset of its bytes, in the same run
    lbytes = lt.NUM_COLUMNS * 8 * n
    d_lops, d_lt = pg.DeviceBuffer.from_host(ctx, ops_for(bits)), pg.DeviceBuffer(ctx, lt.NUM_COLUMNS * n)
    lms = timed_alternating(ctx, reps, {"logic": lambda: _lib.call("gl_debug_logic_table_fill", d_lops.ptr, n, bits, d_lt.ptr, n, 1, ctx.ptr),
                                        "memset": lambda: _lib.call("gl_memset_zero", d_lt.ptr, lbytes, ctx.ptr)})
    d_lops.free(), d_lt.free()
    lmed = float(np.median(lms["logic"]))
    res["logic_table_rows_kernel"] = dict(stats(lms["logic"]), bytes=lbytes, tb_per_s=round(lbytes / lmed / 1e9, 3),
                                          fraction_of_memset=round(float(np.median(lms["memset"])) / lmed, 4))
    res["yardstick_fraction"] = round(res["logic_table_rows_kernel"]["fraction_of_memset"] - 0.05, 4)
    res["rows_kernel_holds"] = res["rows_kernel"]["fraction_of_memset"] >= res["yardstick_fraction"]
    # the product calls by the wall clock
    call_ms = wall(ctx, reps, t.call)
    res["call_wall"] = stats(call_ms)
    num_bytes = n * ONE_BLOCK_LEN
    d_k, d_l, d_m = pg.DeviceBuffer(ctx, n * 25), pg.DeviceBuffer(ctx, n * 5 * 17), pg.DeviceBuffer(ctx, num_bytes * 14)
    ops_ms = wall(ctx, reps, lambda: _lib.call("gl_keccak_sponge_table_ops", t.d_trace.ptr, n, bits, n, d_k.ptr, d_l.ptr, d_m.ptr, t.scratch.ptr, ctx.ptr))
    res["ops_wall"] = dict(stats(ops_ms), bytes_written=(n * 25 + n * 85 + num_bytes * 14) * 8)
    for b in (d_k, d_l, d_m):
        b.free()
    if upload:
        nbytes = ks.NUM_COLUMNS * 8 * n
        host = t.d_trace.download()  # a finished trace, in pageable host memory
        up = wall(ctx, 3, lambda: t.d_trace.upload(host))
        both = float(np.median(call_ms)) + float(np.median(ops_ms))
        res["upload_of_the_finished_trace"] = dict(stats(up), bytes=nbytes, gb_per_s=round(nbytes / float(np.median(up)) / 1e6, 2),
                                                   over_call=round(float(np.median(up)) / float(np.median(call_ms)), 1),
                                                   over_call_and_ops=round(float(np.median(up)) / both, 1))
        res["call_and_ops_faster_than_upload"] = both < float(np.median(up))
        del host
    t.free()
    return res


def chain_case(ctx, bits, num_ops, length, reps, warm=2):
    t = Trace(ctx, bits, *operations(num_ops, length))
    rows = t.count()
    assert rows == 1 << bits, (rows, bits)
    ms = t.stage_ms(reps, warm)["chain"]
    t.free()
    med = float(np.median(ms))
    return dict(stats(ms), operations=num_ops, blocks_per_operation=length // 136 + 1, permutations_per_s=round((1 << bits) / med * 1e3))


def measure_chain(ctx, bits, reps, serial_budget_s):
    n = 1 << bits
    res = {"blocks": n, "one_block_operations": chain_case(ctx, bits, n, ONE_BLOCK_LEN, reps)}
    # the Keccak leaf kernel: n leaves of 16 words, one block and one permutation each
    d_in = pg.DeviceBuffer.from_host(ctx, np.random.default_rng(bits).integers(0, pg.P, size=16 * n, dtype=np.uint64))
    d_out = pg.DeviceBuffer(ctx, 4 * n)
    lms = timed_alternating(ctx, reps, {"leaves": lambda: _lib.call("gl_keccak_hash_no_pad_batch", d_in.ptr, 16, 16, n, d_out.ptr, ctx.ptr)})["leaves"]
    d_in.free(), d_out.free()
    res["keccak_leaf_kernel"] = dict(stats(lms), leaves=n, permutations_per_s=round(n / float(np.median(lms)) * 1e3))
    res["chain_over_leaf_kernel_time"] = round(res["one_block_operations"]["median_ms"] / res["keccak_leaf_kernel"]["median_ms"], 3)
    res["operations_of_64_blocks"] = chain_case(ctx, bits, n // 64, 63 * 136 + ONE_BLOCK_LEN, reps)
    per_block_ms = res["operations_of_64_blocks"]["median_ms"] / 64  # one lane's time per block when every lane of its waves is busy
    projected_s = per_block_ms * n / 1e3
    if projected_s <= serial_budget_s:
        res["one_operation_of_all_blocks"] = chain_case(ctx, bits, 1, (n - 1) * 136 + ONE_BLOCK_LEN, *((1, 0) if projected_s > 1 else (3, 1)))
    else:
        res["one_operation_of_all_blocks"] = {"skipped": "projected %.0f s on one lane, above --serial-budget-s" % projected_s}
    return res


def measure_prove(ctx, bits, reps, verify):
    """interpreted against compiled in units, alternating, inside a TemporaryKernelCache: the first size carries the cold compile"""
    desc = ks.stark_desc(bits, 2, fast_config_fri_params(bits))
    words, data = operations(1 << bits, ONE_BLOCK_LEN)
    d_trace = ks.generate_trace(ctx, words, data, degree_bits=bits)
    interpreted, compiled = pg.NativeStark(ctx, desc), pg.NativeStark(ctx, desc)
    t0 = time.perf_counter()
    compiled.compile(unit_instrs=0)
    compile_ms = round((time.perf_counter() - t0) * 1e3, 1)
    handles = {"interpreted": interpreted, "compiled": compiled}
    first = interpreted.prove_bytes(d_trace, [])
    if compiled.prove_bytes(d_trace, []) != first:
        raise SystemExit("bench_keccak_sponge_table: at 2^%d rows the compiled proof differs from the interpreted one" % bits)
    ms, stages = {k: [] for k in handles}, {}
    for _ in range(reps):
        for k, ns in handles.items():
            timing = {}
            t0 = time.perf_counter()
            data = ns.prove_bytes(d_trace, [], timing)
            ms[k].append((time.perf_counter() - t0) * 1e3)
            stages[k] = {name: round(v, 3) for name, v in timing.items()}
            if data != first:
                raise SystemExit("bench_keccak_sponge_table: the bytes changed between two calls")
    res = {"rows": 1 << bits, "units": compiled.num_units, "compile_ms": compile_ms, "proof_bytes": len(first), "bytes_equal": True,
           "program_instructions": int(desc.instrs.shape[0])}
    for k in handles:
        res[k] = {"proof": stats(ms[k]), "stage_ms": stages[k]}
    res["proof_interpreted_over_compiled"] = round(res["interpreted"]["proof"]["median_ms"] / res["compiled"]["proof"]["median_ms"], 3)
    for ns in handles.values():
        ns.close()
    d_trace.free()
    if verify:
        import stark_verify

        if not stark_verify.accepts(desc, first):
            raise SystemExit("bench_keccak_sponge_table: the reference verifier rejects the proof at 2^%d rows" % bits)
        res["reference_verifier_accepts"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="*", default=[14, 16, 18, 20])
    ap.add_argument("--chain-bits", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--prove-bits", type=int, nargs="*", default=[12, 16])
    ap.add_argument("--upload-max-bits", type=int, default=20, help="the upload is timed up to this size (2^20 rows are 3.5 GB of host memory)")
    ap.add_argument("--serial-budget-s", type=float, default=20.0, help="one operation of all blocks runs only if its projected time is below this")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keccak_sponge_table.json"))
    a = ap.parse_args()
    if a.reps < 3 or not all(7 <= b <= 20 for b in a.bits + a.prove_bits + a.chain_bits):
        ap.error("--reps >= 3; sizes in 2^7 .. 2^20 rows (a trace at 2^20 rows is 3.5 GB)")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_keccak_sponge_table.py", "device": a.device, "library": _lib.load().gl_version().decode(), "reps": a.reps,
           "columns": ks.NUM_COLUMNS, "operation_bytes": ONE_BLOCK_LEN,
           "yardstick": "logic_table_rows_kernel's fraction of the memset rate of its bytes in the same run, less 5 points",
           "prove_config": "KeccakSpongeStark: 414 columns, 435 constraints, Poseidon, standard_fast_config (2 challenges, rate_bits 1, cap_height 4, "
                           "16 PoW bits, arity 4 down to 2^5, 84 queries); trace built on the device and resident; compiled in units at the library's cap",
           "trace": {}, "chain": {}, "prove": {}}
    for bits in sorted(a.bits):
        res["trace"]["2^%d" % bits] = measure_rows_and_call(ctx, bits, a.reps, bits <= a.upload_max_bits)
        print("2^%d" % bits, json.dumps(res["trace"]["2^%d" % bits]), file=sys.stderr, flush=True)
    for bits in sorted(a.chain_bits):
        res["chain"]["2^%d" % bits] = measure_chain(ctx, bits, a.reps, a.serial_budget_s)
        print("chain 2^%d" % bits, json.dumps(res["chain"]["2^%d" % bits]), file=sys.stderr, flush=True)
    with TemporaryKernelCache("keccak_sponge_table"):
        for k, bits in enumerate(sorted(a.prove_bits)):
            res["prove"]["2^%d" % bits] = measure_prove(ctx, bits, a.reps, verify=k == 0)
            print("prove 2^%d" % bits, json.dumps(res["prove"]["2^%d" % bits]), file=sys.stderr, flush=True)
    res["rows_kernel_holds_at_every_size"] = all(v["rows_kernel_holds"] for v in res["trace"].values())
    res["call_and_ops_faster_than_upload_at_every_measured_size"] = all(v.get("call_and_ops_faster_than_upload", True) for v in res["trace"].values())
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
