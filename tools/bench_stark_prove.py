#!/usr/bin/env python3
"""Whole STARK proofs (gl_stark_create / gl_stark_prove) of two shapes under starky's standard_fast_config (2 challenges, rate_bits 1,
cap_height 4, 16 proof-of-work bits, ConstantArityBits(4, 5), 84 query rounds; starky/src/config.rs:17-29):

  fibonacci  the reference's FibonacciStark: 4 columns, degree 2, one permutation pair
  wide       100 columns, degree 3: a counter and 33 triples (a, b, c) with c = a * b * counter on every row, two permutation-free
             transition / boundary constraints on the counter: 35 constraints, quotient_degree_factor 2

at 2^16 .. 2^20 rows, trace resident in HBM. Per shape and size: the handle is created and warmed (two proofs), then `--reps` proofs
are timed by the wall clock around gl_stark_prove (it ends synchronised); median, min and max, and the h_stage_ms breakdown of one
further proof. Oracle-free: every proof must equal the first one and round-trip through the wire format; that the proofs of these
shapes are VALID — accepted by the reference verifier — is tests/test_gpu_stark_scale.py's, which imports the shapes from here. One
JSON line on stdout (and --out, by default profiles/stark_prove.json).

  python tools/bench_stark_prove.py [--min-bits 16] [--max-bits 20] [--reps 7] [--out profiles/stark_prove.json]

The shape `ctl` (--shapes ctl, not among the defaults) is a multi-table STARK (gl_stark_tables_create / gl_stark_tables_prove): three
tables of 100, 30 and 8 columns at 2^18, 2^16 and 2^14 rows, degree 3, tied by four cross-table lookups, each table under
standard_fast_config at its own size. In the same run the three tables are also proved one by one with gl_stark_prove, without their
lookups; the result — per-table stage times, both totals and their ratio — goes to --ctl-out (profiles/stark_ctl_prove.json).

  python tools/bench_stark_prove.py --shapes ctl [--reps 7] [--ctl-out profiles/stark_ctl_prove.json]

--compiled measures the compiled quotient kernels (gl_stark_compile, csrc/stark_jit.hip) against the interpreter IN THE SAME RUN:
for every shape and size the same trace is proved through an interpreted and a compiled handle, the bytes must be equal (else the
tool exits non-zero), and median / min / max and stage_ms of both are recorded, with compile_ms cold (an empty temporary
PLONKY2_HIP_KERNEL_CACHE; the compiler's own library is asked not to cache either, AMD_COMGR_CACHE=0) and warm (the same cache
again). A shape's source does not depend on the number of rows: the FIRST size of a shape carries the cold figure, the later ones
come back from the compiler library in about 11 ms. The shapes are fibonacci, wide, ctl and

  dense      100 columns, degree 3, 1 466 instructions at the density of the reference's bitwise tables: a filter column, 96 bit
             columns (three words of 32 bits) and three word columns; per bit column booleanity and the xor of two neighbours
             against the next row, per word the 32-bit recomposition by ACC / ACCR, every constraint under the filter. Timed
             through gl_stark_quotient_polys on random words (that needs no valid trace), compiled against interpreted.

  python tools/bench_stark_prove.py --compiled [--shapes fibonacci,wide,dense,ctl] [--reps 7] [--compiled-out profiles/stark_compiled.json]

--unit-instrs N (with --compiled) adds to the shapes timed through gl_stark_quotient_polys a THIRD handle, compiled in units of at
most N instructions (gl_stark_compile_units; 0: the library's default cap): `cut` beside `compiled`, with its own cold and warm
compile_ms and its number of units — what cutting costs at run time and saves at compile time. Besides dense that is

  fuzz4000   the 4 000-instruction program of tests/stark_fuzz.py (description 11: 4 challenges, 3 public inputs) without its
             permutation pairs: the longest single basic block the suite compiles

  python tools/bench_stark_prove.py --compiled --unit-instrs 0 --shapes dense,fuzz4000 [--min-bits 16] [--max-bits 20]"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import plonky2_gpu_amd as pg
from bench_common import fast_config_fri_params
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd import stark as pstark

P = 0xFFFFFFFF00000001
WIDE_TRIPLES = 33


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


CTL_TABLES = ((100, 18), (30, 16), (8, 14))  # (columns, degree_bits)


def ctl_table(ctx, columns, degree_bits, flags):
    """(program, trace in HBM) of one table: c0 counts from 5, then triples (a, b, c) with c = a * b * c0 (degree 3), then one
    binary flag column per entry of `flags` (1 on the first 2^flag rows), then free columns"""
    triples = (columns - 1 - len(flags)) // 3
    a = pstark.StarkAsm()
    a.emit_first_row(a.sub(a.local(0), a.imm(5)))
    a.emit_transition(a.sub(a.next(0), a.add(a.local(0), a.imm(1))))
    for j in range(triples):
        a.release()
        a.emit(a.sub(a.local(3 + 3 * j), a.mul(a.mul(a.local(1 + 3 * j), a.local(2 + 3 * j)), a.local(0))))
    for k in range(len(flags)):
        a.release()
        f = a.local(1 + 3 * triples + k)
        a.emit(a.mul(f, a.sub(f, a.imm(1))))
    n = 1 << degree_bits
    trace = np.random.default_rng(columns).integers(0, P, size=(columns, n), dtype=np.uint64)
    trace[0] = np.arange(5, n + 5, dtype=np.uint64)
    for k, bits in enumerate(flags):
        trace[1 + 3 * triples + k] = (np.arange(n) < (1 << bits)).astype(np.uint64)
    d_trace = pg.DeviceBuffer.from_host(ctx, trace)
    for j in range(triples):
        out = d_trace.at((3 + 3 * j) * n)
        _lib.call("gl_debug_field_op", 2, d_trace.at((1 + 3 * j) * n), d_trace.at((2 + 3 * j) * n), out, n, ctx.ptr)
        _lib.call("gl_debug_field_op", 2, out, d_trace.at(0), out, n, ctx.ptr)
    ctx.synchronize()
    return a.program(), d_trace, 1 + 3 * triples


def ctl_system(ctx, hasher="poseidon"):
    """(StarkTablesDesc, the tables' StarkDescs, traces in HBM). Four lookups, all of them satisfied: the first 2^14 counters of
    tables 0 and 1 into table 2 and the first 2^16 counters of table 0 into table 1 (filtered on the looking side by a flag column,
    on the looked side by the constant 1), and table 2 into itself without filters over two columns: 4, 4 and 8 CTL Zs."""
    Col, Twc, Lookup = pstark.CtlColumn, pstark.TableWithColumns, pstark.CrossTableLookup
    flags = ((14, 16), (14,), ())
    built = [ctl_table(ctx, cols, db, fl) for (cols, db), fl in zip(CTL_TABLES, flags)]
    descs = [pstark.StarkDesc(db, cols, 0, 3, 2, fast_config_fri_params(db), prog[0], prog[1], [])
             for (cols, db), (prog, _, _) in zip(CTL_TABLES, built)]
    f0, f1 = built[0][2], built[1][2]  # the first flag column of tables 0 and 1
    one, counter = Col.constant(1), [Col.single(0)]
    both = [Col.single(0), Col.linear_combination([(0, 2)], 1)]
    lookups = [Lookup([Twc(0, counter, Col.single(f0))], Twc(2, counter, one)), Lookup([Twc(1, counter, Col.single(f1))], Twc(2, counter, one)),
               Lookup([Twc(0, counter, Col.single(f0 + 1))], Twc(1, counter, one)), Lookup([Twc(2, both)], Twc(2, both))]
    desc = pstark.StarkTablesDesc(descs, lookups)
    desc.validate(hasher)
    return desc, descs, [d for _, d, _ in built]


def measure_ctl(ctx, reps, hasher="poseidon"):
    desc, descs, traces = ctl_system(ctx, hasher)

    def timed(fn):
        first = fn()
        fn()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            data = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            if data != first:
                raise SystemExit("bench_stark_prove: the proof is not deterministic")
        return first, {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    nt = pg.NativeStarkTables(ctx, desc, hasher)
    first, res = timed(lambda: nt.prove_bytes(traces))
    if pstark.tables_proof_to_bytes(pstark.tables_proof_from_bytes(first, desc, hasher), desc, hasher) != first:
        raise SystemExit("bench_stark_prove: the proof does not round-trip through the wire format")
    timing = []
    nt.prove_bytes(traces, timing=timing)
    nt.close()
    res["proof_bytes"] = len(first)
    res["tables"] = [{"columns": cols, "degree_bits": db, "ctl_zs": desc.num_ctl_zs(k), "stage_ms": {s: round(v, 3) for s, v in timing[k].items()},
                      "total_ms": round(sum(timing[k].values()), 3)} for k, (cols, db) in enumerate(CTL_TABLES)]
    alone = []
    for d, d_trace in zip(descs, traces):  # the same tables without their lookups, one gl_stark_prove each
        ns = pg.NativeStark(ctx, d, hasher)
        stages = {}
        _, r = timed(lambda: ns.prove_bytes(d_trace, []))
        ns.prove_bytes(d_trace, [], stages)
        ns.close()
        r["stage_ms"] = {s: round(v, 3) for s, v in stages.items()}
        alone.append(r)
    for d_trace in traces:
        d_trace.free()
    res["without_lookups"] = alone
    res["without_lookups_sum_median_ms"] = round(sum(r["median_ms"] for r in alone), 3)
    res["ratio"] = round(res["median_ms"] / res["without_lookups_sum_median_ms"], 4)
    return res


# ---------------------------------------------------------------- --compiled: the compiled quotient kernels against the interpreter
DENSE_WORDS = 3


def dense_desc(degree_bits):
    """the description of `dense`: column 0 the filter, columns 1 .. 96 bits, columns 97 .. 99 words"""
    bits, cols = 32 * DENSE_WORDS, 1 + 33 * DENSE_WORDS
    a = pstark.StarkAsm()
    f, one = a.local(0), a.imm(1)
    for w in range(DENSE_WORDS):
        halves = []
        for h in range(2):  # 16 bits per ACCR: 32 weights up to 2^31 would pass the accumulator's bound of 2^63
            for k in range(16):
                j = 32 * w + 16 * h + k
                b = a.local(1 + j)
                a.acc(b, 1 << k)
                t = a.sub(b, one)
                a.mul(b, t, dst=t)
                a.mul(f, t, dst=t)
                a.emit(t)  # f b (b - 1)
                b2, nxt = a.local(1 + (j + 1) % bits), a.next(1 + j)
                a.mul(b, b2, dst=t)
                a.add(b, b2, dst=b)
                a.mulk(t, 1, dst=t)
                a.sub(b, t, dst=b)  # b xor b' = b + b' - 2 b b'
                a.sub(nxt, b, dst=nxt)
                a.mul(f, nxt, dst=nxt)
                a.emit_transition(nxt)  # f (b_j' - (b_j xor b_j+1))
                a.free(b, t, b2, nxt)
            halves.append(a.accr())
        lo, s = halves
        a.mulk(s, 16, dst=s)
        a.add(lo, s, dst=s)
        word = a.local(1 + bits + w)
        a.sub(word, s, dst=s)
        a.mul(f, s, dst=s)
        a.emit(s)  # f (word - sum 2^k b_k)
        a.free(lo, word, s)
    instrs, imms = a.program()
    return pstark.StarkDesc(degree_bits, cols, 0, 3, 2, fast_config_fri_params(degree_bits), instrs, imms, [])


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def _compile_ms(make_handle, unit_instrs=None):
    """(cold, warm): gl_stark_compile / gl_stark_tables_compile of a fresh handle with an empty temporary kernel cache, and of
    another fresh handle with the cache the first one filled; `unit_instrs`: in units (gl_stark_compile_units)"""
    cache = tempfile.mkdtemp(prefix="stark_kernel_cache_")
    saved = os.environ.get("PLONKY2_HIP_KERNEL_CACHE")
    os.environ["PLONKY2_HIP_KERNEL_CACHE"] = cache
    try:
        out = []
        for _ in range(2):
            h = make_handle()
            t0 = time.perf_counter()
            h.compile(unit_instrs)
            out.append(round((time.perf_counter() - t0) * 1e3, 1))
            h.close()
        return out
    finally:
        if saved is None:
            os.environ.pop("PLONKY2_HIP_KERNEL_CACHE", None)
        else:
            os.environ["PLONKY2_HIP_KERNEL_CACHE"] = saved
        shutil.rmtree(cache, ignore_errors=True)


def _both(reps, interpreted, compiled):
    """`reps` timed calls of each, alternating, after two warm-up calls of each; both must return what the interpreter returned first"""
    first = interpreted()
    if compiled() != first:
        raise SystemExit("bench_stark_prove: the compiled handle's bytes differ from the interpreted handle's")
    interpreted(), compiled()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((interpreted, compiled)):
            t0 = time.perf_counter()
            data = fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            if data != first:
                raise SystemExit("bench_stark_prove: the bytes changed between two calls")
    return _stats(ms[0]), _stats(ms[1])


def measure_compiled(ctx, make, degree_bits, reps, hasher="poseidon"):
    desc, d_trace, pis = make(ctx, degree_bits)
    cold, warm = _compile_ms(lambda: pg.NativeStark(ctx, desc, hasher))
    handles = [pg.NativeStark(ctx, desc, hasher), pg.NativeStark(ctx, desc, hasher, compiled=True)]
    res = {"columns": desc.num_columns, "instructions": int(desc.instrs.shape[0]), "compile_ms": {"cold": cold, "warm": warm}}
    res["interpreted"], res["compiled"] = _both(reps, *[lambda ns=ns: ns.prove_bytes(d_trace, pis) for ns in handles])
    for key, ns in zip(("interpreted", "compiled"), handles):
        timing = {}
        ns.prove_bytes(d_trace, pis, timing)
        res[key]["stage_ms"] = {k: round(v, 3) for k, v in timing.items()}
        ns.close()
    d_trace.free()
    return res


def fuzz4000_desc(degree_bits):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import stark_fuzz as sf

    case = sf.fuzz_case(sf.LENGTHS.index(4000))
    s = case["stark"]
    return pstark.StarkDesc(degree_bits, s.num_columns, s.num_public_inputs, s.constraint_degree, case["num_challenges"],
                            fast_config_fri_params(degree_bits), s.instrs, s.immediates, [])


def measure_dense(ctx, degree_bits, reps, hasher="poseidon", make_desc=None, unit_instrs=None):
    """gl_stark_quotient_polys on random words in place of the trace's LDE: the call ends synchronised and includes the upload of the
    public inputs and the coset iNTT of the quotient columns, the same on every side. `unit_instrs`: a third handle, compiled in
    units of at most that many instructions"""
    desc = (make_desc or dense_desc)(degree_bits)
    n_ext, size = 1 << (degree_bits + 1), 1 << (degree_bits + desc.quotient_degree_bits)
    rng = np.random.default_rng(degree_bits)
    d_lde = pg.DeviceBuffer(ctx, desc.num_columns * n_ext)
    for c in range(desc.num_columns):
        _lib.call("gl_memcpy_h2d", d_lde.at(c * n_ext), rng.integers(0, P, size=n_ext, dtype=np.uint64), 8 * n_ext, ctx.ptr)
    alphas = np.ascontiguousarray(rng.integers(0, P, size=desc.num_challenges, dtype=np.uint64))
    pis = np.ascontiguousarray(rng.integers(0, P, size=max(1, desc.num_public_inputs), dtype=np.uint64))
    cold, warm = _compile_ms(lambda: pg.NativeStark(ctx, desc, hasher))
    handles = [pg.NativeStark(ctx, desc, hasher), pg.NativeStark(ctx, desc, hasher, compiled=True)]
    names = ["interpreted", "compiled"]
    if unit_instrs is not None:
        cut_cold, cut_warm = _compile_ms(lambda: pg.NativeStark(ctx, desc, hasher), unit_instrs)
        handles.append(pg.NativeStark(ctx, desc, hasher, compiled=True, unit_instrs=unit_instrs))
        names.append("cut")
    outs = [pg.DeviceBuffer(ctx, desc.num_challenges * size) for _ in handles]

    def call(ns, d_q):
        _lib.call("gl_stark_quotient_polys", ns.ptr, d_lde.ptr, None, n_ext, alphas, None, pis, d_q.ptr, ctx.ptr)

    for ns, d_q in zip(handles, outs):
        call(ns, d_q)
    if not all((outs[0].download() == d_q.download()).all() for d_q in outs[1:]):
        raise SystemExit("bench_stark_prove: a compiled handle's quotient differs from the interpreted handle's")
    ms = tuple([] for _ in handles)
    for _ in range(reps):
        for k, (ns, d_q) in enumerate(zip(handles, outs)):
            t0 = time.perf_counter()
            call(ns, d_q)
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {"columns": desc.num_columns, "instructions": int(desc.instrs.shape[0]), "compile_ms": {"cold": cold, "warm": warm}}
    for k, name in enumerate(names):
        res[name] = dict(_stats(ms[k]), call="gl_stark_quotient_polys")
    if unit_instrs is not None:
        res["cut"].update(unit_instrs=unit_instrs, units=handles[2].num_units, compile_ms={"cold": cut_cold, "warm": cut_warm})
    for ns in handles:
        ns.close()
    for b in outs + [d_lde]:
        b.free()
    return res


def measure_ctl_compiled(ctx, reps, hasher="poseidon"):
    desc, _, traces = ctl_system(ctx, hasher)
    cold, warm = _compile_ms(lambda: pg.NativeStarkTables(ctx, desc, hasher))
    handles = [pg.NativeStarkTables(ctx, desc, hasher), pg.NativeStarkTables(ctx, desc, hasher, compiled=True)]
    res = {"tables": [{"columns": cols, "degree_bits": db, "ctl_zs": desc.num_ctl_zs(k), "instructions": int(desc.tables[k].instrs.shape[0])}
                      for k, (cols, db) in enumerate(CTL_TABLES)], "compile_ms": {"cold": cold, "warm": warm}}
    res["interpreted"], res["compiled"] = _both(reps, *[lambda nt=nt: nt.prove_bytes(traces) for nt in handles])
    for key, nt in zip(("interpreted", "compiled"), handles):
        timing = []
        nt.prove_bytes(traces, timing=timing)
        res[key]["stage_ms"] = [{s: round(v, 3) for s, v in t.items()} for t in timing]
        res[key]["quotient_polys_ms"] = round(sum(t["quotient polys"] for t in timing), 3)
        nt.close()
    for d_trace in traces:
        d_trace.free()
    return res


def main_compiled(a, ctx, res):
    os.environ["AMD_COMGR_CACHE"] = "0"  # a cold compile_ms is meant to be hiprtc's own time (see the module's text on later sizes)
    res = dict(res, yardstick="the interpreter (stark_quotient_values_kernel) in the same run: calls of the two handles alternate")
    makers = {"fibonacci": fibonacci, "wide": wide}
    for shape in a.shapes.split(","):
        if shape == "ctl":
            res["ctl"] = measure_ctl_compiled(ctx, a.reps)
            continue
        res[shape] = {}
        for bits in range(a.min_bits, a.max_bits + 1):
            if shape in ("dense", "fuzz4000"):
                res[shape]["2^%d" % bits] = measure_dense(ctx, bits, a.reps, make_desc=fuzz4000_desc if shape == "fuzz4000" else None, unit_instrs=a.unit_instrs)
            else:
                res[shape]["2^%d" % bits] = measure_compiled(ctx, makers[shape], bits, a.reps)
            print(shape, bits, json.dumps(res[shape]["2^%d" % bits]), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    if a.compiled_out:
        os.makedirs(os.path.dirname(a.compiled_out), exist_ok=True)
        with open(a.compiled_out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-bits", type=int, default=16)
    ap.add_argument("--max-bits", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=None, help="default: fibonacci,wide; with --compiled: fibonacci,wide,dense,ctl")
    ap.add_argument("--compiled", action="store_true", help="compiled quotient kernels against the interpreter, in one run")
    ap.add_argument("--unit-instrs", type=int, default=None, help="with --compiled: also a handle compiled in units of at most N (0: the default cap)")
    ap.add_argument("--compiled-out", default=os.path.join(ROOT, "profiles", "stark_compiled.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_prove.json"))
    ap.add_argument("--ctl-out", default=os.path.join(ROOT, "profiles", "stark_ctl_prove.json"))
    a = ap.parse_args()
    if a.reps < 1 or not 6 <= a.min_bits <= a.max_bits <= 22:
        ap.error("--reps >= 1 and 6 <= --min-bits <= --max-bits <= 22")
    a.shapes = a.shapes or ("fibonacci,wide,dense,ctl" if a.compiled else "fibonacci,wide")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_stark_prove.py", "library": _lib.load().gl_version().decode(), "hasher": "poseidon", "reps": a.reps,
           "config": "standard_fast_config: 2 challenges, rate_bits 1, cap_height 4, 16 PoW bits, arity 4 down to 2^5, 84 queries; trace resident"}
    if a.compiled:
        return main_compiled(a, ctx, res)
    makers = {"fibonacci": fibonacci, "wide": wide}
    shapes = a.shapes.split(",")
    if "ctl" in shapes:
        shapes.remove("ctl")
        ctl = dict(res, shape="three tables of 100, 30 and 8 columns at 2^18, 2^16 and 2^14 rows, degree 3, four cross-table lookups",
                   **measure_ctl(ctx, a.reps))
        line = json.dumps(ctl)
        if a.ctl_out:
            os.makedirs(os.path.dirname(a.ctl_out), exist_ok=True)
            with open(a.ctl_out, "w") as f:
                f.write(line + "\n")
        print(line)
    if not shapes:
        ctx.close()
        return
    for shape in shapes:
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
