#!/usr/bin/env python3
"""The lookup columns of a trace on the device (gl_stark_fill_lookups, csrc/lookup.hip) against the host route they replace, and
against the proof of the same table, at 2^16 .. 2^22 rows, trace resident in HBM. Per size:

  fill        gl_stark_fill_lookups of ONE lookup, timed by events on the context's stream and by the wall clock around the call and
              a synchronisation, for two kinds of columns:
                range_check  inputs uniform in [0, n), table = the counter 0 .. n - 1 (5 - 6 of the 8 radix passes drop out)
                full_width   inputs drawn from a table of random words of the whole field
  host        the route a host without this call takes for the same two columns: download both, numpy.sort of their canonical values,
              the serial merge of permuted_cols (evm/src/lookup.rs:95-128), upload both results. The merge is a plain Python loop here
              (a Rust host runs it one to two orders of magnitude faster): it is timed once, up to --merge-max-bits, reported apart
              from the three steps that do not depend on the host's language, and its result must equal the device's.
  prove       gl_stark_prove of the range-check STARK "L" (6 columns, degree 3: a counter, the values, the two permuted columns with
              eval_lookups and their two permutation pairs, two filler columns) under starky's standard_fast_config, its lookup
              columns filled by the device

Oracle-free. One JSON line on stdout and in --out (default profiles/lookup_permuted_cols.json).

  python tools/bench_lookup.py [--min-bits 16] [--max-bits 22] [--reps 7] [--merge-max-bits 20] [--device LABEL]
                              [--out profiles/lookup_permuted_cols.json]"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import plonky2_gpu_amd as pg
from bench_common import fast_config_fri_params, stats
from plonky2_gpu_amd import _lib, lookup
from plonky2_gpu_amd import stark as pstark

P = 0xFFFFFFFF00000001
C0, V, PV, PT, F4, F5 = range(6)
LOOKUPS = [(V, C0, PV, PT)]


def serial_merge(s, t):
    """lookup.rs:90-128 over the sorted canonical columns (Python ints)"""
    n = len(s)
    inds, vals, out = [], [], [0] * n
    i = j = 0
    while j < n and i < n:
        a, b = s[i], t[j]
        if a > b:
            vals.append(b)
            j += 1
        elif a < b:
            if vals:
                out[i] = vals.pop()
            else:
                inds.append(i)
            i += 1
        else:
            out[i] = b
            i += 1
            j += 1
    vals.extend(t[j:])
    inds.extend(range(i, n))
    for ind, val in zip(inds, vals):
        out[ind] = val
    return out


def measure_fill(ctx, n, inputs, table, reps, merge):
    """one lookup in a four-column trace (input, table, permuted input, permuted table)"""
    host = np.zeros((4, n), dtype=np.uint64)
    host[0], host[1] = inputs, table
    d = pg.DeviceBuffer.from_host(ctx, host)
    scratch = pg.DeviceBuffer(ctx, lookup.scratch_words(n))
    e0, e1 = pg.Event(), pg.Event()
    dev_ms, wall_ms = [], []
    for rep in range(reps + 2):  # two warm-up calls
        ctx.synchronize()
        t0 = time.perf_counter()
        e0.record(ctx)
        lookup.fill_lookups(ctx, d, n, 4, [(0, 1, 2, 3)], scratch=scratch)
        e1.record(ctx)
        ctx.synchronize()
        if rep >= 2:
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(e1.elapsed_ms_since(e0))
    got = d.download().reshape(4, n)
    res = {"device": stats(dev_ms), "device_wall": stats(wall_ms)}
    # the host route
    down, sort, up = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        a, b = d.download(0, n), d.download(n, n)
        t1 = time.perf_counter()
        s = np.sort(np.where(a >= np.uint64(P), a - np.uint64(P), a))
        t = np.sort(np.where(b >= np.uint64(P), b - np.uint64(P), b))
        t2 = time.perf_counter()
        d.upload(s, 2 * n)
        d.upload(got[3], 3 * n)
        t3 = time.perf_counter()
        down.append((t1 - t0) * 1e3), sort.append((t2 - t1) * 1e3), up.append((t3 - t2) * 1e3)
    if not (s == got[2]).all():
        raise SystemExit("bench_lookup: the device's permuted inputs are not the sorted inputs")
    res["host"] = {"download": stats(down), "numpy_sort": stats(sort), "upload": stats(up),
                   "without_merge_median_ms": round(float(np.median(down) + np.median(sort) + np.median(up)), 4)}
    if merge:
        t0 = time.perf_counter()
        pt = serial_merge(s.tolist(), t.tolist())
        res["host"]["merge_python_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        if not (np.array(pt, dtype=np.uint64) == got[3]).all():
            raise SystemExit("bench_lookup: the device's permuted table is not the serial merge's")
    d.free(), scratch.free()
    return res


def l_desc(degree_bits):
    a = pstark.StarkAsm()
    a.emit_first_row(a.local(C0))
    a.emit_transition(a.sub(a.next(C0), a.add(a.local(C0), a.imm(1))))
    a.release()
    a.eval_lookups(PV, PT)
    a.release()
    a.emit_transition(a.sub(a.sub(a.next(F4), a.local(F4)), a.local(C0)))
    a.emit_transition(a.sub(a.sub(a.next(F5), a.local(F5)), a.mul(a.mul(a.local(V), a.local(PV)), a.local(PT))))
    instrs, imms = a.program()
    return pstark.StarkDesc(degree_bits, 6, 0, 3, 2, fast_config_fri_params(degree_bits), instrs, imms, lookup.lookup_pairs(LOOKUPS))


def measure_prove(ctx, degree_bits, values, reps):
    """the device fills pv and pt; f5 needs them, so it is completed on the host once and uploaded"""
    n = 1 << degree_bits
    host = np.zeros((6, n), dtype=np.uint64)
    host[C0], host[V] = np.arange(n, dtype=np.uint64), values
    host[F4] = np.uint64(3) + np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(host[C0][:-1], dtype=np.uint64)))  # below 2^45: no reduction needed
    d = pg.DeviceBuffer.from_host(ctx, host)
    scratch = pg.DeviceBuffer(ctx, lookup.scratch_words(n))
    lookup.fill_lookups(ctx, d, n, 6, LOOKUPS, scratch=scratch)
    pv, pt = d.download(PV * n, n), d.download(PT * n, n)
    prod = (host[V] * pv).tolist()  # below 2^44
    steps = (x * int(y) for x, y in zip(prod[:-1], pt[:-1]))
    d.upload(np.array(list(itertools.accumulate(steps, lambda acc, x: (acc + x) % P, initial=5)), dtype=np.uint64), F5 * n)
    desc = l_desc(degree_bits)
    ns = pg.NativeStark(ctx, desc)
    first = ns.prove_bytes(d, [])
    ns.prove_bytes(d, [])
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        data = ns.prove_bytes(d, [])
        ms.append((time.perf_counter() - t0) * 1e3)
        if data != first:
            raise SystemExit("bench_lookup: the proof is not deterministic")
    timing = {}
    ns.prove_bytes(d, [], timing)
    ns.close()
    d.free(), scratch.free()
    return dict(stats(ms), proof_bytes=len(first), stage_ms={k: round(v, 3) for k, v in timing.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-bits", type=int, default=16)
    ap.add_argument("--max-bits", type=int, default=22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--merge-max-bits", type=int, default=20)
    ap.add_argument("--device", default="one MI355X (gfx950)", help="label of the device the numbers come from, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_permuted_cols.json"))
    a = ap.parse_args()
    if a.reps < 1 or not 6 <= a.min_bits <= a.max_bits <= 22:
        ap.error("--reps >= 1 and 6 <= --min-bits <= --max-bits <= 22")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_lookup.py", "device": a.device, "library": _lib.load().gl_version().decode(), "reps": a.reps,
           "prove_config": "L: 6 columns, degree 3, Poseidon, standard_fast_config (2 challenges, rate_bits 1, cap_height 4, 16 PoW bits, "
                           "arity 4 down to 2^5, 84 queries); trace resident", "sizes": {}}
    for bits in range(a.min_bits, a.max_bits + 1):
        n = 1 << bits
        rng = np.random.default_rng(bits)
        values = rng.integers(0, n, size=n, dtype=np.uint64)
        words = rng.integers(0, P, size=n, dtype=np.uint64)
        merge = bits <= a.merge_max_bits
        entry = {"scratch_bytes": lookup.scratch_words(n) * 8,
                 "range_check": measure_fill(ctx, n, values, np.arange(n, dtype=np.uint64), a.reps, merge),
                 "full_width": measure_fill(ctx, n, words[rng.integers(0, n, size=n)], words, a.reps, merge),
                 "prove": measure_prove(ctx, bits, values, a.reps)}
        entry["fill_over_prove"] = round(entry["range_check"]["device"]["median_ms"] / entry["prove"]["median_ms"], 4)
        entry["host_without_merge_over_fill"] = round(entry["range_check"]["host"]["without_merge_median_ms"] / entry["range_check"]["device_wall"]["median_ms"], 2)
        res["sizes"]["2^%d" % bits] = entry
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
