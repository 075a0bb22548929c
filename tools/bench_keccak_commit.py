#!/usr/bin/env python3
"""Commit with the Keccak tree against the commit with the Poseidon tree, same device, same minute: rows x 135 columns, rate 8
(rate_bits 3), cap height 4, with the leaf-major output. Both paths are warmed, then Poseidon (gl_commit_from_values) and
Keccak (gl_commit_from_values_h) commits alternate, HIP events around each; medians and min-max for both, leaves per second, and
the gate: the Keccak commit's median is not above the Poseidon commit's. One JSON line on stdout (and in --out).

  python tools/bench_keccak_commit.py [--log-rows 20 21 22] [--reps 7] [--out profiles/keccak_commit.json]
  --only keccak | poseidon: that path alone (for a kernel trace of its own: rocprofv3 --kernel-trace --stats -- python tools/...)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import plonky2_gpu_amd as pg
from plonky2_gpu_amd import _lib

COLS, RATE_BITS, CAP_HEIGHT = 135, 3, 4


def run_size(ctx, log_n, reps, only):
    n, n_ext = 1 << log_n, 1 << (log_n + RATE_BITS)
    rng = np.random.default_rng(log_n)
    bufs = []
    try:
        d_vals = pg.DeviceBuffer(ctx, COLS * n)
        bufs.append(d_vals)
        for c in range(0, COLS, 15):  # uploaded in slices: the host never holds the whole trace
            d_vals.upload(rng.integers(0, pg.P, size=15 * n, dtype=np.uint64), offset=c * n)
        d_work, d_lde, d_leaves = pg.DeviceBuffer(ctx, COLS * n), pg.DeviceBuffer(ctx, COLS * n_ext), pg.DeviceBuffer(ctx, COLS * n_ext)
        bufs += [d_work, d_lde, d_leaves]
        d_dig, d_cap = pg.DeviceBuffer(ctx, 8 * (n_ext - (1 << CAP_HEIGHT))), pg.DeviceBuffer(ctx, 4 << CAP_HEIGHT)
        bufs += [d_dig, d_cap]
    except _lib.Plonky2HipError as e:
        for b in bufs:
            b.free()
        return {"skipped": "device memory: %s" % e}

    def commit(hasher):
        _lib.call("gl_memcpy_d2d", d_work.ptr, d_vals.ptr, COLS * n * 8, ctx.ptr)  # the commit consumes its input
        e0, e1 = pg.Event(), pg.Event()
        e0.record(ctx)
        args = (d_work.ptr, COLS, log_n, RATE_BITS, CAP_HEIGHT, 0, 7, d_lde.ptr, d_leaves.ptr, d_dig.ptr, d_cap.ptr, ctx.ptr)
        if hasher == "poseidon":
            _lib.call("gl_commit_from_values", *args)
        else:
            _lib.call("gl_commit_from_values_h", _lib.GL_HASHER_KECCAK25, *args)
        e1.record(ctx)
        ctx.synchronize()
        return e1.elapsed_ms_since(e0)

    hashers = [h for h in ("poseidon", "keccak") if only in ("both", h)]
    for h in hashers:  # warm both paths: tables, the hashing stream, code objects
        commit(h)
        commit(h)
    ms = {h: [] for h in hashers}
    for _ in range(reps):
        for h in hashers:
            ms[h].append(commit(h))
    out = {"rows": "2^%d" % log_n, "columns": COLS, "leaves": n_ext, "reps": reps}
    for h in hashers:
        med = float(np.median(ms[h]))
        out[h] = {"median_ms": round(med, 3), "min_ms": round(min(ms[h]), 3), "max_ms": round(max(ms[h]), 3),
                  "leaves_per_s": round(n_ext / med * 1e3)}
    if len(hashers) == 2:
        out["keccak_over_poseidon"] = round(out["keccak"]["median_ms"] / out["poseidon"]["median_ms"], 4)
        out["gate_keccak_median_not_above_poseidon_median"] = out["keccak"]["median_ms"] <= out["poseidon"]["median_ms"]
    for b in bufs:
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, nargs="+", default=[20, 21, 22])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["both", "keccak", "poseidon"], default="both")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.reps < 1:
        ap.error("--reps must be at least 1")
    ctx = pg.Context(0)
    res = {"tool": "tools/bench_keccak_commit.py", "library": _lib.load().gl_version().decode(), "rate_bits": RATE_BITS, "cap_height": CAP_HEIGHT,
           "leaf_major_output": True, "sizes": [run_size(ctx, lg, a.reps, a.only) for lg in a.log_rows]}
    gates = [s["gate_keccak_median_not_above_poseidon_median"] for s in res["sizes"] if "gate_keccak_median_not_above_poseidon_median" in s]
    if gates:
        res["gate"] = all(gates)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if res.get("gate", True) else 1)


if __name__ == "__main__":
    main()
