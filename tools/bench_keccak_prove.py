#!/usr/bin/env python3
"""A whole proof with Keccak trees (KeccakGoldilocksConfig, gl_circuit_create_h) against the same proof with Poseidon trees, same
device, same minute: the synthetic circuit of bench.py's prove() leg (tools/synth_circuit.py: n = 2^18, 234 wires, 80 routed, the
25-gate table of the ed25519 circuit, FRI arities [4, 4, 4, 4] — all >= 2, as a Keccak circuit needs). Both handles are created
and warmed, then Poseidon and Keccak proofs alternate; wall time around each gl_prove (it ends synchronised). Median and min-max
per hasher, their ratio, and the h_stage_ms breakdown of one further proof each. Oracle-free; one JSON line on stdout (and --out).

  python tools/bench_keccak_prove.py [--degree-bits 18] [--wires 234] [--reps 7] [--out profiles/keccak_prove.json]
  --only keccak | poseidon: that path alone (for a kernel trace of its own: rocprofv3 --kernel-trace --stats -- python tools/...)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import plonky2_gpu_amd as pg
import synth_circuit
from plonky2_gpu_amd import _lib
from plonky2_gpu_amd.challenger import hash_no_pad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree-bits", type=int, default=18)
    ap.add_argument("--wires", type=int, default=234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["both", "keccak", "poseidon"], default="both")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.reps < 1:
        ap.error("--reps must be at least 1")
    ctx = pg.Context(0)
    table = "ed25519" if a.wires == 234 else "mini"
    circuit, wires, pis = synth_circuit.make(a.degree_bits, num_wires=a.wires, num_routed=80, num_constants=8, seed=1, gate_table=table)
    synth_circuit.set_public_input_row(wires, hash_no_pad(ctx, pis))
    arities = list(circuit["fri_params"]["reduction_arity_bits"])
    if any(ab < 2 for ab in arities):
        raise SystemExit("bench_keccak_prove: FRI arities %s hold a reduction below 2, which no Keccak circuit can have" % arities)
    hashers = [h for h in ("poseidon", "keccak") if a.only in ("both", h)]
    d_wires = pg.DeviceBuffer.from_host(ctx, np.ascontiguousarray(wires))
    ncs = {h: pg.NativeCircuit(ctx, dict(circuit, circuit_digest=None), hasher=h) for h in hashers}

    def prove(h, timing=None):
        t0 = time.perf_counter()
        data = ncs[h].prove_bytes(d_wires, pis, timing)
        return (time.perf_counter() - t0) * 1e3, data

    first = {}
    for h in hashers:  # warm both: tables, the hashing stream, code objects, the handle's buffer pool
        first[h] = prove(h)[1]
        prove(h)
    ms = {h: [] for h in hashers}
    for _ in range(a.reps):
        for h in hashers:
            t, data = prove(h)
            if data != first[h]:
                raise SystemExit("bench_keccak_prove: the %s proof is not deterministic" % h)
            ms[h].append(t)
    res = {"tool": "tools/bench_keccak_prove.py", "library": _lib.load().gl_version().decode(),
           "workload": "synthetic circuit of bench.py's prove(): n=2^%d, %d wires (80 routed), gate table %s, 2 challenges, rate 8, cap_height 4, "
                       "FRI arities %s, 28 queries, 16 PoW bits; witness and preprocessed commitment resident" % (a.degree_bits, a.wires, table, arities),
           "reps": a.reps}
    for h in hashers:
        timing = {}
        prove(h, timing)
        stages = {k: round(v, 3) for k, v in timing.items()}
        res[h] = {"median_ms": round(float(np.median(ms[h])), 3), "min_ms": round(min(ms[h]), 3), "max_ms": round(max(ms[h]), 3),
                  "proof_bytes": len(first[h]), "stage_ms": stages, "largest_stage": max(stages, key=stages.get)}
        parsed = pg.serialization.proof_from_bytes(first[h], circuit, hasher=ncs[h].hasher)
        if pg.serialization.proof_to_bytes(parsed, hasher=ncs[h].hasher) != first[h]:
            raise SystemExit("bench_keccak_prove: the %s proof does not round-trip through the wire format" % h)
    if len(hashers) == 2:
        res["keccak_over_poseidon"] = round(res["keccak"]["median_ms"] / res["poseidon"]["median_ms"], 4)
    for nc in ncs.values():
        nc.close()
    d_wires.free()
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
