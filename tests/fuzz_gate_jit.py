"""Differential campaign for the gate-kernel generator (csrc/gate_jit.hip): random gate lists drawn from the catalog of tests/gate_fuzz.py
(all twenty gate kinds, several parameter sets each), in one or two selector groups, compiled with random generator settings (gates per
fused unit, statements a load is issued ahead, waves per SIMD, fused or one function per gate, peephole pass on or off) and run through
gl_compute_quotient_polys on the inputs tests/gate_fuzz.py draws — leaves, k_is, challenges and hash of uniform u64 words with edge words
sprinkled in (0..5, 2^32 +- 1, 2^63, p - 4 .. p + 3, 2^64 - 1 ...), honest selector words in half of the rows. The INTERPRETER, which
executes the programs as written, must give what the CPU reference gives (gate_fuzz.quotient_of: oracle/gates_ref.py under
oracle/plonk_ref.py), and the compiled kernel must give the same under the default setting and under a random one. The fixed list of
tests/gate_fuzz.py is what the suite runs (tests/test_gpu_gate_fuzz.py); this script goes on drawing. Run it on a GPU box:
    python tests/fuzz_gate_jit.py [cases=40] [seed=1]
Prints one line per case and a JSON summary; exits non-zero on the first mismatch."""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# the generator's switches are read by the DIAGNOSTIC build of the library only (csrc/knobs.h)
os.environ.setdefault("PLONKY2_HIP_LIBRARY", os.path.join(ROOT, "plonky2_gpu_amd", "libplonky2_hip_debug.so"))

import plonky2_gpu_amd as pg  # noqa: E402

import gate_fuzz as gf  # noqa: E402
import gate_fuzz_device as gd  # noqa: E402

P = gf.P
EDGES = gf.EDGES
CATALOG = gf.CATALOG
KNOBS = ("PLONKY2_HIP_JIT_FUSE", "PLONKY2_HIP_JIT_PEEPHOLE", "PLONKY2_HIP_JIT_FUSE_GATES", "PLONKY2_HIP_JIT_PREFETCH", "PLONKY2_HIP_JIT_WAVES")


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    ctx = pg.Context(0)
    t0 = time.time()
    for number in range(cases):
        count = rng.randint(2, 9)
        kinds = [rng.choice(CATALOG[:-1]) for _ in range(count)]
        if rng.random() < 0.15:
            kinds[rng.randrange(count)] = CATALOG[-1]  # the Poseidon gate: 4 000 operations, now and then
        two_groups = count >= 4 and rng.random() < 0.5
        case = gf.gate_list_case(kinds, 2 if two_groups else 1, rng.choice([1, 2, 2, 3]), rng.choice([2, 3, 4]), 8, index=number)
        inp = gf.draw_inputs(nrng, case, rng.choice(gf.EDGE_SHARES))
        reference = gf.quotient_of(case, inp)
        lay = gd.LeafMajor(ctx, inp)
        prog = gd.program(ctx, case, inp)
        want = gd.quotient(ctx, case, inp, lay.ptrs, prog, False)  # the interpreter
        ok = bool((want == reference).all())
        settings = [{}]  # the default generator
        s = {"PLONKY2_HIP_JIT_FUSE_GATES": str(rng.choice([1, 2, 3, 5, 8, 16])), "PLONKY2_HIP_JIT_PREFETCH": str(rng.choice([0, 3, 16, 100])),
             "PLONKY2_HIP_JIT_WAVES": str(rng.choice([2, 3, 4]))}
        if rng.random() < 0.25:
            s = {"PLONKY2_HIP_JIT_FUSE": "0", "PLONKY2_HIP_JIT_PEEPHOLE": rng.choice(["0", "1"])}
        elif rng.random() < 0.2:
            s["PLONKY2_HIP_JIT_PEEPHOLE"] = "0"
        settings.append(s)
        for env in settings:
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            gd.compile_program(prog, case)
            got = gd.quotient(ctx, case, inp, lay.ptrs, prog, True)
            ok &= bool((got == want).all()) and bool((got == reference).all())
        for k in KNOBS:
            os.environ.pop(k, None)
        lay.free()
        print(f"case {number:3d} {'ok  ' if ok else 'FAIL'} gates={[k for k, _ in kinds]} groups={case['groups']} nch={case['num_challenges']} "
              f"rows={case['n_ext']} second={settings[1]}", flush=True)
        if not ok:
            print(json.dumps(dict(result="MISMATCH", case=number, seed=seed, kinds=kinds, settings=settings[1],
                                  interpreter_equals_reference=bool((want == reference).all()))))
            sys.exit(1)
    print(json.dumps(dict(result="all equal", cases=cases, seed=seed, seconds=round(time.time() - t0, 1))))


if __name__ == "__main__":
    main()
