"""Child process of tests/test_gpu_gate_fuzz.py::test_generator_variants_give_the_product_library_s_outputs: the DIAGNOSTIC build of the
library (csrc/knobs.h; the parent points PLONKY2_HIP_LIBRARY at it) reads the gate-kernel generator's switches from the environment
(PLONKY2_HIP_JIT_FUSE, _FUSE_GATES, _PEEPHOLE, _PREFETCH). The cases of tests/gate_fuzz.py named on the command line are compiled under
them and run on the compiled routes; one line "sha256 <case> <digest of the outputs>" per case, which the parent holds against the
product library's.
usage: python tests/gate_fuzz_variant_child.py <case> [<case> ...]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gate_fuzz as gf  # noqa: E402
import gate_fuzz_device as gd  # noqa: E402


def digest(outputs):
    h = hashlib.sha256()
    for _, got in outputs:
        h.update(got.tobytes())
    return h.hexdigest()


def compiled_outputs(ctx, i):
    """[(route, output)] of the compiled routes of case i, and what the generator made of it"""
    case, inp = gf.fuzz_case(i), gf.fuzz_inputs(i)
    prog = gd.program(ctx, case, inp)
    gd.compile_program(prog, case)
    outputs = []
    for name, lay in gd.layouts(ctx, case, inp):
        try:
            outputs.append((name, gd.quotient(ctx, case, inp, lay.ptrs, prog, True, lay.column_stride)))
            lay.check_unchanged()
        finally:
            lay.free()
    return outputs, gd.generated(prog)


def main():
    import plonky2_gpu_amd as pg

    ctx = pg.Context(0)
    for i in (int(a) for a in sys.argv[1:]):
        outputs, made = compiled_outputs(ctx, i)
        print("sha256", i, digest(outputs), "rewrites", made["rewrites"], flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
