"""gl_compute_quotient_polys on a case of tests/gate_fuzz.py (TEST INFRASTRUCTURE ONLY), shared by tests/test_gpu_gate_fuzz.py, its child
process tests/gate_fuzz_variant_child.py and the campaign script tests/fuzz_gate_jit.py. A case runs on four ROUTES: the interpreter
(a GlGateProgram in device memory) or the compiled kernel (gl_gate_kernel_build), each on leaf-major leaves [n_ext][leaf_len] or on
column-major leaves [leaf_len][pitch] in a guarded, padded buffer (tests/strided.py)."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gate_fuzz as gf  # noqa: E402
from strided import Strided  # noqa: E402

MARKER = 0xFFFFFFFFABCD0000  # no canonical word: what an output buffer holds before a call that must not write it
LEAVES = ("wires", "cs", "zs")


def program(ctx, case, inp):
    import plonky2_gpu_amd as pg

    return pg.GateProgram(ctx, case["programs"], case["selector_indices"], case["groups"], inp["pih"], immediates=case["immediates"] or None)


def compile_program(prog, case):
    """-> seconds in gl_gate_kernel_build (hiprtc, or the kernel cache)"""
    import time

    t0 = time.perf_counter()
    prog.compile(case["num_gate_constraints"], case["num_challenges"])
    return time.perf_counter() - t0


def generated(prog):
    """what the generator made of the table, counted in gl_gate_kernel_source: gates per unit, whether a unit takes a bias off, how
    many range checks were rewritten (gate_jit.hip, rewrite 2)"""
    units = prog.kernel_source().split('extern "C" __global__')[1:]
    import re

    return dict(sums=len(set(re.findall(r"gj_acc\(l(\d+)l,", prog.kernel_source()))),  # the accumulators of the fused generator's sums
                gates_per_unit=[u.count("gl::DotCol2 ga") for u in units],  # (the fused generator's per-gate accumulators)
                bias=any("g_bias[c * NGU + " in u for u in units), rewrites=prog.kernel_source().count("gl::mul_add_small<1>("))


def quotient(ctx, case, inp, ptrs, prog, compiled, column_stride=0, out=None, num_gate_constraints=None):
    """one call. `ptrs`: device addresses of the three leaf arrays and of k_is; `out`: a DeviceBuffer to use (else a fresh one, freed)
    -> uint64 [num_challenges][rows_read]"""
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    a, b, g = (np.ascontiguousarray(np.array(inp[k], dtype=np.uint64)) for k in ("alphas", "betas", "gammas"))
    pih = np.array(inp["pih"], dtype=np.uint64)
    nch, rows = case["num_challenges"], case["rows_read"]
    work = pg.DeviceBuffer(ctx, nch * rows) if compiled else None
    ngc = case["num_gate_constraints"] if num_gate_constraints is None else num_gate_constraints
    args = _lib.GlQuotientArgs(ptrs["wires"], ptrs["cs"], ptrs["zs"], case["wires_len"], case["cs_len"], case["zs_len"], ptrs["k_is"], None,
                               b.ctypes.data, g.ctypes.data, a.ctypes.data, case["num_constants"], gf.ROUTED, nch, ngc, case["degree_bits"],
                               gf.RATE_BITS, case["quotient_degree_factor"], 7, None if compiled else ctypes.pointer(prog.struct), column_stride,
                               prog.kernel if compiled else None, pih.ctypes.data if compiled else None, work.ptr if compiled else None)
    mine = out is None
    if mine:
        out = pg.DeviceBuffer(ctx, nch * rows)
    try:
        _lib.call("gl_compute_quotient_polys", ctypes.byref(args), out.ptr, ctx.ptr)
        return out.download().copy().reshape(nch, rows)
    finally:
        if mine:
            out.free()
        if work is not None:
            ctx.synchronize()
            work.free()


class LeafMajor:
    """the three commitments' leaves as the library's leaf-major rows, and k_is"""

    def __init__(self, ctx, inp):
        import plonky2_gpu_amd as pg

        self.inp = inp
        self.bufs = {k: pg.DeviceBuffer.from_host(ctx, np.ascontiguousarray(inp[k]).reshape(-1)) for k in LEAVES + ("k_is",)}
        self.ptrs = {k: b.ptr for k, b in self.bufs.items()}
        self.column_stride = 0

    def check_unchanged(self):
        for k, b in self.bufs.items():
            assert (b.download() == np.ascontiguousarray(self.inp[k]).reshape(-1)).all(), ("the call wrote to its input", k)

    def free(self):
        for b in self.bufs.values():
            b.free()


class ColumnMajor:
    """the leaves the kernel reads (the first n << qdb) as columns at distance `pitch`, between guards and pads"""

    def __init__(self, ctx, case, inp, pitch):
        import plonky2_gpu_amd as pg

        self.inp, self.rows = inp, case["rows_read"]
        self.cols = {k: Strided(ctx, np.ascontiguousarray(inp[k][: self.rows].T), pitch) for k in LEAVES}
        self.k_is = pg.DeviceBuffer.from_host(ctx, np.ascontiguousarray(inp["k_is"]))
        self.ptrs = dict({k: s.ptr for k, s in self.cols.items()}, k_is=self.k_is.ptr)
        self.column_stride = pitch

    def check_unchanged(self):
        for k, s in self.cols.items():
            assert (s.polys(k) == self.inp[k][: self.rows].T).all(), ("the call wrote to its input", k)  # (.polys checks guards and pads)
        assert (self.k_is.download() == self.inp["k_is"]).all()

    def free(self):
        for s in self.cols.values():
            s.free()
        self.k_is.free()


def layouts(ctx, case, inp):
    """the leaf-major layout and the column-major one at the smallest legal pitch and at a padded one"""
    yield "leaf-major", LeafMajor(ctx, inp)
    for pitch in (case["rows_read"], case["rows_read"] + 6):
        yield "column-major, pitch %d" % pitch, ColumnMajor(ctx, case, inp, pitch)


def run_routes(ctx, case, inp, prog, compiled_too=True):
    """every route -> [(route name, output)], the inputs, guards and pads checked after every call"""
    out = []
    for name, lay in layouts(ctx, case, inp):
        try:
            for compiled in ((False, True) if compiled_too else (False,)):
                got = quotient(ctx, case, inp, lay.ptrs, prog, compiled, lay.column_stride)
                lay.check_unchanged()
                out.append((("compiled" if compiled else "interpreter") + ", " + name, got))
        finally:
            lay.free()
    return out


def lifted_inputs(inp, seed):
    """every word that has a second representative word + p is that one (tests/representatives.lift with frac=1.0)"""
    import representatives as rep

    rng = np.random.default_rng(seed)
    out, count = {}, 0
    for k in LEAVES + ("k_is",):
        out[k], more = rep.lift(np.asarray(inp[k], dtype=np.uint64) % np.uint64(gf.P), rng, frac=1.0)
        count += more
    for k in ("alphas", "betas", "gammas", "pih"):
        out[k] = [rep.lift_scalar(v) for v in inp[k]]
    return out, count
