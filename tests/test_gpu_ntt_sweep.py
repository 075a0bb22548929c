"""The two-pass plans of gl_ntt_batch with alternating sweep direction (csrc/ntt.hip sweep_of_pass, csrc/ntt_direct.hip
tile_of): sizes 2^16 .. 2^21, batches 1, 3, 18, 64 and 65 polynomials, natural, inverse and
bit-reversed order, padded strides, two consecutive calls on the same buffer; every result equals the C oracle's bit for bit.

A sweep that mirrored loads and stores differently would swap polynomials (every polynomial here is different, polynomial 0 is
all p - 1); the buffers are guarded and padded (tests/strided.py). 18 polynomials are the shape that leaves workgroups of the column
pass with different tile counts (per_b = 4 at 64 column tiles: 5, 5, 4, 4); 65 leaves one polynomial for a second tile row.

The FIRST call on a buffer is compared with the oracle in every polynomial. The SECOND call on the same buffer is compared in
every polynomial where the expectation costs nothing more (the inverse of the forward transform must be the input), and otherwise
in three watched polynomials (first, middle, last): a full oracle transform of every intermediate would double the test's CPU
time, and a mirrored or swapped polynomial shows at the ends and in the middle."""
import numpy as np
import pytest

import strided
from gpu_util import P, gpu  # noqa: F401
from strided import Strided, bitrev_perm

pytestmark = pytest.mark.gpu

SIZES = [16, 17, 18, 19, 20, 21]
BATCHES = [1, 3, 18, 64, 65]


def _L():
    from plonky2_gpu_amd import _lib

    return _lib


def _differ(got, exp):
    return np.flatnonzero((got != exp).any(axis=1))[:8].tolist()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("log_n", SIZES)
def test_alternating_sweeps_against_the_oracle(gpu, oracle, log_n, batch):
    L = _L()
    n = 1 << log_n
    x = oracle.random_field((batch, n), seed=7100 + 8 * log_n + batch)
    x[0, :] = np.uint64(P - 1)
    if batch > 1:
        strided.lift_some(x, 1, 7200 + log_n)
    xc = oracle.canon(x)
    exp_f = oracle.canon(oracle.fft_batch(xc.copy(), threads=8))
    perm = bitrev_perm(log_n)
    exp_r = exp_f[:, perm]
    watch = sorted({0, batch // 2, batch - 1})

    # natural order at stride 2n (the inverse wants stride % n == 0), then the inverse of that in the same buffer: the second call's
    # first pass starts on what the first call's last pass wrote last
    s = Strided(gpu, x, 2 * n)
    L.call("gl_ntt_batch", s.ptr, batch, log_n, 2 * n, 0, 0, gpu.ptr)
    f = s.polys(("forward", 2 * n))
    assert (f == exp_f).all(), ("forward, stride 2n", _differ(f, exp_f))
    L.call("gl_ntt_batch", s.ptr, batch, log_n, 2 * n, 1, 0, gpu.ptr)
    back = s.polys(("inverse of the forward, same buffer", 2 * n))
    s.free()
    exp_b = oracle.canon(oracle.fft_batch(exp_f[watch].copy(), inverse=True, threads=8))
    assert (exp_b == xc[watch]).all()
    assert (back == xc).all(), ("inverse, stride 2n", _differ(back, xc))

    # the inverse of the INPUT at stride 3n, twice in a row in the same buffer
    exp_i = oracle.canon(oracle.fft_batch(xc.copy(), inverse=True, threads=8))
    s = Strided(gpu, x, 3 * n)
    L.call("gl_ntt_batch", s.ptr, batch, log_n, 3 * n, 1, 0, gpu.ptr)
    got = s.polys(("inverse", 3 * n))
    assert (got == exp_i).all(), ("inverse, stride 3n", _differ(got, exp_i))
    L.call("gl_ntt_batch", s.ptr, batch, log_n, 3 * n, 1, 0, gpu.ptr)
    got = s.polys(("inverse twice", 3 * n))
    s.free()
    exp_ii = oracle.canon(oracle.fft_batch(exp_i[watch].copy(), inverse=True, threads=8))
    assert (got[watch] == exp_ii).all(), ("inverse twice, stride 3n", _differ(got[watch], exp_ii))
    del exp_i

    # natural and bit-reversed order at the smallest legal pad and at a pitch that is no power of two, twice in a row each
    exp_ff = oracle.canon(oracle.fft_batch(exp_f[watch].copy(), threads=8))
    exp_rr = oracle.canon(oracle.fft_batch(exp_r[watch].copy(), threads=8))[:, perm]
    for stride in (n + 2, n + 48):
        s = Strided(gpu, x, stride)
        L.call("gl_ntt_batch", s.ptr, batch, log_n, stride, 0, 0, gpu.ptr)
        got = s.polys(("forward", stride))
        assert (got == exp_f).all(), ("forward, stride", stride, _differ(got, exp_f))
        L.call("gl_ntt_batch", s.ptr, batch, log_n, stride, 0, 0, gpu.ptr)
        got = s.polys(("forward twice", stride))
        s.free()
        assert (got[watch] == exp_ff).all(), ("forward twice, stride", stride, _differ(got[watch], exp_ff))

        s = Strided(gpu, x, stride)
        L.call("gl_ntt_batch", s.ptr, batch, log_n, stride, 0, 1, gpu.ptr)
        got = s.polys(("bit-reversed", stride))
        assert (got == exp_r).all(), ("bit-reversed, stride", stride, _differ(got, exp_r))
        L.call("gl_ntt_batch", s.ptr, batch, log_n, stride, 0, 1, gpu.ptr)
        got = s.polys(("bit-reversed twice", stride))
        s.free()
        assert (got[watch] == exp_rr).all(), ("bit-reversed twice, stride", stride, _differ(got[watch], exp_rr))
