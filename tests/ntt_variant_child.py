"""Child process of test_gpu_ntt.py::test_alternative_kernel_selections: the environment selects another set of NTT
kernels (read once per process by the library), the transforms must equal the oracle's all the same, at stride n and at a padded
stride (tests/strided.py: guarded and padded buffers, the matrix of test_gpu_strides.py::test_ntt_padded_strides cut to one stride per
order: n + 2 forward and bit-reversed, 3n inverse)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

import plonky2_gpu_amd as pg  # noqa: E402
import strided  # noqa: E402


def bitrev_perm(bits):
    idx = np.arange(1 << bits, dtype=np.uint64)
    out = np.zeros_like(idx)
    for b in range(bits):
        out |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
    return out.astype(np.int64)


def main():
    gpu = pg.Context(0)
    for log_n in (9, 13, 16, 20, 21, 22):
        x = oracle.random_field((3, 1 << log_n), seed=9100 + log_n)
        exp = oracle.canon(oracle.fft_batch(x, threads=2))
        f = pg.fft_with_options(gpu, x)
        assert (f == exp).all(), ("forward", log_n)
        assert (pg.ifft_with_options(gpu, f) == x).all(), ("inverse", log_n)
        b = pg.fft_with_options(gpu, x[1], bit_reversed=True)
        assert (b == exp[1][bitrev_perm(log_n)]).all(), ("bit-reversed", log_n)
    for log_n, rate_bits in ((14, 3), (20, 1), (21, 1), (22, 0)):
        c = oracle.random_field((2, 1 << log_n), seed=9200 + log_n)
        got = pg.coset_lde_bit_reversed(gpu, c, rate_bits)
        perm = bitrev_perm(log_n + rate_bits)
        for i in range(2):
            assert (got[i] == oracle.canon(oracle.coset_lde(c[i], rate_bits))[perm]).all(), ("lde", log_n)
    for log_n, n_polys in strided.NTT_SHAPES:
        case = strided.ntt_case(oracle, log_n, n_polys)
        for order in ("forward", "bit_reversed", "inverse"):
            strided.check_ntt(gpu, case, order, strided.ntt_strides(log_n, order)[-1:] if order == "inverse" else strided.ntt_strides(log_n, order)[:1])
    for log_n, rate_bits in ((12, 3), (16, 3), (20, 1), (22, 1)):  # the coset LDE from a padded source into a padded destination
        n, n_ext = 1 << log_n, 1 << (log_n + rate_bits)
        c = oracle.random_field((2, n), seed=9250 + log_n)
        exp = oracle.canon(oracle.coset_lde_batch(c, rate_bits, threads=2))[:, bitrev_perm(log_n + rate_bits)]
        src = strided.Strided(gpu, c, n + 2)
        dst = strided.Strided(gpu, np.broadcast_to(strided.filler(n_ext, 7), (2, n_ext)), n_ext + 48)
        pg._lib.call("gl_coset_lde_batch", src.ptr, dst.ptr, 2, log_n, rate_bits, 7, n + 2, n_ext + 48, gpu.ptr)
        assert (dst.polys(("lde", log_n)) == exp).all(), ("lde at padded strides", log_n)
        assert (src.polys(("lde source", log_n)) == c).all(), ("lde source", log_n)
        src.free()
        dst.free()
    print("ok")


if __name__ == "__main__":
    main()
