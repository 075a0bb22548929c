"""Canonical form with the subtraction deferred (gl_field.h canon_f / canon_fix): one compare per value flags a superset of the values
>= p, one branch per group guards the exact subtraction. The pair is checked through gl_debug_field_op 28-30, whose results are stored
as canon_fix left them. (The passes' tails do NOT use the pair: measured, it did not pay, LABNOTES 17; they keep gl::canon.) Then whole
transforms through the kernels whose butterflies subtract in four instructions, on inputs full of the field's edge representatives:
every stored word must be canonical and equal to the oracle's."""
import numpy as np
import pytest

from gpu_util import P, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
EDGE = [P - 1, P, P + 1, M64, 0xFFFFFFFF00000000] + [(0xFFFFFFFF << 32) | low for low in (0, 1, 0xFFFFFFFF)]


def run_op(gpu, op, a, b):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    da, db = pg.DeviceBuffer.from_host(gpu, a), pg.DeviceBuffer.from_host(gpu, b)
    do = pg.DeviceBuffer(gpu, len(a))
    _lib.call("gl_debug_field_op", op, da.ptr, db.ptr, do.ptr, len(a), gpu.ptr)
    return do.download().tolist()


def test_canon_group_flagged_first_in_the_middle_and_last(gpu):
    """The group canonicalises x, y and x ^ y; op 28 + k returns member k. Every edge value as each member beside random (unflagged)
    neighbours, beside other edge values, a whole wavefront of them, and random u64."""
    rng = np.random.default_rng(51)
    rnd = [int(v) for v in rng.integers(0, 1 << 64, size=4096, dtype=np.uint64, endpoint=False)]
    xy = []
    for i, v in enumerate(EDGE):
        for r in rnd[16 * i:16 * i + 16]:
            xy += [(v, r), (r, v), (r, r ^ v)]          # flagged first, in the middle, last
        xy += [(v, w) for w in EDGE] + [(v ^ w, w) for w in EDGE]
        xy += [(v, v ^ P)] * 64 + [(v, 0)] * 64        # whole wavefronts
    xy += list(zip(rnd[:2048], rnd[2048:]))
    x = np.array([p[0] for p in xy], dtype=np.uint64)
    y = np.array([p[1] for p in xy], dtype=np.uint64)
    assert run_op(gpu, 28, x, y) == [a % P for a, _ in xy]
    assert run_op(gpu, 29, x, y) == [b % P for _, b in xy]
    assert run_op(gpu, 30, x, y) == [(a ^ b) % P for a, b in xy]


@pytest.fixture(scope="module")
def edge_columns():
    """log_n -> three columns drawn from {0, 1, p - 1, p, 2^64 - 1} mixed with random u64, and the oracle's forward and inverse
    transforms of their canonical form (computed once)."""
    cache = {}

    def get(oracle, log_n):
        if log_n not in cache:
            rng = np.random.default_rng(5200 + log_n)
            n = 1 << log_n
            pick = rng.integers(0, 8, size=(3, n))
            edge = np.array([0, 1, P - 1, P, M64], dtype=np.uint64)[np.minimum(pick, 4)]
            x = np.where(pick < 5, edge, rng.integers(0, 1 << 64, size=(3, n), dtype=np.uint64, endpoint=False))
            c = oracle.canon(x)
            cache[log_n] = (x, oracle.canon(oracle.fft_batch(c, threads=3)), oracle.canon(oracle.fft_batch(c, inverse=True, threads=3)))
        return cache[log_n]

    return get


# the smallest sizes at which the planner picks each kernel the butterflies run in: the column pass with G = 1, 2, 4 in front of the
# natural-order row pass (2^18, 2^19, 2^20) and the final column pass of the two-pass plan (2^22)
@pytest.mark.parametrize("n_cols", [1, 3])
@pytest.mark.parametrize("log_n", [18, 19, 20, 22])
def test_transforms_of_edge_representatives_are_canonical_and_right(gpu, oracle, edge_columns, log_n, n_cols):
    import plonky2_gpu_amd as pg
    from plonky2_gpu_amd import _lib

    x, exp_f, exp_i = edge_columns(oracle, log_n)
    n = 1 << log_n
    for inverse, exp in ((0, exp_f), (1, exp_i)):
        buf = pg.DeviceBuffer.from_host(gpu, np.ascontiguousarray(x[:n_cols]).reshape(-1))
        _lib.call("gl_ntt_batch", buf.ptr, n_cols, log_n, n, inverse, 0, gpu.ptr)
        out = buf.download().reshape(n_cols, n)
        assert (out < np.uint64(P)).all(), ("a stored word is not canonical", inverse)
        assert (out == exp[:n_cols]).all(), ("inverse" if inverse else "forward")
