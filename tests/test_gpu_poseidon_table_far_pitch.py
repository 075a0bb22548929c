"""gl_poseidon_table_trace at a column pitch at which the last columns lie more than 2^32 words from the first (tests/far.py): 65
records of the mixed family — STARTs and ABSORBs of every kind, so the serial pass writes and the rows kernel reads the INPUT
columns at that pitch — in 128 rows. Every column offset has to be formed in 64 bits; one formed in 32 bits, in words or in
bytes, lands in another window of the allocation and shows as a wrong value or a changed guard word, never as a fault."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import far  # noqa: E402
from far import Far  # noqa: E402
from gpu_util import gpu, kernel_cache  # noqa: E402,F401

COLUMNS, NUM_OPS, ROWS = 249, 65, 128
# far.declare() serves ONE module per process and is frozen once tests/test_gpu_far_pitch.py has been imported: this module's one
# layout is entered beside its layouts, and checked (far.check_layout) in the test and again where the matrix is made
LAYOUT = far.DECLARED.setdefault(far.Layout(COLUMNS, ROWS).key(), far.Layout(COLUMNS, ROWS))


@pytest.fixture(scope="module")
def room(gpu):
    """the module's one far allocation (48 GiB + 128 MiB); only a device too small for it anyway skips"""
    if far.device_bytes() < far.MIN_DEVICE_BYTES:
        pytest.skip("the device has less than 96 GiB")
    alloc = far.FarAllocation(gpu)
    yield alloc
    assert not alloc.live, "a test left a matrix in the far allocation"
    alloc.free()


@pytest.mark.gpu
def test_poseidon_table_trace(gpu, room):
    import plonky2_gpu_amd as pg
    import test_gpu_poseidon_table as tpt

    far.check_layout(LAYOUT)  # it can tell a cut offset from a whole one
    assert LAYOUT.stride == far.far_pitch(COLUMNS) and (COLUMNS - 1) * LAYOUT.stride >= (1 << 32) + 2
    exp = tpt._reference(NUM_OPS, 7)
    assert set(tpt._ops(NUM_OPS)[:, 0].tolist()) == set(range(9))
    d_ops = pg.DeviceBuffer.from_host(gpu, np.ascontiguousarray(tpt._ops(NUM_OPS)).reshape(-1))
    scratch = pg.DeviceBuffer(gpu, 2)
    t = Far.filled(room, LAYOUT, 21)
    try:
        assert tpt._call(gpu, d_ops.ptr, NUM_OPS, 7, t.ptr, t.stride, scratch.ptr) is None
        got = t.read("the trace")
    finally:
        t.free()
    assert (d_ops.download().reshape(NUM_OPS, 13) == tpt._ops(NUM_OPS)).all()
    assert tpt.th.first_difference(got, exp) is None
