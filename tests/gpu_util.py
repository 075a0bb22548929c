"""Shared helpers for the -m gpu parity tests (HIP path through the C ABI vs the CPU oracle)."""
import os

import numpy as np
import pytest

P = 0xFFFFFFFF00000001


@pytest.fixture(scope="session")
def gpu():
    import plonky2_gpu_amd as pg

    lib = pg.load()
    if lib.gl_device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (the product has no CPU fallback)")
    ctx = pg.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module", autouse=True)
def kernel_cache(request, tmp_path_factory):
    """An empty kernel cache of its own for every module that imports this fixture (the library reads the variable at every
    compile); the variable is put back behind the module."""
    cache = str(tmp_path_factory.mktemp(request.module.__name__ + "_kernel_cache"))
    saved = os.environ.get("PLONKY2_HIP_KERNEL_CACHE")
    os.environ["PLONKY2_HIP_KERNEL_CACHE"] = cache
    yield cache
    if saved is None:
        os.environ.pop("PLONKY2_HIP_KERNEL_CACHE", None)
    else:
        os.environ["PLONKY2_HIP_KERNEL_CACHE"] = saved


def bitrev_perm(log_n):
    n = 1 << log_n
    idx = np.arange(n, dtype=np.uint64)
    out = np.zeros(n, dtype=np.uint64)
    for b in range(log_n):
        out |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(log_n - 1 - b)
    return out.astype(np.int64)
