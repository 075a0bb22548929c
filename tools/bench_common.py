"""What the bench_*.py tools share: the proofs' FRI parameters, the summary of a list of times, and a kernel cache of a tool's own.
The timing loops (wall, timed, timed_alternating) differ on purpose and stay with their tools."""
import os
import shutil
import tempfile

import numpy as np


def fast_config_fri_params(degree_bits):
    """FriConfig::fri_params of standard_fast_config (plonky2/src/fri/reduction_strategies.rs:38-49)"""
    rate_bits, cap_height, arity, final_poly_bits = 1, 4, 4, 5
    arities, db = [], degree_bits
    while db > final_poly_bits and db + rate_bits - arity >= cap_height:
        arities.append(arity)
        db -= arity
    return dict(rate_bits=rate_bits, cap_height=cap_height, proof_of_work_bits=16, num_query_rounds=84, reduction_arity_bits=arities, hiding=False)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4), "max_ms": round(float(max(ms)), 4)}


class TemporaryKernelCache:
    """an empty kernel cache of its own while the block runs; `env`: further variables set for the block (AMD_COMGR_CACHE="0", so
    that a cold compile is hiprtc's own time). Everything is put back and the directory removed behind the block."""

    def __init__(self, prefix, env=None):
        self.prefix, self.env = prefix, dict(env or {})

    def __enter__(self):
        self.dir = tempfile.mkdtemp(prefix=self.prefix + "_kernel_cache_")
        self.env["PLONKY2_HIP_KERNEL_CACHE"] = self.dir
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        return self.dir

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        shutil.rmtree(self.dir, ignore_errors=True)
