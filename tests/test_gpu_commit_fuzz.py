"""The fixed case list of tests/fuzz_commit.py on the device: randomly shaped commits (from values and from coefficients, with and
without the leaf-major copy, every legal cap height, words >= p), their openings, and the forward / bit-reversed / inverse NTT of
the same data, against the C oracle (oracle/gl_oracle.c). What the list reaches is asserted on the CPU by tests/test_commit_fuzz.py;
longer campaigns, other seeds and the `large` branch run from the script's command line."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_commit as fc  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(fc.CASES)))
def test_commit_openings_and_transforms_equal_the_c_oracle(gpu, i):
    case = fc.fuzz_case(i)
    print("case %d (seed %d): %s" % (i, fc.SEED, fc.describe(case)))
    assert fc.check(gpu, case) is None
