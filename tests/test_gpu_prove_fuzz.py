"""The fixed case lists of the two prove campaigns on the device: tests/fuzz_prove.py (randomly shaped small circuits against the
Python prover, oracle/prove_ref.py) and tests/fuzz_prove_c.py (three circuit families up to 2^10 rows, a third blinded, against the
C prover, oracle/prove_oracle.c). Every proof byte for byte. What the lists reach is asserted on the CPU by tests/test_prove_fuzz.py;
longer campaigns with other seeds run from the command line of the two scripts."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_prove as fp  # noqa: E402
import fuzz_prove_c as fpc  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(fp.CASES)))
def test_proof_bytes_equal_the_python_prover(gpu, i):
    case = fp.fuzz_case(i)
    print("case %d (seed %d): %s" % (i, fp.SEED, fp.describe(case)))
    assert fp.check(gpu, case) is None


@pytest.mark.parametrize("i", range(len(fpc.CASES)))
def test_proof_bytes_equal_the_c_prover(gpu, i):
    case = fpc.fuzz_case(i)
    print("case %d (seed %d): %s" % (i, fpc.SEED, fpc.describe(case)))
    assert fpc.check(gpu, case) is None
