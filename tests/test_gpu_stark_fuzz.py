"""gl_stark_quotient_polys on random programs and random words, and gl_stark_create's validator against the reference validator.

The quotient: for every description of tests/stark_fuzz.py's fixed list (random programs of 8 .. 4000 instructions over 1 / 5 / 70
columns, quotient degree factors 1 .. 16 with 1 .. 4 challenges, 0 .. 3 permutation pairs of 0 .. 3 column pairs, 0 / 1 / 3 public
inputs, 2 .. 16 rows) the trace "LDE", the Z "LDE", the public inputs, alphas, betas and gammas are uniform random words — neither
the device nor tests/stark_ref.py's compute_quotient_polys needs them to be low-degree extensions — and all num_challenges x
(n << qdb) coefficients are compared bit for bit. What the list reaches is asserted on the CPU (tests/test_stark_fuzz.py).

The validator: mutants of the generated programs, one field of one instruction or one immediate changed to a random or a boundary
value; gl_stark_create must refuse exactly those that tests/stark_ref.py's validate_program refuses. No kernel is launched for a
refused description, and an accepted mutant is only created and destroyed: nothing here runs a program that was not validated."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stark_fuzz as sf  # noqa: E402
import stark_instances as si  # noqa: E402
import stark_ref as sr  # noqa: E402
from gpu_util import gpu  # noqa: E402,F401
from strided import Strided  # noqa: E402

P = sr.P


def _desc(case, instrs=None, immediates=None):
    from plonky2_gpu_amd.stark import StarkDesc

    s = case["stark"]
    desc = StarkDesc(case["degree_bits"], s.num_columns, s.num_public_inputs, s.constraint_degree, case["num_challenges"],
                     si.fri_params(rate_bits=case["rate_bits"]), s.instrs if instrs is None else instrs, s.immediates, s.pairs)
    if immediates is not None:
        desc.immediates = list(immediates)  # as they are: StarkDesc reduces its own, and the library must
    return desc


@pytest.mark.gpu
@pytest.mark.parametrize("i", sf.CASES)
def test_quotient_of_a_random_program_on_random_words(gpu, i):
    import plonky2_gpu_amd as pg

    case = sf.fuzz_case(i)
    s = case["stark"]
    trace, zs, sets, alphas, pis = sf.fuzz_inputs(i, case)
    exp = sf.reference_quotient(case, trace, zs, sets, alphas, pis)
    shape = dict(seed=sf.SEED + i, columns=s.num_columns, public_inputs=s.num_public_inputs, constraint_degree=s.constraint_degree,
                 challenges=case["num_challenges"], degree_bits=case["degree_bits"], rate_bits=case["rate_bits"], instructions=len(s.instrs),
                 pairs=s.pairs)
    qdb = (sr.quotient_degree_factor(s) - 1).bit_length()
    assert exp.shape == (case["num_challenges"], 1 << (case["degree_bits"] + qdb)) and exp.any(axis=1).all(), shape
    ns = pg.NativeStark(gpu, _desc(case))  # every generated description is accepted: nothing is filtered by what the device says
    try:
        n_ext = trace.shape[1]
        for stride in (n_ext, n_ext + 6):
            t = Strided(gpu, trace, stride)
            z = Strided(gpu, zs, stride) if zs is not None else None
            got = ns.quotient_polys(t.ptr, z.ptr if z else None, stride, alphas, sets, pis)
            assert (t.polys() == trace).all() and (z is None or (z.polys() == zs).all())  # guards and pads: only read
            bad = np.argwhere(got != exp)
            assert bad.size == 0, ("column pitch", stride, "first (challenge, coefficient) that differs", bad[0].tolist(), len(bad), shape)
            t.free()
            if z:
                z.free()
    finally:
        ns.close()


# ---------------------------------------------------------------- the validator
def _boundaries(case):
    cols = case["stark"].num_columns
    return [3, 4, 63, 64, max(cols - 1, 0), cols, 14, 15, 65535, 0, 1, 2]


IMMEDIATE_MUTANTS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 31) + 1, P - 1, P, P + 1, P + (1 << 31), (1 << 64) - 1]


def _mutants(count, seed):
    """(case, instrs, immediates) with one field of one instruction or one immediate changed"""
    rng = np.random.default_rng(seed)
    short = [i for i in sf.CASES if sf.LENGTHS[i] <= 400]
    out = []
    while len(out) < count:
        case = sf.fuzz_case(short[int(rng.integers(0, len(short)))])
        s = case["stark"]
        instrs, imms = s.instrs.copy(), list(s.immediates)
        if imms and rng.random() < 0.2:
            k = int(rng.integers(0, len(imms)))
            imms[k] = IMMEDIATE_MUTANTS[int(rng.integers(0, len(IMMEDIATE_MUTANTS)))] if rng.random() < 0.7 else int(rng.integers(0, 1 << 64, dtype=np.uint64))
        else:
            pc, field = int(rng.integers(0, len(instrs))), int(rng.integers(0, 4))
            b = _boundaries(case)
            instrs[pc, field] = b[int(rng.integers(0, len(b)))] if rng.random() < 0.7 else int(rng.integers(0, 1 << 16))
        out.append((case, instrs, imms))
    return out


def _create(gpu, desc):
    """None if gl_stark_create accepts (the handle is destroyed), else its message"""
    import plonky2_gpu_amd as pg

    try:
        ns = pg.NativeStark(gpu, desc)
    except pg.Plonky2HipError as e:
        assert e.code == pg.GL_E_INVALID and str(e).strip(), (e.code, str(e))
        return str(e)
    ns.close()
    return None


@pytest.mark.gpu
def test_create_refuses_exactly_what_the_reference_validator_refuses(gpu):
    refused = accepted = 0
    for k, (case, instrs, imms) in enumerate(_mutants(200, seed=4242)):
        s = case["stark"]
        try:
            sr.validate_program(instrs, imms, s.num_columns, s.num_public_inputs)
            want = None
        except ValueError as e:
            want = str(e)
        got = _create(gpu, _desc(case, instrs, imms))
        changed = np.argwhere(instrs != s.instrs).tolist(), [(j, hex(v)) for j, (v, w) in enumerate(zip(imms, s.immediates)) if v != w]
        assert (got is None) == (want is None), ("mutant", k, "reference", want, "library", got, "changed", changed)
        refused += want is not None
        accepted += want is None
    assert refused >= 40 and accepted >= 40, (refused, accepted)  # both answers are exercised


def _acc_program(*accs, accr=(0,)):
    """LOAD_WIRE r0 <- column 0; ACC q r0 weight ..; ACCR r1 <- q ..; EMIT r1. Returns (instrs, immediates)"""
    imms = sorted({w for _, w in accs})
    rows = [[sr.LOAD_WIRE, 0, 0, 0]] + [[sr.ACC, q, 0, imms.index(w)] for q, w in accs] + [[sr.ACCR, 1, q, 0] for q in accr] + [[sr.EMIT, 0, 1, 0]]
    return np.array(rows, dtype=np.uint16), imms


W = (1 << 32) - 1
ACC_BOUND_CASES = [
    # two weights whose bound 3 (2^32 - 1) + (2^32 - 1)^2 = 2^64 + 2^32 - 2 wraps 64 bits to a small number
    ("3 then 2^32 - 1", _acc_program((0, 3), (0, W)), "2^63"),
    ("2^32 - 1 then 3", _acc_program((0, W), (0, 3)), "2^63"),
    ("2^31 alone", _acc_program((0, 1 << 31)), None),  # 2^31 (2^32 - 1) < 2^63: the largest sum the contract allows
    ("2^31 then 1", _acc_program((0, 1 << 31), (0, 1)), "2^63"),
    ("2^31 on two accumulators", _acc_program((0, 1 << 31), (1, 1 << 31), accr=(0, 1)), None),  # the bounds are per accumulator
    ("2^31, ACCR, 2^31", (np.array([[sr.LOAD_WIRE, 0, 0, 0], [sr.ACC, 0, 0, 0], [sr.ACCR, 1, 0, 0], [sr.ACC, 0, 0, 0], [sr.ACCR, 1, 0, 0],
                                   [sr.EMIT, 0, 1, 0]], dtype=np.uint16), [1 << 31]), None),  # ACCR starts the bound again
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,program,message", ACC_BOUND_CASES, ids=[c[0] for c in ACC_BOUND_CASES])
def test_the_acc_bound_is_kept_beyond_64_bits(gpu, name, program, message):
    from plonky2_gpu_amd.stark import StarkDesc

    instrs, imms = program
    desc = StarkDesc(3, 4, 0, 2, 2, si.fri_params(), instrs, imms, [])
    got = _create(gpu, desc)
    if message is None:
        sr.validate_program(instrs, imms, 4, 0)
        assert got is None, got
    else:
        with pytest.raises(ValueError):
            sr.validate_program(instrs, imms, 4, 0)
        assert got is not None and message in got, got
