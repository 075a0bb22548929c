"""Random STARK constraint programs and random STARK descriptions (TEST INFRASTRUCTURE ONLY).

gen_program builds a register program that is valid by construction under the rules of include/plonky2_hip.h (what gl_stark_create
and tests/stark_ref.py's validate_program check) and goes where the three hand-written STARKs of tests/stark_instances.py do not:
every register up to 63, destinations that are their own sources, registers overwritten after use, MULK by 0 / 32 / 63, the four ACC
accumulators interleaved up to the largest sum the overflow contract allows, the four kinds of EMIT in any order.

fuzz_case(i) is description i of the fixed list CASES that tests/test_gpu_stark_fuzz.py runs on the device; coverage() is what
tests/test_stark_fuzz.py asserts about that list, so that a change of the generator that loses a path fails on the CPU."""
import numpy as np

import stark_ref as sr

P = sr.P
ACC_WEIGHTS = [0, 1, 3, (1 << 30) - 1, 1 << 31, (1 << 32) - 1]  # 2^32 - 1 never fits: (2^32 - 1)^2 > 2^63; 2^31 fits alone
MULK_SHIFTS = [0, 1, 31, 32, 33, 63]
IMMEDIATES = [P - 1, 1 << 32, (1 << 32) - 1]
EMITS = (sr.EMIT, sr.EMIT_TRANSITION, sr.EMIT_FIRST_ROW, sr.EMIT_LAST_ROW)
# relative frequencies: every opcode near or above 5 % of the instructions
WEIGHTS = {sr.LOAD_WIRE: 8, sr.LOAD_NEXT: 7, sr.LOAD_PI: 5, sr.LOAD_IMM: 6, sr.ADD: 9, sr.SUB: 9, sr.MUL: 10, sr.MULK: 7, sr.ACC: 10,
           sr.ACCR: 6, sr.EMIT: 5, sr.EMIT_TRANSITION: 5, sr.EMIT_FIRST_ROW: 5, sr.EMIT_LAST_ROW: 5}


def _word(rng):
    return int(rng.integers(0, P, dtype=np.uint64))


def gen_program(rng, num_columns, num_public_inputs, length):
    """(instrs [length][4] uint16, immediates): `length` >= 2 instructions, the first a load, the last an EMIT"""
    assert length >= 2 and num_columns >= 1
    instrs, imms, imm_index = [], [], {}
    written, bound, used = [], [0] * 4, [False] * 4

    def imm(v):
        if v not in imm_index:
            imm_index[v] = len(imms)
            imms.append(v)
        return imm_index[v]

    def column():
        return num_columns - 1 if rng.random() < 0.2 else int(rng.integers(0, num_columns))

    def src():
        return written[int(rng.integers(0, len(written)))]

    def dst(sources=()):
        u = rng.random()
        if sources and u < 0.15:
            r = sources[int(rng.integers(0, len(sources)))]  # ADD r, r, x
        elif u < 0.30:
            r = 63
        elif written and u < 0.55:
            r = src()  # overwritten after use
        else:
            r = int(rng.integers(0, sr.MAX_REGS))
        if r not in written:
            written.append(r)
        return r

    while len(instrs) < length:
        last = len(instrs) == length - 1
        ops = [op for op in WEIGHTS if not (op == sr.LOAD_PI and num_public_inputs == 0) and not (op == sr.ACCR and not any(used))]
        if not written:
            ops = [sr.LOAD_WIRE, sr.LOAD_NEXT]
        if last:
            ops = list(EMITS)
        w = np.array([WEIGHTS[op] for op in ops], dtype=np.float64)
        op = ops[int(rng.choice(len(ops), p=w / w.sum()))]
        if op in (sr.LOAD_WIRE, sr.LOAD_NEXT):
            instrs.append((op, dst(), column(), 0))
        elif op == sr.LOAD_PI:
            instrs.append((op, dst(), int(rng.integers(0, num_public_inputs)), 0))
        elif op == sr.LOAD_IMM:
            v = IMMEDIATES[int(rng.integers(0, len(IMMEDIATES)))] if rng.random() < 0.5 else _word(rng)
            instrs.append((op, dst(), imm(v), 0))
        elif op in (sr.ADD, sr.SUB, sr.MUL):
            a = src()
            b = a if rng.random() < 0.1 else src()
            instrs.append((op, dst((a, b)), a, b))
        elif op == sr.MULK:
            a = src()
            shift = MULK_SHIFTS[int(rng.integers(0, len(MULK_SHIFTS)))] if rng.random() < 0.75 else int(rng.integers(0, 64))
            instrs.append((op, dst((a,)), a, shift))
        elif op == sr.ACC:
            q = int(rng.integers(0, 4))
            fits = [k for k in ACC_WEIGHTS if bound[q] + k * 0xFFFFFFFF < sr.ACC_LIMIT]  # 0 always fits
            k = fits[int(rng.integers(0, len(fits)))]
            bound[q] += k * 0xFFFFFFFF
            used[q] = True
            instrs.append((op, q, src(), imm(k)))
        elif op == sr.ACCR:
            q = [k for k in range(4) if used[k]]
            q = q[int(rng.integers(0, len(q)))]
            bound[q], used[q] = 0, False
            instrs.append((op, dst(), q, 0))
        else:
            instrs.append((op, 0, src(), 0))
    return np.array(instrs, dtype=np.uint16).reshape(-1, 4), imms


def coverage(instrs, immediates):
    """what one program reaches: the opcodes, whether register 63 is a destination, the accumulators, the MULK shifts, whether an
    accumulator's bound exceeded 2^62 at its ACCR, whether an instruction overwrote one of its own sources"""
    ops, accs, shifts = set(), set(), set()
    dst63 = high = own = False
    bound = [0] * 4
    for op, dst, a, b in ([int(x) for x in row] for row in instrs):
        ops.add(op)
        writes = op not in EMITS and op != sr.ACC
        dst63 |= writes and dst == 63
        if op in (sr.ADD, sr.SUB, sr.MUL):
            own |= dst in (a, b)
        elif op == sr.MULK:
            shifts.add(b)
            own |= dst == a
        elif op == sr.ACC:
            accs.add(dst)
            bound[dst] += (immediates[b] % P) * 0xFFFFFFFF
        elif op == sr.ACCR:
            high |= bound[a] > 1 << 62
            bound[a] = 0
    return dict(ops=ops, dst63=dst63, accs=accs, shifts=shifts, high_bound=high, own_source=own)


# ---------------------------------------------------------------- random STARK descriptions for gl_stark_quotient_polys
class FuzzStark:
    """what tests/stark_ref.py and StarkDesc need of a STARK; no closure and no trace generator: only the quotient is run"""

    def __init__(self, num_columns, num_public_inputs, constraint_degree, pairs, instrs, immediates):
        self.num_columns, self.num_public_inputs, self.constraint_degree = num_columns, num_public_inputs, constraint_degree
        self.pairs, self.instrs, self.immediates = pairs, instrs, immediates


QDFS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16]
# program lengths: the short ones cannot hold every opcode, so there are fewer of them; one long program
LENGTHS = [60, 400, 8, 60, 400, 60, 8, 400, 60, 400, 8, 4000, 60, 400, 60, 8, 400, 60, 400, 400, 8, 60, 400, 8]
CASES = list(range(len(LENGTHS)))
SEED = 20260


def fuzz_case(i):
    """description i: dict(stark, degree_bits, rate_bits, num_challenges). num_challenges cycles through 1..4 and the quotient degree
    factor through QDFS (index 19 is qdf 16 with 4 challenges: all 64 (beta, gamma) pairs), the public inputs through 1, 3, 0, 3, 1;
    the rest is drawn from seed SEED + i"""
    rng = np.random.default_rng(SEED + i)
    num_columns = (1, 5, 70)[int(rng.integers(0, 3))]
    num_public_inputs = (1, 3, 0, 3, 1)[i % 5]  # none in a fifth of the cases: LOAD_PI has to occur in half of the programs
    num_challenges, qdf = 1 + i % 4, QDFS[i % len(QDFS)]
    constraint_degree = qdf + 1 if qdf > 1 else 1 + (i // len(QDFS)) % 2
    qdb = (qdf - 1).bit_length()
    degree_bits = int(rng.integers(1, 5)) if LENGTHS[i] < 1000 else 2  # the long program on few points: the reference is Python
    rate_bits = max(1, qdb + int(rng.integers(0, 2)))
    pairs = [[(int(rng.integers(0, num_columns)), int(rng.integers(0, num_columns))) for _ in range(int(rng.integers(0, 4)))]
             for _ in range(int(rng.integers(0, 4)))]
    instrs, immediates = gen_program(rng, num_columns, num_public_inputs, LENGTHS[i])
    stark = FuzzStark(num_columns, num_public_inputs, constraint_degree, pairs, instrs, immediates)
    return dict(stark=stark, degree_bits=degree_bits, rate_bits=rate_bits, num_challenges=num_challenges)


def fuzz_inputs(i, case):
    """uniform canonical words for everything gl_stark_quotient_polys reads: (trace "LDE" columns [num_columns][n_ext], Z "LDE"
    columns or None, challenge sets or None, alphas, public inputs)"""
    rng = np.random.default_rng(7 * SEED + i)
    stark, nch = case["stark"], case["num_challenges"]
    n_ext = 1 << (case["degree_bits"] + case["rate_bits"])
    words = lambda *shape: rng.integers(0, P, size=shape, dtype=np.uint64)  # noqa: E731
    trace = words(stark.num_columns, n_ext)
    zs = sets = None
    if stark.pairs:
        qdf = sr.quotient_degree_factor(stark)
        zs = words(sr.num_zs(stark, nch), n_ext)
        sets = [[(_word(rng), _word(rng)) for _ in range(nch)] for _ in range(qdf)]
    return trace, zs, sets, [int(x) for x in words(nch)], [int(x) for x in words(stark.num_public_inputs)]


def reference_quotient(case, trace, zs, sets, alphas, pis):
    """sr.compute_quotient_polys on column-major words (any words: they need not be LDEs) -> uint64 [num_challenges][n << qdb]"""
    leaves = lambda cols: None if cols is None else np.asarray(cols, dtype=np.uint64).T.tolist()  # noqa: E731
    out = sr.compute_quotient_polys(case["stark"], case["num_challenges"], case["degree_bits"], case["rate_bits"], leaves(trace), leaves(zs), sets,
                                    pis, alphas)
    return np.array(out, dtype=np.uint64)


def fast_permutation_z_polys(stark, num_challenges, trace, challenge_sets):
    """sr.compute_permutation_z_polys with ONE inversion per Z (Montgomery's batch inversion) instead of one per row, for traces of
    2^19 rows; every denominator must be non-zero. tests/test_stark_fuzz.py holds it against the original."""
    n = len(trace[0])
    zs = []
    for instances in sr.get_permutation_batches(stark.pairs, challenge_sets, num_challenges, sr.quotient_degree_factor(stark)):
        nums, dens = [], []
        for r in range(n):
            num = den = 1
            for pair, (beta, gamma) in instances:
                lhs = rhs = gamma
                weight = 1
                for i, j in pair:
                    lhs = (lhs + trace[i][r] * weight) % P
                    rhs = (rhs + trace[j][r] * weight) % P
                    weight = weight * beta % P
                num, den = num * lhs % P, den * rhs % P
            nums.append(num)
            dens.append(den)
        prefix, acc = [], 1
        for d in dens:
            assert d, "a zero denominator: batch inversion does not apply"
            prefix.append(acc)
            acc = acc * d % P
        inv = pow(acc, P - 2, P)  # 1 / (d_0 .. d_{n-1})
        for r in range(n - 1, -1, -1):
            nums[r] = nums[r] * (inv * prefix[r] % P) % P  # the row's quotient
            inv = inv * dens[r] % P
        z, acc = [], 1
        for q in nums:
            z.append(acc)
            acc = acc * q % P
        zs.append(z)
    return zs
