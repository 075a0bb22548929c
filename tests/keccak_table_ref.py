"""The reference's Keccak-f table restated in Python (TEST INFRASTRUCTURE ONLY), written from the Rust and independent of
plonky2_gpu_amd/keccak_table.py, which it checks:

    column indices        evm/src/keccak/columns.rs
    generate_trace_rows   evm/src/keccak/keccak_stark.rs:53-204 (numpy over all permutations at once, integer columns)
    eval_constraints      eval_packed_generic (keccak_stark.rs:230-375) with eval_round_flags (round_flags.rs:12-27) and logic.rs:
                          one hand-written closure per constraint group, the list of (kind, value) in emission order
    KeccakTableStark      the object tests/stark_ref.py and tests/ctl_ref.py prove and verify

Constraints are evaluated over a field object F with zero, one, add, sub, mul, lift — Fp below, or stark_ref's Base / Ext."""
import numpy as np

P = 0xFFFFFFFF00000001
NUM_ROUNDS, NUM_INPUTS = 24, 25
RC = [  # constants.rs
    0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
    0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
    0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
    0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008,
]
R = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]  # columns.rs:43-49

# ---------------------------------------------------------------- columns.rs
START_A = NUM_ROUNDS
START_C = START_A + 50
START_C_PRIME = START_C + 320
START_A_PRIME = START_C_PRIME + 320
START_A_PRIME_PRIME = START_A_PRIME + 1600
START_A_PRIME_PRIME_0_0_BITS = START_A_PRIME_PRIME + 50
REG_A_PRIME_PRIME_PRIME_0_0_LO = START_A_PRIME_PRIME_0_0_BITS + 64
NUM_COLUMNS = REG_A_PRIME_PRIME_PRIME_0_0_LO + 2

reg_step = lambda i: i  # noqa: E731
reg_a = lambda x, y: START_A + (x * 5 + y) * 2  # noqa: E731
reg_c = lambda x, z: START_C + x * 64 + z  # noqa: E731
reg_c_prime = lambda x, z: START_C_PRIME + x * 64 + z  # noqa: E731
reg_a_prime = lambda x, y, z: START_A_PRIME + x * 320 + y * 64 + z  # noqa: E731
reg_a_prime_prime = lambda x, y: START_A_PRIME_PRIME + x * 10 + y * 2  # noqa: E731
reg_a_prime_prime_0_0_bit = lambda i: START_A_PRIME_PRIME_0_0_BITS + i  # noqa: E731


def reg_b(x, y, z):
    a, b = (x + 3 * y) % 5, x
    return reg_a_prime(a, b, (z + 64 - R[a][b]) % 64)


def reg_a_prime_prime_prime(x, y):
    return REG_A_PRIME_PRIME_PRIME_0_0_LO if (x, y) == (0, 0) else reg_a_prime_prime(x, y)


def reg_input_limb(i):
    return reg_a((i // 2) % 5, (i // 2) // 5) + i % 2


def reg_output_limb(i):
    return reg_a_prime_prime_prime((i // 2) % 5, (i // 2) // 5) + i % 2


# ---------------------------------------------------------------- the trace
def _rotl(w, r):
    return w if r == 0 else (w << np.uint64(r)) | (w >> np.uint64(64 - r))


def _bits(w):
    return (w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)


def generate_trace_rows(inputs, n):
    """generate_trace_rows(inputs, min_rows) for a power of two n >= 24 len(inputs): uint64 [n][NUM_COLUMNS]. The permutations behind
    the inputs are the zero state's (pad_rows), the last one cut at n (drain)."""
    inputs = np.asarray(inputs, dtype=np.uint64).reshape(-1, NUM_INPUTS)
    assert n & (n - 1) == 0 and NUM_ROUNDS * inputs.shape[0] <= n
    perms = -(-n // NUM_ROUNDS)
    states = np.zeros((perms, NUM_INPUTS), dtype=np.uint64)
    states[: inputs.shape[0]] = inputs
    rows = np.zeros((perms, NUM_ROUNDS, NUM_COLUMNS), dtype=np.uint64)
    lo, hi = (lambda w: w & np.uint64(0xFFFFFFFF)), (lambda w: w >> np.uint64(32))
    A = [[states[:, y * 5 + x].copy() for y in range(5)] for x in range(5)]  # rows[0][reg_a(x, y)] <- input[y * 5 + x]
    for rnd in range(NUM_ROUNDS):
        row = rows[:, rnd, :]
        row[:, reg_step(rnd)] = 1
        for x in range(5):
            for y in range(5):
                row[:, reg_a(x, y)], row[:, reg_a(x, y) + 1] = lo(A[x][y]), hi(A[x][y])
        C = [A[x][0] ^ A[x][1] ^ A[x][2] ^ A[x][3] ^ A[x][4] for x in range(5)]
        Cp = [C[x] ^ C[(x + 4) % 5] ^ _rotl(C[(x + 1) % 5], 1) for x in range(5)]  # bit z of rotl(c, 1) is bit z - 1 of c
        Ap = [[A[x][y] ^ C[x] ^ Cp[x] for y in range(5)] for x in range(5)]
        for x in range(5):
            row[:, reg_c(x, 0) : reg_c(x, 0) + 64] = _bits(C[x])
            row[:, reg_c_prime(x, 0) : reg_c_prime(x, 0) + 64] = _bits(Cp[x])
            for y in range(5):
                row[:, reg_a_prime(x, y, 0) : reg_a_prime(x, y, 0) + 64] = _bits(Ap[x][y])
        # bit z of B[x, y] is A'[a, x, z - r[a][x]] with a = (x + 3 y) mod 5 (reg_b): B[x, y] = rotl(A'[a, x], r[a][x])
        B = [[_rotl(Ap[(x + 3 * y) % 5][x], R[(x + 3 * y) % 5][x]) for y in range(5)] for x in range(5)]
        App = [[B[x][y] ^ (~B[(x + 1) % 5][y] & B[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        for x in range(5):
            for y in range(5):
                row[:, reg_a_prime_prime(x, y)], row[:, reg_a_prime_prime(x, y) + 1] = lo(App[x][y]), hi(App[x][y])
        row[:, reg_a_prime_prime_0_0_bit(0) : reg_a_prime_prime_0_0_bit(0) + 64] = _bits(App[0][0])
        out00 = App[0][0] ^ np.uint64(RC[rnd])
        row[:, REG_A_PRIME_PRIME_PRIME_0_0_LO], row[:, REG_A_PRIME_PRIME_PRIME_0_0_LO + 1] = lo(out00), hi(out00)
        A = App  # copy_output_to_input
        A[0][0] = out00
    return rows.reshape(perms * NUM_ROUNDS, NUM_COLUMNS)[:n].copy()


def outputs_of(rows, k):
    """the 25 output words of permutation k, from reg_output_limb of its last row"""
    last = rows[NUM_ROUNDS * k + NUM_ROUNDS - 1]
    return [int(last[reg_output_limb(2 * i)]) | (int(last[reg_output_limb(2 * i + 1)]) << 32) for i in range(NUM_INPUTS)]


# ---------------------------------------------------------------- the constraints
class Fp:
    zero, one = 0, 1
    add = staticmethod(lambda x, y: (x + y) % P)
    sub = staticmethod(lambda x, y: (x - y) % P)
    mul = staticmethod(lambda x, y: x * y % P)
    lift = staticmethod(lambda x: int(x) % P)


ALL, TRANSITION, FIRST_ROW = "constraint", "transition", "first_row"
# (group name, number of constraints) in emission order
GROUPS = [("round_flags_first_row", 24), ("round_flags_transition", 24), ("c_prime", 320), ("a_from_a_prime", 50), ("a_prime_parity", 320),
          ("a_prime_prime", 50), ("a_prime_prime_0_0_bits", 2), ("a_prime_prime_prime_0_0", 2), ("next_input", 50)]
NUM_CONSTRAINTS = sum(k for _, k in GROUPS)


def group_of(index):
    """the name of the group constraint number `index` belongs to"""
    for name, k in GROUPS:
        if index < k:
            return name
        index -= k
    raise IndexError(index)


def eval_constraints(local, nxt, F=Fp):
    """[(kind, value)] of the 842 constraints in emission order"""
    out = []
    two, four = F.lift(2), F.lift(4)
    xor_gen = lambda x, y: F.sub(F.add(x, y), F.mul(x, F.add(y, y)))  # noqa: E731  x + y - x * y.doubles()
    xor3_gen = lambda x, y, z: xor_gen(x, xor_gen(y, z))  # noqa: E731
    andn_gen = lambda x, y: F.mul(F.sub(F.one, x), y)  # noqa: E731

    def fold(bits):  # (z0 .. z1).rev().fold(0, |acc, z| acc.doubles() + bit(z)) with the bits listed from z0 up
        acc = F.zero
        for b in reversed(bits):
            acc = F.add(F.add(acc, acc), b)
        return acc

    def round_flags_first_row():
        out.append((FIRST_ROW, F.sub(local[reg_step(0)], F.one)))
        for i in range(1, NUM_ROUNDS):
            out.append((FIRST_ROW, local[reg_step(i)]))

    def round_flags_transition():
        for i in range(NUM_ROUNDS):
            out.append((TRANSITION, F.sub(nxt[reg_step((i + 1) % NUM_ROUNDS)], local[reg_step(i)])))

    def c_prime():
        for x in range(5):
            for z in range(64):
                xor = xor3_gen(local[reg_c(x, z)], local[reg_c((x + 4) % 5, z)], local[reg_c((x + 1) % 5, (z + 63) % 64)])
                out.append((ALL, F.sub(local[reg_c_prime(x, z)], xor)))

    def a_from_a_prime():
        for x in range(5):
            for y in range(5):
                bit = lambda z: xor3_gen(local[reg_a_prime(x, y, z)], local[reg_c(x, z)], local[reg_c_prime(x, z)])  # noqa: E731
                out.append((ALL, F.sub(fold([bit(z) for z in range(32)]), local[reg_a(x, y)])))
                out.append((ALL, F.sub(fold([bit(z) for z in range(32, 64)]), local[reg_a(x, y) + 1])))

    def a_prime_parity():
        for x in range(5):
            for z in range(64):
                s = F.zero
                for i in range(5):
                    s = F.add(s, local[reg_a_prime(x, i, z)])
                diff = F.sub(s, local[reg_c_prime(x, z)])
                out.append((ALL, F.mul(F.mul(diff, F.sub(diff, two)), F.sub(diff, four))))

    def a_prime_prime():
        for x in range(5):
            for y in range(5):
                bit = lambda z: xor_gen(local[reg_b(x, y, z)], andn_gen(local[reg_b((x + 1) % 5, y, z)], local[reg_b((x + 2) % 5, y, z)]))  # noqa: E731
                out.append((ALL, F.sub(fold([bit(z) for z in range(32)]), local[reg_a_prime_prime(x, y)])))
                out.append((ALL, F.sub(fold([bit(z) for z in range(32, 64)]), local[reg_a_prime_prime(x, y) + 1])))

    bits00 = [local[reg_a_prime_prime_0_0_bit(i)] for i in range(64)]

    def a_prime_prime_0_0_bits():
        out.append((ALL, F.sub(fold(bits00[:32]), local[reg_a_prime_prime(0, 0)])))
        out.append((ALL, F.sub(fold(bits00[32:]), local[reg_a_prime_prime(0, 0) + 1])))

    def a_prime_prime_prime_0_0():
        def xored(i):
            rc_bit = F.zero
            for r in range(NUM_ROUNDS):
                rc_bit = F.add(rc_bit, F.mul(local[reg_step(r)], F.lift((RC[r] >> i) & 1)))
            return xor_gen(bits00[i], rc_bit)

        out.append((ALL, F.sub(fold([xored(i) for i in range(32)]), local[reg_a_prime_prime_prime(0, 0)])))
        out.append((ALL, F.sub(fold([xored(i) for i in range(32, 64)]), local[reg_a_prime_prime_prime(0, 0) + 1])))

    def next_input():
        not_last = F.sub(F.one, local[reg_step(NUM_ROUNDS - 1)])
        for x in range(5):
            for y in range(5):
                for limb in range(2):
                    out.append((TRANSITION, F.mul(not_last, F.sub(local[reg_a_prime_prime_prime(x, y) + limb], nxt[reg_a(x, y) + limb]))))

    closures = dict(round_flags_first_row=round_flags_first_row, round_flags_transition=round_flags_transition, c_prime=c_prime,
                    a_from_a_prime=a_from_a_prime, a_prime_parity=a_prime_parity, a_prime_prime=a_prime_prime,
                    a_prime_prime_0_0_bits=a_prime_prime_0_0_bits, a_prime_prime_prime_0_0=a_prime_prime_prime_0_0, next_input=next_input)
    for name, count in GROUPS:
        before = len(out)
        closures[name]()
        assert len(out) - before == count, name
    return out


def violated(rows, r):
    """indices of the constraints that do not hold on row r of `rows` (next row r + 1, wrapping): transition constraints are not
    checked on the last row, first-row constraints only on row 0"""
    n = len(rows)
    local, nxt = [int(v) for v in rows[r]], [int(v) for v in rows[(r + 1) % n]]
    bad = []
    for k, (kind, v) in enumerate(eval_constraints(local, nxt)):
        if kind == TRANSITION and r == n - 1:
            continue
        if kind == FIRST_ROW and r != 0:
            continue
        if v != 0:
            bad.append(k)
    return bad


class KeccakTableStark:
    """what tests/stark_ref.py and tests/ctl_ref.py take: shape, the register program under test and the closures above"""
    num_columns, num_public_inputs, constraint_degree, pairs = NUM_COLUMNS, 0, 3, []

    def __init__(self, instrs, immediates):
        # plain tuples of ints: the interpreter of tests/stark_ref.py walks them once per point
        self.instrs, self.immediates = [tuple(int(x) for x in row) for row in instrs], [int(x) for x in immediates]

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        for kind, v in eval_constraints(local, nxt, F):
            getattr(consumer, kind)(v) if kind == ALL else getattr(consumer, "constraint_" + kind)(v)
