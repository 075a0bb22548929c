"""The reference's Keccak-f table (evm/src/keccak/: keccak_stark.rs, columns.rs, round_flags.rs, logic.rs, constants.rs) as a
STARK of this package: 2430 columns, 24 rows per permutation, constraints of degree 3.

    column indices      columns.rs (reg_b is an alias into A', it has no columns of its own)
    program()           eval_packed_generic (keccak_stark.rs:230-375) with eval_round_flags, as one StarkAsm register program, the
                        constraints in the reference's order; gl_keccak_table_program emits the same words natively
    stark_desc()        the StarkDesc gl_stark_create / gl_stark_tables_create take
    ctl_data() / ctl_filter()   the cross-table lookup's columns (keccak_stark.rs:34-43)
    generate_trace()    gl_keccak_table_trace: generate_trace_rows (keccak_stark.rs:53-72) built in HBM

The bit recompositions (acc.doubles() + bit over 32 bits) run through an ACC accumulator in two blocks of 16 weights 2^0 .. 2^15
joined by one shift: 32 weights up to 2^31 on one accumulator would break its overflow contract. rc_value_bit(r, i) is known when
the program is emitted: the sum over the rounds of flag_r * rc_value_bit(r, i) keeps the rounds whose bit is 1 (weight 1) and is
left out altogether for the 57 bit positions no round constant has — xor_gen(bit, 0) is the bit."""
from . import table
from .stark import CtlColumn, StarkAsm, StarkDesc

NUM_ROUNDS = 24
NUM_INPUTS = 25
RC = [
    0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
    0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
    0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
    0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008,
]
R = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]

START_A = NUM_ROUNDS
START_C = START_A + 5 * 5 * 2
START_C_PRIME = START_C + 5 * 64
START_A_PRIME = START_C_PRIME + 5 * 64
START_A_PRIME_PRIME = START_A_PRIME + 5 * 5 * 64
START_A_PRIME_PRIME_0_0_BITS = START_A_PRIME_PRIME + 5 * 5 * 2
REG_A_PRIME_PRIME_PRIME_0_0_LO = START_A_PRIME_PRIME_0_0_BITS + 64
NUM_COLUMNS = REG_A_PRIME_PRIME_PRIME_0_0_LO + 2
assert NUM_COLUMNS == 2430


def reg_step(i):
    return i


def reg_a(x, y):
    return START_A + (x * 5 + y) * 2


def reg_c(x, z):
    return START_C + x * 64 + z


def reg_c_prime(x, z):
    return START_C_PRIME + x * 64 + z


def reg_a_prime(x, y, z):
    return START_A_PRIME + x * 64 * 5 + y * 64 + z


def reg_b(x, y, z):
    """B[x, y] = ROT(A'[a, x], r[a, x]) with a = (x + 3 y) mod 5: an alias into A'"""
    a = (x + 3 * y) % 5
    return reg_a_prime(a, x, (z + 64 - R[a][x]) % 64)


def reg_a_prime_prime(x, y):
    return START_A_PRIME_PRIME + x * 2 * 5 + y * 2


def reg_a_prime_prime_0_0_bit(i):
    return START_A_PRIME_PRIME_0_0_BITS + i


def reg_a_prime_prime_prime(x, y):
    return REG_A_PRIME_PRIME_PRIME_0_0_LO if x == 0 and y == 0 else reg_a_prime_prime(x, y)


def reg_input_limb(i):
    """limb i of the input: input[i / 2] is lane (x, y) = (i / 2 % 5, i / 2 / 5)"""
    return reg_a((i // 2) % 5, (i // 2) // 5) + i % 2


def reg_output_limb(i):
    return reg_a_prime_prime_prime((i // 2) % 5, (i // 2) // 5) + i % 2


def rc_value_bit(r, i):
    return (RC[r] >> i) & 1


# ---------------------------------------------------------------- the constraints
def _xor(a, x, y):
    """xor_gen(x, y) = x + y - 2 x y in a fresh register; x and y stay"""
    s = a.add(x, y)
    m = a.mul(x, y)
    a.mulk(m, 1, dst=m)
    a.sub(s, m, dst=s)
    a.free(m)
    return s


def _xor3(a, x, y, z):
    """xor3_gen(x, y, z) = xor_gen(x, xor_gen(y, z))"""
    t = _xor(a, y, z)
    u = _xor(a, x, t)
    a.free(t)
    return u


def _limb(a, bit, z0):
    """sum_{k < 32} 2^k bit(z0 + k): what the fold acc.doubles() + bit over the limb's bits computes. `bit(z)` returns a register
    that is freed here."""
    halves = []
    for h in range(2):
        for k in range(16):
            t = bit(z0 + 16 * h + k)
            a.acc(t, 1 << k)
            a.free(t)
        halves.append(a.accr())
    lo, hi = halves
    a.mulk(hi, 16, dst=hi)
    a.add(hi, lo, dst=hi)
    a.free(lo)
    return hi


def program():
    """(instrs [k][4] uint16, immediates): eval_packed_generic, 842 constraints in the reference's order"""
    a = StarkAsm()
    # eval_round_flags (round_flags.rs:12-27)
    a.emit_first_row(a.sub(a.local(reg_step(0)), a.imm(1)))
    for i in range(1, NUM_ROUNDS):
        a.release()
        a.emit_first_row(a.local(reg_step(i)))
    for i in range(NUM_ROUNDS):
        a.release()
        a.emit_transition(a.sub(a.next(reg_step((i + 1) % NUM_ROUNDS)), a.local(reg_step(i))))
    # C'[x, z] = xor(C[x, z], C[x - 1, z], C[x + 1, z - 1])
    for x in range(5):
        for z in range(64):
            a.release()
            xor = _xor3(a, a.local(reg_c(x, z)), a.local(reg_c((x + 4) % 5, z)), a.local(reg_c((x + 1) % 5, (z + 63) % 64)))
            a.emit(a.sub(a.local(reg_c_prime(x, z)), xor))
    # A[x, y, z] = xor(A'[x, y, z], C[x, z], C'[x, z]), recomposed into the two input limbs
    for x in range(5):
        for y in range(5):

            def bit(z):
                ap, c, cp = a.local(reg_a_prime(x, y, z)), a.local(reg_c(x, z)), a.local(reg_c_prime(x, z))
                t = _xor3(a, ap, c, cp)
                a.free(ap, c, cp)
                return t

            for limb in range(2):
                a.release()
                a.emit(a.sub(_limb(a, bit, 32 * limb), a.local(reg_a(x, y) + limb)))
    # xor_i A'[x, i, z] = C'[x, z]: diff (diff - 2) (diff - 4) = 0 with diff = sum_i A'[x, i, z] - C'[x, z]
    for x in range(5):
        for z in range(64):
            a.release()
            s = a.local(reg_a_prime(x, 0, z))
            for i in range(1, 5):
                t = a.local(reg_a_prime(x, i, z))
                a.add(s, t, dst=s)
                a.free(t)
            diff = a.sub(s, a.local(reg_c_prime(x, z)))
            d2, d4 = a.sub(diff, a.imm(2)), a.sub(diff, a.imm(4))
            a.emit(a.mul(a.mul(diff, d2), d4))
    # A''[x, y] = xor(B[x, y], andn(B[x + 1, y], B[x + 2, y]))
    for x in range(5):
        for y in range(5):
            for limb in range(2):
                a.release()
                one = a.imm(1)

                def bit(z):
                    b0, b1, b2 = a.local(reg_b(x, y, z)), a.local(reg_b((x + 1) % 5, y, z)), a.local(reg_b((x + 2) % 5, y, z))
                    n = a.sub(one, b1)
                    a.mul(n, b2, dst=n)  # andn_gen(x, y) = (1 - x) y
                    t = _xor(a, b0, n)
                    a.free(b0, b1, b2, n)
                    return t

                a.emit(a.sub(_limb(a, bit, 32 * limb), a.local(reg_a_prime_prime(x, y) + limb)))
    # A'''[0, 0] = A''[0, 0] xor RC: the bits of A''[0, 0] recompose into its limbs ...
    for limb in range(2):
        a.release()
        a.emit(a.sub(_limb(a, lambda z: a.local(reg_a_prime_prime_0_0_bit(z)), 32 * limb), a.local(reg_a_prime_prime(0, 0) + limb)))

    # ... and xored with the round's constant into the limbs of A'''[0, 0]
    def xored_bit(i):
        b = a.local(reg_a_prime_prime_0_0_bit(i))
        rounds = [r for r in range(NUM_ROUNDS) if rc_value_bit(r, i)]
        if not rounds:
            return b
        for r in rounds:
            f = a.local(reg_step(r))
            a.acc(f, 1, q=1)
            a.free(f)
        rc = a.accr(1)
        t = _xor(a, b, rc)
        a.free(b, rc)
        return t

    for limb in range(2):
        a.release()
        a.emit(a.sub(_limb(a, xored_bit, 32 * limb), a.local(reg_a_prime_prime_prime(0, 0) + limb)))
    # this round's output is the next round's input, except behind the last round
    for x in range(5):
        for y in range(5):
            for limb in range(2):
                a.release()
                not_last = a.sub(a.imm(1), a.local(reg_step(NUM_ROUNDS - 1)))
                diff = a.sub(a.local(reg_a_prime_prime_prime(x, y) + limb), a.next(reg_a(x, y) + limb))
                a.emit_transition(a.mul(not_last, diff))
    return a.program()


def stark_desc(degree_bits, num_challenges, fri_params):
    """KeccakStark as a StarkDesc: constraint_degree 3, no public inputs, no permutation pairs"""
    instrs, immediates = program()
    return StarkDesc(degree_bits, NUM_COLUMNS, 0, 3, num_challenges, fri_params, instrs, immediates)


def ctl_data():
    """keccak_stark.rs:34-38: the 50 input limbs, then the 50 output limbs"""
    return [CtlColumn.single(reg_input_limb(i)) for i in range(2 * NUM_INPUTS)] + [CtlColumn.single(reg_output_limb(i)) for i in range(2 * NUM_INPUTS)]


def ctl_filter():
    """keccak_stark.rs:40-43: the rows of round 23 (those of the padding permutations too, as in the reference)"""
    return CtlColumn.single(reg_step(NUM_ROUNDS - 1))


def native_program():
    """gl_keccak_table_program: (instrs, immediates, number of constraints) as the library emits them — program() word for word"""
    return table.native_program("gl_keccak_table_program")


def generate_trace(ctx, inputs, degree_bits, trace_stride=None):
    """gl_keccak_table_trace: the trace of the Keccak-f[1600] states `inputs` ([num_inputs][25] words, input[5 y + x]; host array or
    DeviceBuffer) with 2^degree_bits rows as a DeviceBuffer [2430][trace_stride] (default 2^degree_bits), built on the context's
    stream; the rows behind the inputs are permutations of the zero state."""
    d_in, num_inputs = table.device_records(ctx, inputs, NUM_INPUTS)
    uploaded = d_in is not None and d_in is not inputs  # the upload's buffer is released on return: the kernel must have read it
    return table.generate_trace(ctx, "gl_keccak_table_trace", [table.ptr(d_in), num_inputs], degree_bits, trace_stride, NUM_COLUMNS,
                                synchronize=uploaded)
