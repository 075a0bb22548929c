"""The reference's arithmetic table (evm/src/arithmetic/, ArithmeticStark) as a STARK of this package: 92 columns, twelve operator
flags and five ranges of sixteen 16-bit limbs, one row per ADD / MUL / SUB / LT / GT and two rows per DIV / MOD / ADDMOD / SUBMOD /
MULMOD of 256-bit words, zero rows behind them.

The reference's snapshot has the columns, `ArithmeticStark::generate(lv, nv)` for one operation's derived cells and
`eval_packed_generic`; it has no generate_trace, no range checks and no cross-table lookup, and SHL / SHR panic. So the TABLE is
defined here: operations in list order, operation k from row `exclusive prefix sum of the row counts` on, a
modular operation's second row with all flags zero and the overlay MODULAR_QUO_INPUT_HI / MODULAR_AUX_INPUT /
MODULAR_MOD_IS_ZERO / MODULAR_OUT_AUX_RED, every cell the reference does not write zero, signed values as p - |v|. The cells of an
operation are bit for bit what add / sub / mul / compare / modular::generate write.

    column indices      columns.rs:25-117
    program()           add, sub, mul, compare and modular::eval_packed_generic (arithmetic_stark.rs:72-87) as one StarkAsm register
                        program, 246 constraints in the reference's order; gl_arithmetic_table_program emits the same words
    stark_desc()        the StarkDesc gl_stark_create / gl_stark_tables_create take. constraint_degree defaults to 5, not the
                        reference's 3: modular.rs:350 makes the less-than's `t` quadratic wherever a DIV row exists
    ctl_data(kind) / ctl_filter(kind)   three looked entries, "binary", "modular" and "div" (the reference has none)
    ops_to_words()      (op, in0, in1, in2) -> the [num_ops][25] records gl_arithmetic_table_trace takes
    result()            the EVM semantics of arithmetic/mod.rs
    generate_trace()    gl_arithmetic_table_trace: the trace built in HBM"""
import ctypes

import numpy as np

from . import _lib, table
from .device import DeviceBuffer
from .stark import CtlColumn, StarkAsm, StarkDesc

P = 0xFFFFFFFF00000001
LIMB_BITS = 16
N_LIMBS = 16
IS_ADD, IS_MUL, IS_SUB, IS_DIV, IS_MOD, IS_ADDMOD, IS_SUBMOD, IS_MULMOD, IS_LT, IS_GT, IS_SHL, IS_SHR = range(12)
NUM_FLAGS = 12
GENERAL_INPUT_0 = NUM_FLAGS
GENERAL_INPUT_1 = GENERAL_INPUT_0 + N_LIMBS
GENERAL_INPUT_2 = GENERAL_INPUT_1 + N_LIMBS
GENERAL_INPUT_3 = GENERAL_INPUT_2 + N_LIMBS
AUX_INPUT_0_LO = GENERAL_INPUT_3 + N_LIMBS
NUM_COLUMNS = AUX_INPUT_0_LO + N_LIMBS
# the second row of a modular operation
MODULAR_QUO_INPUT_HI = GENERAL_INPUT_0
MODULAR_AUX_INPUT = MODULAR_QUO_INPUT_HI + N_LIMBS  # 31 values
MODULAR_MOD_IS_ZERO = MODULAR_AUX_INPUT + 2 * N_LIMBS - 1
MODULAR_OUT_AUX_RED = MODULAR_MOD_IS_ZERO + 1
assert NUM_COLUMNS == 92 == _lib.GL_ARITHMETIC_TABLE_COLUMNS
assert (MODULAR_MOD_IS_ZERO, MODULAR_OUT_AUX_RED) == (59, 60)
# a record's operator is the index of its flag column
OP_ADD, OP_MUL, OP_SUB, OP_DIV, OP_MOD, OP_ADDMOD, OP_SUBMOD, OP_MULMOD, OP_LT, OP_GT = range(10)
ONE_ROW_OPS = (OP_ADD, OP_MUL, OP_SUB, OP_LT, OP_GT)
TWO_ROW_OPS = (OP_DIV, OP_MOD, OP_ADDMOD, OP_SUBMOD, OP_MULMOD)
OP_WORDS = 25  # the operator and the eight 32-bit limbs of in0, in1, in2
assert OP_WORDS == _lib.GL_ARITHMETIC_TABLE_OP_WORDS
NUM_CONSTRAINTS = 16 + 16 + 16 + 35 + 163
MAX_DEGREE_BITS = 22  # gl_stark_create: degree_bits + rate_bits <= 24, and degree 5 needs rate_bits >= 2
OVERFLOW = 1 << LIMB_BITS
OVERFLOW_INV = pow(OVERFLOW, P - 2, P)


def rows_of(op):
    """the rows an operation of operator `op` takes"""
    return 2 if op in TWO_ROW_OPS else 1


# ---------------------------------------------------------------- the constraints
def _are_equal(a, is_op, larger, smaller, emit):
    """eval_packed_generic_are_equal (add.rs:33-62): 16 constraints is_op * t * (2^16 - t) with t = cy + larger[i] - smaller[i];
    returns the register of the last carry. larger(i) / smaller(i) give registers that are consumed here."""
    overflow, overflow_inv = a.imm(OVERFLOW), a.imm(OVERFLOW_INV)
    cy = None
    for i in range(N_LIMBS):
        t = larger(i)
        s = smaller(i)
        if cy is not None:
            a.add(t, cy, dst=t)
            a.free(cy)
        a.sub(t, s, dst=t)
        a.free(s)
        u = a.sub(overflow, t)
        a.mul(u, t, dst=u)
        a.mul(u, is_op, dst=u)
        emit(u)
        a.free(u)
        a.mul(t, overflow_inv, dst=t)
        cy = t
    a.free(overflow, overflow_inv)
    return cy


def _pair(a, op, load0, c0, load1, c1):
    """i -> load0(c0 + i) op load1(c1 + i) in a fresh register"""
    def limb(i):
        x, y = load0(c0 + i), load1(c1 + i)
        op(x, y, dst=x)
        a.free(y)
        return x
    return limb


def _conv(a, d, left, num_left, right, num_right):
    """sum over i + j = d, i < num_left, j < num_right of left(i) * right(j) in a fresh register (the operands are loaded for every
    product and consumed); None where the sum is empty"""
    total = None
    for i in range(max(0, d - num_right + 1), min(d, num_left - 1) + 1):
        x, y = left(i), right(d - i)
        a.mul(x, y, dst=x)
        a.free(y)
        if total is None:
            total = x
        else:
            a.add(total, x, dst=total)
            a.free(x)
    return total


def _lt(a, is_op, in0, in1, aux, output, emit):
    """eval_packed_generic_lt (compare.rs:53-81); `output` gives a register that is consumed"""
    def lhs(i):
        x, y = in0(i), in1(i)
        a.sub(x, y, dst=x)
        a.free(y)
        return x
    cy = _are_equal(a, is_op, aux, lhs, emit)
    out = output()
    a.sub(cy, out, dst=cy)
    a.free(out)
    a.mul(cy, is_op, dst=cy)
    emit(cy)
    a.free(cy)


def program():
    """(instrs [k][4] uint16, immediates): the 246 constraints of arithmetic_stark.rs:72-87 in the reference's order"""
    a = StarkAsm()
    local, nxt = a.local, a.next
    col = lambda load, c: (lambda i: load(c + i))  # noqa: E731
    in0, in1, in2, in3 = (col(local, c) for c in (GENERAL_INPUT_0, GENERAL_INPUT_1, GENERAL_INPUT_2, GENERAL_INPUT_3))

    # add.rs:116-140: in0 + in1 against the output
    a.release()
    flag = local(IS_ADD)
    a.free(_are_equal(a, flag, _pair(a, a.add, local, GENERAL_INPUT_0, local, GENERAL_INPUT_1), in2, a.emit))
    # sub.rs:40-62: the output against in0 - in1
    a.release()
    flag = local(IS_SUB)
    a.free(_are_equal(a, flag, in2, _pair(a, a.sub, local, GENERAL_INPUT_0, local, GENERAL_INPUT_1), a.emit))
    # mul.rs:102-146: a(x) b(x) - c(x) - (x - 2^16) s(x), the sixteen low coefficients
    a.release()
    flag = local(IS_MUL)
    for d in range(N_LIMBS):
        c = _conv(a, d, in0, N_LIMBS, in1, N_LIMBS)
        t = local(GENERAL_INPUT_2 + d)
        a.sub(c, t, dst=c)
        a.free(t)
        t = local(GENERAL_INPUT_3 + d)  # pol_adjoin_root: s[d - 1] - 2^16 s[d]
        a.mulk(t, LIMB_BITS, dst=t)
        a.add(c, t, dst=c)
        a.free(t)
        if d:
            t = local(GENERAL_INPUT_3 + d - 1)
            a.sub(c, t, dst=c)
            a.free(t)
        a.mul(c, flag, dst=c)
        a.emit(c)
        a.free(c)
    # compare.rs:83-104
    a.release()
    is_lt, is_gt = local(IS_LT), local(IS_GT)
    t = a.add(is_lt, is_gt)
    out = local(GENERAL_INPUT_2)
    a.mul(t, out, dst=t)
    one = a.imm(1)
    a.sub(out, one, dst=out)
    a.mul(t, out, dst=t)
    a.emit(t)
    a.free(t, out, one)
    output = lambda: local(GENERAL_INPUT_2)  # noqa: E731
    _lt(a, is_lt, in0, in1, in3, output, a.emit)
    _lt(a, is_gt, in1, in0, in3, output, a.emit)

    # modular.rs:407-459
    a.release()
    flt = local(IS_ADDMOD)
    for f in (IS_MULMOD, IS_MOD, IS_SUBMOD, IS_DIV):
        t = local(f)
        a.add(flt, t, dst=flt)
        a.free(t)
    a.emit_last_row(flt)
    # modular_constr_poly (:316-404)
    miz = nxt(MODULAR_MOD_IS_ZERO)
    t = a.mul(miz, miz)
    a.sub(t, miz, dst=t)
    a.mul(t, flt, dst=t)
    a.emit_transition(t)
    a.free(t)
    t = local(GENERAL_INPUT_2)
    for i in range(1, N_LIMBS):
        u = local(GENERAL_INPUT_2 + i)
        a.add(t, u, dst=t)
        a.free(u)
    a.mul(t, flt, dst=t)
    a.mul(t, miz, dst=t)
    a.emit_transition(t)
    a.free(t)
    is_div = local(IS_DIV)
    zd = a.mul(miz, is_div)  # mod_is_zero * lv[IS_DIV]
    a.free(is_div)

    def modulus(i):  # modulus[0] += mod_is_zero
        r = local(GENERAL_INPUT_2 + i)
        if i == 0:
            a.add(r, miz, dst=r)
        return r

    def reduced(i):  # output - modulus, with output[0] += mod_is_zero * lv[IS_DIV]
        x = local(GENERAL_INPUT_3 + i)
        if i == 0:
            a.add(x, zd, dst=x)
        y = modulus(i)
        a.sub(x, y, dst=x)
        a.free(y)
        return x

    def is_less_than():
        r = a.imm(1)
        a.sub(r, zd, dst=r)
        return r

    cy = _are_equal(a, flt, col(nxt, MODULAR_OUT_AUX_RED), reduced, a.emit_transition)
    t = is_less_than()
    a.sub(cy, t, dst=cy)
    a.free(t)
    a.mul(cy, flt, dst=cy)
    a.emit_transition(cy)
    a.free(cy, zd)

    def quot(i):
        return local(AUX_INPUT_0_LO + i) if i < N_LIMBS else nxt(MODULAR_QUO_INPUT_HI + i - N_LIMBS)

    # the higher order terms of q(x) m(x) must be zero
    for d in range(2 * N_LIMBS, 3 * N_LIMBS - 1):
        t = _conv(a, d, quot, 2 * N_LIMBS, modulus, N_LIMBS)
        a.mul(t, flt, dst=t)
        a.emit_transition(t)
        a.free(t)
    a.free(flt)
    # constr_poly = c(x) + q(x) m(x) + (x - 2^16) s(x): 32 registers
    constr = []
    for d in range(2 * N_LIMBS):
        c = _conv(a, d, quot, 2 * N_LIMBS, modulus, N_LIMBS)
        if d < N_LIMBS:
            t = local(GENERAL_INPUT_3 + d)
            a.add(c, t, dst=c)
            a.free(t)
        if d < 2 * N_LIMBS - 1:
            t = nxt(MODULAR_AUX_INPUT + d)
            a.mulk(t, LIMB_BITS, dst=t)
            a.sub(c, t, dst=c)
            a.free(t)
        if d:
            t = nxt(MODULAR_AUX_INPUT + d - 1)
            a.add(c, t, dst=c)
            a.free(t)
        constr.append(c)
    a.free(miz)
    # the four operations' inputs against it, each under its own filter
    mul_input = lambda d: _conv(a, d, in0, N_LIMBS, in1, N_LIMBS)  # noqa: E731
    inputs = (
        ((IS_ADDMOD,), lambda d: _pair(a, a.add, local, GENERAL_INPUT_0, local, GENERAL_INPUT_1)(d) if d < N_LIMBS else None),
        ((IS_SUBMOD,), lambda d: _pair(a, a.sub, local, GENERAL_INPUT_0, local, GENERAL_INPUT_1)(d) if d < N_LIMBS else None),
        ((IS_MULMOD,), mul_input),
        ((IS_MOD, IS_DIV), lambda d: in0(d) if d < N_LIMBS else None),
    )
    for flags, operation in inputs:
        f = local(flags[0])
        for other in flags[1:]:
            t = local(other)
            a.add(f, t, dst=f)
            a.free(t)
        for d in range(2 * N_LIMBS):
            t = operation(d)
            if t is None:
                t = a.mul(constr[d], f)
            else:
                a.sub(constr[d], t, dst=t)
                a.mul(t, f, dst=t)
            a.emit_transition(t)
            a.free(t)
        a.free(f)
    return a.program()


def stark_desc(degree_bits, num_challenges, fri_params, constraint_degree=5):
    """ArithmeticStark as a StarkDesc: no public inputs, no permutation pairs. constraint_degree 5 (quotient_degree_factor 4,
    rate_bits >= 2) is what a trace with a DIV row needs; the reference's 3 holds only where no DIV row exists"""
    instrs, immediates = program()
    return StarkDesc(degree_bits, NUM_COLUMNS, 0, constraint_degree, num_challenges, fri_params, instrs, immediates)


def native_program():
    """gl_arithmetic_table_program: (instrs, immediates, number of constraints) as the library emits them — program() word for word"""
    return table.native_program("gl_arithmetic_table_program")


# ---------------------------------------------------------------- cross-table lookups
def _u32_limbs(start):
    """the eight 32-bit limbs of the sixteen 16-bit columns from `start` on"""
    return [CtlColumn.linear_combination([(start + 2 * i, 1), (start + 2 * i + 1, 1 << LIMB_BITS)]) for i in range(N_LIMBS // 2)]


_CTL = {
    "binary": ((IS_ADD, IS_MUL, IS_SUB, IS_LT, IS_GT), (GENERAL_INPUT_0, GENERAL_INPUT_1, GENERAL_INPUT_2), True),
    "modular": ((IS_MOD, IS_ADDMOD, IS_SUBMOD, IS_MULMOD), (GENERAL_INPUT_0, GENERAL_INPUT_1, GENERAL_INPUT_2, GENERAL_INPUT_3), True),
    "div": ((IS_DIV,), (GENERAL_INPUT_0, GENERAL_INPUT_2, AUX_INPUT_0_LO), False),
}


def ctl_data(kind):
    """The looked columns of one of the table's three entries, all on an operation's first row: "binary" the five flags of the
    one-row operators, in0, in1 and GENERAL_INPUT_2 (the result); "modular" the flags of MOD, ADDMOD, SUBMOD, MULMOD, in0, in1, in2
    and GENERAL_INPUT_3 (the result); "div" in0, in2 and columns 76..91 (the quotient). Values are eight 32-bit limbs each."""
    flags, ranges, with_flags = _CTL[kind]
    res = [CtlColumn.single(f) for f in flags] if with_flags else []
    for start in ranges:
        res += _u32_limbs(start)
    return res


def ctl_filter(kind):
    """the sum of the entry's flags"""
    return CtlColumn.sum(list(_CTL[kind][0]))


# ---------------------------------------------------------------- the operations
def result(op, in0, in1, in2=0):
    """the 256-bit result of an operation (arithmetic/mod.rs:33-100); a zero modulus or denominator gives 0. DIV and MOD take the
    denominator as `in2`, as their records do."""
    m = 1 << 256
    if op == OP_ADD:
        return (in0 + in1) % m
    if op == OP_MUL:
        return in0 * in1 % m
    if op == OP_SUB:
        return (in0 - in1) % m
    if op == OP_LT:
        return int(in0 < in1)
    if op == OP_GT:
        return int(in0 > in1)
    if op not in TWO_ROW_OPS:
        raise ValueError("the arithmetic table has no operator %d" % op)
    if in2 == 0:
        return 0
    return {OP_DIV: in0 // in2, OP_MOD: in0 % in2, OP_ADDMOD: (in0 + in1) % in2, OP_SUBMOD: (in0 - in1) % in2, OP_MULMOD: in0 * in1 % in2}[op]


def _limbs(value):
    if isinstance(value, (int, np.integer)):
        if not 0 <= int(value) < 1 << 256:
            raise ValueError("an input is below 2^256")
        return [(int(value) >> (32 * j)) & 0xFFFFFFFF for j in range(8)]
    limbs = [int(v) for v in value]
    if len(limbs) != 8:
        raise ValueError("an input has eight 32-bit limbs")
    return limbs


def ops_to_words(ops):
    """`ops`: an iterable of (op, in0, in1, in2) with `op` one of the OP_* constants and the inputs integers below 2^256 (or
    sequences of their eight 32-bit limbs, least significant first) -> [num_ops][25] uint64. What a record may hold is the trace
    call's to refuse."""
    out = [[int(op)] + _limbs(in0) + _limbs(in1) + _limbs(in2) for op, in0, in1, in2 in ops]
    return np.array(out, dtype=np.uint64).reshape(-1, OP_WORDS)


def _scratch(ctx, num_ops, degree_bits):
    return table.scratch(ctx, "gl_arithmetic_table_scratch_bytes", num_ops, degree_bits,
                         "gl_arithmetic_table_scratch_bytes: num_ops must be at most 2^22 and degree_bits in 1 ..= 22")


def rows(ctx, ops):
    """the rows the operations take: the sum of their row counts. `ops`: host [num_ops][25] words or a DeviceBuffer of them."""
    d_ops, num_ops = table.device_records(ctx, ops, OP_WORDS)
    count = ctypes.c_uint64()
    scratch = _scratch(ctx, num_ops, 1)
    _lib.call("gl_arithmetic_table_trace", table.ptr(d_ops), num_ops, 1, None, 0, scratch.ptr, ctypes.byref(count), ctx.ptr)
    return int(count.value)  # the call has waited for the stream: an upload of this call may go


def generate_trace(ctx, ops, degree_bits=None, trace_stride=None):
    """gl_arithmetic_table_trace: the trace of the operations `ops` ([num_ops][25] words, host array or DeviceBuffer; or the
    iterable ops_to_words takes) with 2^degree_bits rows as a DeviceBuffer [92][trace_stride] (default 2^degree_bits), built on the
    context's stream. degree_bits=None asks for the count first and takes the smallest trace that holds it. The rows the operations
    take are left in the buffer's attribute `rows`."""
    if not isinstance(ops, (DeviceBuffer, np.ndarray)):
        ops = ops_to_words(ops)
    d_ops, num_ops = table.device_records(ctx, ops, OP_WORDS)
    if degree_bits is None:
        degree_bits = max(1, (max(rows(ctx, d_ops) if num_ops else 0, 1) - 1).bit_length())
    # synchronised: the scratch and an upload of this call are released on return
    return table.generate_trace(ctx, "gl_arithmetic_table_trace", [table.ptr(d_ops), num_ops], degree_bits, trace_stride, NUM_COLUMNS,
                                scratch=_scratch(ctx, num_ops, degree_bits), counted=True)
