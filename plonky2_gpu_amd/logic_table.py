"""The reference's logic table (evm/src/logic.rs) as a STARK of this package: 523 columns, one row per AND / OR / XOR of two
256-bit words, zero rows behind them, constraints of degree 3, no lookups of its own. It is the looked table of ctl_logic: the CPU
table's AND / OR / XOR and the Keccak sponge's byte XORs look into it.

    column indices      logic.rs:28-52
    program()           eval_packed_generic (logic.rs:182-231) as one StarkAsm register program, the constraints in the reference's
                        order; gl_logic_table_program emits the same words natively
    stark_desc()        the StarkDesc gl_stark_create / gl_stark_tables_create take
    ctl_data() / ctl_filter()   the cross-table lookup's columns (logic.rs:54-68)
    ops_to_words()      (op, input0, input1) -> the [num_ops][17] records gl_logic_table_trace takes
    generate_trace()    gl_logic_table_trace: generate_trace_rows (logic.rs:157-176) built in HBM

The 32-bit recompositions and the weighted sum of the 32 bit products run through an ACC accumulator in two blocks of 16 weights
2^0 .. 2^15 joined by one shift, as the Keccak-f table's do: 32 weights up to 2^31 on one accumulator would break its overflow
contract."""
import numpy as np

from . import _lib, table
from .device import DeviceBuffer
from .keccak_table import _limb
from .stark import CtlColumn, StarkAsm, StarkDesc

VAL_BITS = 256
PACKED_LIMB_BITS = 32
PACKED_LEN = VAL_BITS // PACKED_LIMB_BITS
IS_AND = 0
IS_OR = IS_AND + 1
IS_XOR = IS_OR + 1
INPUT0 = IS_XOR + 1  # the first of 256 bit columns, least significant first
INPUT1 = INPUT0 + VAL_BITS
RESULT = INPUT1 + VAL_BITS  # the first of eight 32-bit limbs
NUM_COLUMNS = RESULT + PACKED_LEN
assert NUM_COLUMNS == 523 == _lib.GL_LOGIC_TABLE_COLUMNS
OP_AND, OP_OR, OP_XOR = IS_AND, IS_OR, IS_XOR  # a record's operator is the index of its flag column
OP_WORDS = 1 + 2 * PACKED_LEN  # a record of gl_logic_table_trace
assert OP_WORDS == _lib.GL_LOGIC_TABLE_OP_WORDS
NUM_CONSTRAINTS = 2 * VAL_BITS + PACKED_LEN


def limb_bit_cols_for_input(input_start):
    """logic.rs:43-49: per limb, the 32 bit columns it is packed from"""
    return [list(range(input_start + i * PACKED_LIMB_BITS, input_start + (i + 1) * PACKED_LIMB_BITS)) for i in range(PACKED_LEN)]


# ---------------------------------------------------------------- the constraints
def program():
    """(instrs [k][4] uint16, immediates): eval_packed_generic, 520 constraints in the reference's order"""
    a = StarkAsm()
    # all bits are indeed bits
    for start in (INPUT0, INPUT1):
        for i in range(VAL_BITS):
            a.release()
            bit = a.local(start + i)
            a.emit(a.mul(bit, a.sub(bit, a.imm(1))))
    # RESULT[i] = sum_coeff (x + y) + and_coeff (x AND y) on the limb's 32 bits
    for i in range(PACKED_LEN):
        a.release()
        x = _limb(a, lambda z: a.local(INPUT0 + z), 32 * i)
        y = _limb(a, lambda z: a.local(INPUT1 + z), 32 * i)

        def product(z):
            x_bit, y_bit = a.local(INPUT0 + z), a.local(INPUT1 + z)
            a.mul(x_bit, y_bit, dst=x_bit)
            a.free(y_bit)
            return x_bit

        x_land_y = _limb(a, product, 32 * i)
        is_and, is_or, is_xor = a.local(IS_AND), a.local(IS_OR), a.local(IS_XOR)
        sum_coeff = a.add(is_or, is_xor)
        and_coeff = a.sub(is_and, is_or)
        a.mulk(is_xor, 1, dst=is_xor)
        a.sub(and_coeff, is_xor, dst=and_coeff)
        a.add(x, y, dst=x)
        a.mul(sum_coeff, x, dst=x)
        a.mul(and_coeff, x_land_y, dst=x_land_y)
        a.add(x, x_land_y, dst=x)
        a.emit(a.sub(a.local(RESULT + i), x))
    return a.program()


def stark_desc(degree_bits, num_challenges, fri_params):
    """LogicStark as a StarkDesc: constraint_degree 3, no public inputs, no permutation pairs"""
    instrs, immediates = program()
    return StarkDesc(degree_bits, NUM_COLUMNS, 0, 3, num_challenges, fri_params, instrs, immediates)


def ctl_data():
    """logic.rs:54-64: the three flags, the eight limbs of each input recomposed from their bits, the eight result limbs"""
    res = [CtlColumn.single(IS_AND), CtlColumn.single(IS_OR), CtlColumn.single(IS_XOR)]
    res += [CtlColumn.le_bits(cols) for cols in limb_bit_cols_for_input(INPUT0)]
    res += [CtlColumn.le_bits(cols) for cols in limb_bit_cols_for_input(INPUT1)]
    res += [CtlColumn.single(RESULT + i) for i in range(PACKED_LEN)]
    return res


def ctl_filter():
    """logic.rs:66-68"""
    return CtlColumn.sum([IS_AND, IS_OR, IS_XOR])


def native_program():
    """gl_logic_table_program: (instrs, immediates, number of constraints) as the library emits them — program() word for word"""
    return table.native_program("gl_logic_table_program")


# ---------------------------------------------------------------- the trace
def _limbs(value):
    if isinstance(value, (int, np.integer)):
        if not 0 <= int(value) < 1 << VAL_BITS:
            raise ValueError("an input is below 2^256")
        return [(int(value) >> (32 * j)) & 0xFFFFFFFF for j in range(PACKED_LEN)]
    limbs = [int(v) for v in value]
    if len(limbs) != PACKED_LEN:
        raise ValueError("an input has eight 32-bit limbs")
    return limbs


def ops_to_words(ops):
    """`ops`: an iterable of (op, input0, input1) with `op` one of OP_AND, OP_OR, OP_XOR and the inputs integers below 2^256 (or
    sequences of their eight 32-bit limbs, least significant first) -> [num_ops][17] uint64"""
    out = [[int(op)] + _limbs(input0) + _limbs(input1) for op, input0, input1 in ops]
    return np.array(out, dtype=np.uint64).reshape(-1, OP_WORDS)


def generate_trace(ctx, ops, degree_bits=None, trace_stride=None):
    """gl_logic_table_trace: the trace of the operations `ops` ([num_ops][17] words, host array or DeviceBuffer) with
    2^degree_bits rows as a DeviceBuffer [523][trace_stride] (default 2^degree_bits), built on the context's stream: the list order
    is the row order, the rows behind the operations are zero. degree_bits=None takes the smallest trace that holds them, the
    reference's."""
    d_ops, num_ops = table.device_records(ctx, ops, OP_WORDS)
    if degree_bits is None:
        degree_bits = max(1, (max(num_ops, 1) - 1).bit_length())
    scratch = DeviceBuffer(ctx, _lib.GL_LOGIC_TABLE_SCRATCH_BYTES // 8)
    uploaded = d_ops is not None and d_ops is not ops  # the upload's buffer is released on return: the kernel must have read it
    return table.generate_trace(ctx, "gl_logic_table_trace", [table.ptr(d_ops), num_ops], degree_bits, trace_stride, NUM_COLUMNS,
                                scratch=scratch, synchronize=uploaded)
