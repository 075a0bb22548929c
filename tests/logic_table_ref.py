"""The reference's logic table on the host (TEST INFRASTRUCTURE ONLY): a restatement of Operation::into_row and
LogicStark::generate_trace_rows (evm/src/logic.rs:100-176) on Python integers and of eval_packed_generic (:182-231) as closures,
written from the Rust line by line. Nothing here knows how the device builds the trace or how the register program is laid out.

The one thing the reference's signature spells differently is `degree_bits`: generate_trace_rows pads to
max(len, min_rows).next_power_of_two(); here the caller gives that power's exponent (None: the reference's with min_rows 0, but at
least two rows, the smallest STARK of this package). There is no Rust toolchain in this project: this model is the truth, and
tests/test_logic_table_ref.py holds it against direct big-integer arithmetic and against its own constraints."""
import numpy as np

P = 0xFFFFFFFF00000001

# logic.rs:21-52
VAL_BITS = 256
PACKED_LIMB_BITS = 32
PACKED_LEN = -(-VAL_BITS // PACKED_LIMB_BITS)
IS_AND = 0
IS_OR = IS_AND + 1
IS_XOR = IS_OR + 1
INPUT0 = range(IS_XOR + 1, IS_XOR + 1 + VAL_BITS)
INPUT1 = range(INPUT0.stop, INPUT0.stop + VAL_BITS)
RESULT = range(INPUT1.stop, INPUT1.stop + PACKED_LEN)
NUM_COLUMNS = RESULT.stop
OP_WORDS = 1 + 2 * PACKED_LEN
AND, OR, XOR = "and", "or", "xor"
FLAG = {AND: IS_AND, OR: IS_OR, XOR: IS_XOR}
OPERATORS = [AND, OR, XOR]  # a record's operator word indexes this list


def limb_bit_cols_for_input(input_bits):
    return [range(input_bits.start + i * PACKED_LIMB_BITS, min(input_bits.start + (i + 1) * PACKED_LIMB_BITS, input_bits.stop)) for i in range(PACKED_LEN)]


def next_power_of_two(x):
    return 1 if x <= 1 else 1 << (x - 1).bit_length()


class Operation:
    def __init__(self, operator, input0, input1):  # Operation::new
        assert operator in FLAG and 0 <= input0 < 1 << 256 and 0 <= input1 < 1 << 256
        self.operator, self.input0, self.input1 = operator, input0, input1
        self.result = {AND: input0 & input1, OR: input0 | input1, XOR: input0 ^ input1}[operator]  # Op::result

    def into_row(self):
        row = [0] * NUM_COLUMNS
        row[FLAG[self.operator]] = 1
        for i in range(256):
            row[INPUT0.start + i] = (self.input0 >> i) & 1
            row[INPUT1.start + i] = (self.input1 >> i) & 1
        result_limbs = [(self.result >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]  # U256 as four u64
        for i, limb in enumerate(result_limbs):
            row[RESULT.start + 2 * i] = limb & 0xFFFFFFFF
            row[RESULT.start + 2 * i + 1] = limb >> 32
        return row


def ops_from_words(words):
    """[num_ops][17] words -> Operations; the limits of gl_logic_table_trace are asserted"""
    ops = []
    for w in words:
        w = [int(x) for x in w]
        assert len(w) == OP_WORDS and w[0] in (0, 1, 2) and all(0 <= x < 1 << 32 for x in w[1:])
        ops.append(Operation(OPERATORS[w[0]], sum(x << (32 * j) for j, x in enumerate(w[1:9])), sum(x << (32 * j) for j, x in enumerate(w[9:17]))))
    return ops


def generate_trace_rows(operations, min_rows=0):
    length = len(operations)
    padded_len = next_power_of_two(max(length, min_rows))
    rows = [op.into_row() for op in operations]
    for _ in range(length, padded_len):
        rows.append([0] * NUM_COLUMNS)
    return rows


def trace_of_words(words, degree_bits=None):
    """-> [523][n] uint64 columns"""
    ops = ops_from_words(words)
    rows = generate_trace_rows(ops, 2 if degree_bits is None else 1 << degree_bits)
    assert degree_bits is None or len(rows) == 1 << degree_bits
    return np.array(rows, dtype=np.uint64).T.copy()


# ---------------------------------------------------------------- the constraints (logic.rs:182-231)
GROUPS = [("input0_bit", 256), ("input1_bit", 256), ("result", 8)]
NUM_CONSTRAINTS = sum(count for _, count in GROUPS)
assert NUM_CONSTRAINTS == 520


class _Base:
    zero, one = 0, 1
    add = staticmethod(lambda x, y: (x + y) % P)
    sub = staticmethod(lambda x, y: (x - y) % P)
    mul = staticmethod(lambda x, y: x * y % P)
    lift = staticmethod(lambda x: int(x) % P)


def limb_from_bits_le(F, bits):  # util.rs: the fold acc.doubles() + bit over the bits, most significant first
    acc = F.zero
    for bit in reversed(list(bits)):
        acc = F.add(F.add(acc, acc), bit)
    return acc


def eval_constraints(lv, F=_Base):
    """the 520 values in the order eval_packed_generic yields them"""
    out = []
    is_and = lv[IS_AND]
    is_or = lv[IS_OR]
    is_xor = lv[IS_XOR]

    sum_coeff = F.add(is_or, is_xor)
    and_coeff = F.sub(F.sub(is_and, is_or), F.mul(is_xor, F.lift(2)))

    for input_bits_cols in (INPUT0, INPUT1):
        for i in input_bits_cols:
            bit = lv[i]
            out.append(F.mul(bit, F.sub(bit, F.one)))

    for result_col, x_bits_cols, y_bits_cols in zip(RESULT, limb_bit_cols_for_input(INPUT0), limb_bit_cols_for_input(INPUT1)):
        x = limb_from_bits_le(F, [lv[col] for col in x_bits_cols])
        y = limb_from_bits_le(F, [lv[col] for col in y_bits_cols])
        x_land_y = F.zero
        for i, (x_col, y_col) in enumerate(zip(x_bits_cols, y_bits_cols)):
            x_land_y = F.add(x_land_y, F.mul(F.mul(lv[x_col], lv[y_col]), F.lift(1 << i)))
        x_op_y = F.add(F.mul(sum_coeff, F.add(x, y)), F.mul(and_coeff, x_land_y))
        out.append(F.sub(lv[result_col], x_op_y))
    assert len(out) == NUM_CONSTRAINTS
    return out


def group_of(k):
    for name, count in GROUPS:
        if k < count:
            return name, k
        k -= count
    raise IndexError(k)


def violated(cols, r):
    """(group, index within the group) of the constraints that do not hold on row r"""
    return [group_of(k) for k, v in enumerate(eval_constraints([int(col[r]) for col in cols])) if v != 0]


def violations(cols):
    return [(r,) + g for r in range(len(cols[0])) for g in violated(cols, r)]


def satisfies_its_constraints(cols):
    return not violations(cols)


class LogicTableStark:
    """what tests/stark_ref.py and tests/ctl_ref.py take: shape, the register program under test and the closures above"""
    num_columns, num_public_inputs, constraint_degree, pairs = NUM_COLUMNS, 0, 3, []

    def __init__(self, instrs, immediates):
        self.instrs, self.immediates = [tuple(int(x) for x in row) for row in instrs], [int(x) for x in immediates]

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        for v in eval_constraints(local, F):
            consumer.constraint(v)
