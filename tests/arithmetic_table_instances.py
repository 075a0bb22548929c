"""Operation lists for the arithmetic table's tests (TEST INFRASTRUCTURE ONLY): [num_ops][25] uint64 records (the operator, the
eight 32-bit limbs of in0, in1, in2) of gl_arithmetic_table_trace, every one within its limits. `edge()` is the fixed list of the
cases a carry chain, the polynomial witness or the device's division can get wrong; DIVISION holds operands found by search with
tests/arithmetic_table_model.py so that every branch of the division is taken (asserted in tests/test_arithmetic_table_ref.py)."""
import numpy as np

ADD, MUL, SUB, DIV, MOD, ADDMOD, SUBMOD, MULMOD, LT, GT = range(10)
ONE_ROW, TWO_ROW = (ADD, MUL, SUB, LT, GT), (DIV, MOD, ADDMOD, SUBMOD, MULMOD)
OP_WORDS = 25
MAX = (1 << 256) - 1


def record(op, in0=0, in1=0, in2=0):
    assert all(0 <= v <= MAX for v in (in0, in1, in2))
    return [op] + [(v >> (32 * j)) & 0xFFFFFFFF for v in (in0, in1, in2) for j in range(8)]


def words(ops):
    return np.array([record(*op) for op in ops], dtype=np.uint64).reshape(-1, OP_WORDS)


def any_op(op, a, b, m):
    """(op, in0, in1, in2) with the must-be-zero input zeroed: one-row operators take (a, b), DIV and MOD (a, m), the others all"""
    if op in ONE_ROW:
        return (op, a, b, 0)
    if op in (DIV, MOD):
        return (op, a, 0, m)
    return (op, a, b, m)


# numerator = in0 (DIV, MOD) or in0 * in1 (MULMOD) by in2: the branches named are those the model counts for them
DIVISION = [
    ("one_too_large", MOD, 0x800000008000000100000001, 0, 0x80000000fffffffe00000000),
    ("two_too_large", DIV, 0xffffffff8000000180000001800000008000000000000000800000017fffffff, 0, 0x80000001fffffffefffffffe00000002fffffffe),
    ("add_back", MOD, 0xfffffffe7fffffff000000010000000080000000, 0, 0xfffffffe7fffffff00000001fffffffe),
    ("add_back", DIV, 0xfffffffe7fffffff000000010000000080000000, 0, 0xfffffffe7fffffff00000001fffffffe),
    ("one_too_large", MULMOD, 0xffffffff0000000100000000ffffffff800000010000000100000002, 0x1fffffffe0000000080000000ffffffff,
     0xfffffffefffffffe7fffffff7ffffffffffffffe80000000),
    ("two_too_large", MULMOD, 0x28000000180000000800000018000000100000002, 0x7fffffff800000017fffffff0000000100000002ffffffff800000007fffffff,
     0x80000001ffffffff00000001ffffffffffffffff7fffffff),
    ("top_equal", MULMOD, 0x800000007fffffff00000002fffffffe80000000ffffffff, 0x800000007fffffff00000001000000000000000000000000ffffffff,
     0x17ffffffffffffffe00000002ffffffff800000017fffffff),
    ("add_back", MULMOD, 0x1000000010000000080000001fffffffe7fffffff0000000280000001, 0x1fffffffe7fffffff80000000fffffffffffffffe80000000,
     0x27ffffffffffffffefffffffe),
]


def numerator_and_modulus(op, in0, in1, in2):
    """what the device divides for a modular operation with a non-zero modulus: (|operation(in0, in1)|, in2)"""
    return abs({DIV: in0, MOD: in0, ADDMOD: in0 + in1, SUBMOD: in0 - in1, MULMOD: in0 * in1}[op]), in2


def edge_ops():
    ops = []
    values = [0, 1, MAX, 1 << 255, (1 << 128) - 1]
    for op in range(10):  # every operator on 0, 1, 2^256 - 1
        for a in values[:3]:
            for b in values[:3]:
                ops.append(any_op(op, a, b, b if op in (DIV, MOD) else 3))
    for k in range(1, 16):  # single set limbs at each 16-bit (and so each 32-bit) boundary
        ops += [(ADD, 1 << (16 * k), (1 << (16 * k)) - 1, 0), (SUB, 1 << (16 * k), 1, 0), (MUL, 1 << (16 * k), (1 << 16) + 1, 0),
                (LT, 1 << (16 * k), (1 << (16 * k)) - 1, 0), (GT, (1 << (16 * k)) - 1, 1 << (16 * k), 0),
                (MOD, MAX, 0, 1 << (16 * k)), (DIV, MAX, 0, (1 << (16 * k)) - 1), (MULMOD, MAX, 1 << (16 * k), (1 << (16 * k)) + 1)]
    # carries and borrows that ripple through all 16 limbs
    ops += [(ADD, MAX, 1, 0), (ADD, 1, MAX, 0), (ADD, MAX, MAX, 0), (SUB, 0, 1, 0), (SUB, 0, MAX, 0), (SUB, 1 << 255, 1, 0),
            (LT, 0, 1, 0), (LT, 1, 0, 0), (LT, 5, 5, 0), (GT, 0, 1, 0), (GT, 1, 0, 0), (GT, MAX, MAX, 0), (LT, MAX - 1, MAX, 0),
            (MUL, MAX, MAX, 0), (MUL, MAX, 2, 0), (MUL, (1 << 128) - 1, (1 << 128) + 1, 0), (MUL, 0xFFFF, 0xFFFF, 0)]
    for op in TWO_ROW:  # modulus 0 (DIV by 0 included), 1, 2^256 - 1
        for m in (0, 1, MAX):
            ops += [any_op(op, MAX, MAX - 1, m), any_op(op, 0x1234567890ABCDEF << 100, 77, m), any_op(op, 0, 0, m)]
    for k in range(1, 17):  # a modulus of 1 .. 16 significant 16-bit limbs
        m = (0x8001 << (16 * (k - 1))) | 0x7F
        for op in TWO_ROW:
            ops.append(any_op(op, MAX - (k << 77), (MAX >> 3) + k, m))
        ops.append((MULMOD, MAX, MAX, (1 << (16 * k)) - 1))
    ops += [(MULMOD, MAX, MAX, 1),  # a 512-bit quotient
            (MULMOD, MAX, MAX, MAX), (MULMOD, MAX, MAX, 2), (ADDMOD, MAX, MAX, 1), (ADDMOD, MAX, MAX, MAX), (ADDMOD, MAX, 1, 2),
            (SUBMOD, 0, MAX, 1), (SUBMOD, 0, MAX, 3), (SUBMOD, 1, MAX, 2), (SUBMOD, 5, 1 << 255, 7),  # in0 < in1, a large negative quotient
            (SUBMOD, 0, 21, 7), (SUBMOD, 7, 7 + (5 << 200), 5 << 100), (SUBMOD, 3, 3, 9),  # an exact multiple of the modulus
            (SUBMOD, MAX, 0, MAX), (SUBMOD, 10, 3, 1 << 255), (SUBMOD, 3, 10, 1 << 255)]
    ops += [(op, a, b, m) for _, op, a, b, m in DIVISION]
    return ops


def edge(num_ops=None):
    ops = edge_ops()
    return words(ops if num_ops is None else [ops[k % len(ops)] for k in range(num_ops)])


def _random_value(rng):
    """a value of 0 .. 256 bits, so that short and long operands and moduli meet"""
    bits = int(rng.integers(0, 257))
    v = int.from_bytes(rng.bytes(32), "little") >> (256 - bits) if bits else 0
    return v


def random_ops(num_ops, seed=92, operators=tuple(range(10))):
    rng = np.random.default_rng(seed)
    ops = []
    for _ in range(num_ops):
        op = operators[int(rng.integers(0, len(operators)))]
        ops.append(any_op(op, _random_value(rng), _random_value(rng), _random_value(rng)))
    return words(ops)


def mixed(num_ops, seed=7):
    """one- and two-row operators interleaved: operator k % 10 in a shuffled order, operands of every length"""
    rng = np.random.default_rng(seed)
    order = [ADD, MULMOD, LT, DIV, MUL, SUBMOD, SUB, MOD, GT, ADDMOD]
    return words([any_op(order[k % 10], _random_value(rng), _random_value(rng), _random_value(rng)) for k in range(num_ops)])


def every_operator():
    """the ten operators once each, 15 rows, and one more ADD: a 16-row trace whose last row is an ADD"""
    ops = [any_op(op, (0xDEADBEEF << 190) + op, (0x12345 << 120) + 17 * op, (1 << 130) + 12345) for op in (DIV, ADD, MULMOD, LT, SUBMOD, MUL, MOD, GT, ADDMOD, SUB)]
    return words(ops + [(ADD, MAX, 1, 0)])


def add_only(num_ops, seed=1):
    return random_ops(num_ops, seed, (ADD,))


def mulmod_only(num_ops, seed=2):
    return random_ops(num_ops, seed, (MULMOD,))


def without_div(num_ops, seed=3):
    return random_ops(num_ops, seed, (ADD, MUL, SUB, MOD, ADDMOD, SUBMOD, MULMOD, LT, GT))


FAMILIES = {"edge": edge, "mixed": mixed, "random": random_ops, "add_only": add_only, "mulmod_only": mulmod_only}
