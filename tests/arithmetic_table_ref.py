"""The reference's arithmetic table on the host (TEST INFRASTRUCTURE ONLY): add / sub / mul / compare / modular::generate
(evm/src/arithmetic/) restated on Python integers and their eval_packed_generic as closures, written from the Rust line by line.
Nothing here knows how the device divides or how the register program is laid out.

The reference's snapshot has no generate_trace: the rows of the TABLE are this project's definition —
operations in list order, a modular operation's second row with all flags zero, every cell the reference does not write zero,
zero rows behind the operations. tests/test_arithmetic_table_ref.py holds this model against direct big-integer arithmetic and
against its own constraints."""
import numpy as np

P = 0xFFFFFFFF00000001
LIMB_BITS, N_LIMBS = 16, 16
BASE, MASK = 1 << LIMB_BITS, (1 << LIMB_BITS) - 1
# columns.rs:25-117
IS_ADD, IS_MUL, IS_SUB, IS_DIV, IS_MOD, IS_ADDMOD, IS_SUBMOD, IS_MULMOD, IS_LT, IS_GT, IS_SHL, IS_SHR = range(12)
START_SHARED_COLS = IS_SHR + 1
GENERAL_INPUT_0 = range(START_SHARED_COLS, START_SHARED_COLS + N_LIMBS)
GENERAL_INPUT_1 = range(GENERAL_INPUT_0.stop, GENERAL_INPUT_0.stop + N_LIMBS)
GENERAL_INPUT_2 = range(GENERAL_INPUT_1.stop, GENERAL_INPUT_1.stop + N_LIMBS)
GENERAL_INPUT_3 = range(GENERAL_INPUT_2.stop, GENERAL_INPUT_2.stop + N_LIMBS)
AUX_INPUT_0_LO = range(GENERAL_INPUT_3.stop, GENERAL_INPUT_3.stop + N_LIMBS)
AUX_INPUT_0_HI = range(START_SHARED_COLS, START_SHARED_COLS + N_LIMBS)
AUX_INPUT_1 = range(AUX_INPUT_0_HI.stop, AUX_INPUT_0_HI.stop + 2 * N_LIMBS)
AUX_INPUT_2 = range(AUX_INPUT_1.stop, AUX_INPUT_1.stop + N_LIMBS)
MODULAR_INPUT_0, MODULAR_INPUT_1, MODULAR_MODULUS, MODULAR_OUTPUT = GENERAL_INPUT_0, GENERAL_INPUT_1, GENERAL_INPUT_2, GENERAL_INPUT_3
MODULAR_QUO_INPUT_LO, MODULAR_QUO_INPUT_HI = AUX_INPUT_0_LO, AUX_INPUT_0_HI
MODULAR_AUX_INPUT = range(AUX_INPUT_1.start, AUX_INPUT_1.stop - 1)
MODULAR_MOD_IS_ZERO = AUX_INPUT_1.stop - 1
MODULAR_OUT_AUX_RED = AUX_INPUT_2
DIV_OUTPUT = MODULAR_QUO_INPUT_LO
CMP_OUTPUT = GENERAL_INPUT_2.start
NUM_COLUMNS = START_SHARED_COLS + 5 * N_LIMBS
assert NUM_COLUMNS == 92
OP_WORDS = 25
ONE_ROW = (IS_ADD, IS_MUL, IS_SUB, IS_LT, IS_GT)
MODULAR = (IS_DIV, IS_MOD, IS_ADDMOD, IS_SUBMOD, IS_MULMOD)
NAMES = {IS_ADD: "ADD", IS_MUL: "MUL", IS_SUB: "SUB", IS_DIV: "DIV", IS_MOD: "MOD", IS_ADDMOD: "ADDMOD", IS_SUBMOD: "SUBMOD",
         IS_MULMOD: "MULMOD", IS_LT: "LT", IS_GT: "GT"}


def limbs16(x, n=N_LIMBS):
    assert 0 <= x < 1 << (LIMB_BITS * n)
    return [(x >> (LIMB_BITS * i)) & MASK for i in range(n)]


def value_of(limbs):
    """columns_to_bigint: the polynomial at 2^16"""
    return sum(int(c) << (LIMB_BITS * i) for i, c in enumerate(limbs))


def signed_limbs(x, n):
    """bigint_to_columns: the limbs of |x|, every one negated where x is negative"""
    mag = limbs16(abs(x), n)
    return [-c for c in mag] if x < 0 else mag


def canonical(v):
    """from_noncanonical_i64"""
    return v % P


# ---------------------------------------------------------------- utils.rs
def pol_mul_wide(a, b):
    res = [0] * (len(a) + len(b) - 1)
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            res[i + j] += ai * bj
    return res


def pol_mul_lo(a, b):
    return [sum(a[i] * b[deg - i] for i in range(deg + 1)) for deg in range(len(a))]


def pol_remove_root_2exp(a):
    """utils.rs:343-367 with EXP = 16: Python's >> is the arithmetic shift of i64"""
    n = len(a)
    q = [0] * n
    q[0] = -(a[0] >> LIMB_BITS)
    for deg in range(1, n - 1):
        q[deg] = (q[deg - 1] - a[deg]) >> LIMB_BITS
    return q


def pol_adjoin_root(F, a, root):
    res = [F.sub(F.zero, F.mul(root, a[0]))]
    for deg in range(1, len(a)):
        res.append(F.sub(a[deg - 1], F.mul(root, a[deg])))
    return res


# ---------------------------------------------------------------- generate
def u256_add_cc(a, b):
    out, cy = [], 0
    for x, y in zip(a, b):
        s = x + y + cy
        cy = s >> LIMB_BITS
        assert cy <= 1
        out.append(s & MASK)
    return out, cy


def u256_sub_br(a, b):
    out, br = [], 0
    for x, y in zip(a, b):
        d = BASE + x - y - br
        br = 1 - (d >> LIMB_BITS)
        assert br <= 1
        out.append(d & MASK)
    return out, br


def _put(row, cols, values):
    values = list(values)
    assert len(values) == len(cols)
    for c, v in zip(cols, values):
        row[c] = canonical(v)


def generate_add(lv):
    out, _ = u256_add_cc([lv[c] for c in GENERAL_INPUT_0], [lv[c] for c in GENERAL_INPUT_1])
    _put(lv, GENERAL_INPUT_2, out)


def generate_sub(lv):
    out, _ = u256_sub_br([lv[c] for c in GENERAL_INPUT_0], [lv[c] for c in GENERAL_INPUT_1])
    _put(lv, GENERAL_INPUT_2, out)


def generate_mul(lv):
    """mul.rs:69-100"""
    input0, input1 = [lv[c] for c in GENERAL_INPUT_0], [lv[c] for c in GENERAL_INPUT_1]
    output_limbs, cy = [0] * N_LIMBS, 0
    unreduced_prod = pol_mul_lo(input0, input1)
    for col in range(N_LIMBS):
        t = unreduced_prod[col] + cy
        cy = t >> LIMB_BITS
        output_limbs[col] = t & MASK
    _put(lv, GENERAL_INPUT_2, output_limbs)
    unreduced_prod = [u - o for u, o in zip(unreduced_prod, output_limbs)]
    aux_limbs = pol_remove_root_2exp(unreduced_prod)
    aux_limbs[N_LIMBS - 1] = -cy
    _put(lv, GENERAL_INPUT_3, aux_limbs)


def generate_compare(lv, op):
    """compare.rs:29-43"""
    input0, input1 = [lv[c] for c in GENERAL_INPUT_0], [lv[c] for c in GENERAL_INPUT_1]
    diff, br = u256_sub_br(input0, input1) if op == IS_LT else u256_sub_br(input1, input0)
    _put(lv, GENERAL_INPUT_3, diff)
    lv[CMP_OUTPUT] = br


def generate_modular(lv, nv, op):
    """generate_modular_op (modular.rs:193-287)"""
    input0_limbs, input1_limbs = [lv[c] for c in MODULAR_INPUT_0], [lv[c] for c in MODULAR_INPUT_1]
    modulus_limbs = [lv[c] for c in MODULAR_MODULUS]
    modulus = value_of(modulus_limbs)
    operation = {IS_ADDMOD: lambda a, b: [x + y for x, y in zip(a, b)] + [0] * (N_LIMBS - 1),
                 IS_SUBMOD: lambda a, b: [x - y for x, y in zip(a, b)] + [0] * (N_LIMBS - 1),
                 IS_MULMOD: pol_mul_wide,
                 IS_MOD: lambda a, b: list(a) + [0] * (N_LIMBS - 1),
                 IS_DIV: lambda a, b: list(a) + [0] * (N_LIMBS - 1)}[op]
    constr_poly = operation(input0_limbs, input1_limbs) + [0]
    assert len(constr_poly) == 2 * N_LIMBS
    two_exp_256 = 1 << 256
    mod_is_zero = 0
    if modulus == 0:
        if op == IS_DIV:
            modulus = two_exp_256
        else:
            modulus = 1
            modulus_limbs[0] = 1
        mod_is_zero = 1
    inp = value_of(constr_poly)
    # BigInt's % truncates: the remainder has the sign of the input, and the modulus is added to a negative one
    output = abs(inp) % modulus
    if inp < 0:
        output = -output
    if output < 0:
        output += modulus
    output_limbs = signed_limbs(output, N_LIMBS)
    assert (inp - output) % modulus == 0
    quot = (inp - output) // modulus
    quot_limbs = signed_limbs(quot, 2 * N_LIMBS)
    out_aux_red = signed_limbs(two_exp_256 + output - modulus, N_LIMBS)
    constr_poly = [c - o for c, o in zip(constr_poly, output_limbs + [0] * N_LIMBS)]
    prod = pol_mul_wide(quot_limbs, modulus_limbs)
    constr_poly = [c - p for c, p in zip(constr_poly, prod[: 2 * N_LIMBS])]
    assert all(x == 0 for x in prod[2 * N_LIMBS :])
    assert all(abs(c) < 1 << 37 for c in constr_poly)
    aux_limbs = pol_remove_root_2exp(constr_poly)
    _put(lv, MODULAR_OUTPUT, output_limbs)
    _put(lv, MODULAR_QUO_INPUT_LO, quot_limbs[:N_LIMBS])
    _put(nv, MODULAR_QUO_INPUT_HI, quot_limbs[N_LIMBS:])
    _put(nv, MODULAR_AUX_INPUT, aux_limbs[: 2 * N_LIMBS - 1])
    nv[MODULAR_MOD_IS_ZERO] = mod_is_zero
    _put(nv, MODULAR_OUT_AUX_RED, out_aux_red)


def generate(lv, nv):
    """ArithmeticStark::generate (arithmetic_stark.rs:20-66)"""
    flags = [lv[c] for c in range(12)]
    assert sorted(flags) == [0] * 11 + [1]
    op = flags.index(1)
    if op == IS_ADD:
        generate_add(lv)
    elif op == IS_SUB:
        generate_sub(lv)
    elif op == IS_MUL:
        generate_mul(lv)
    elif op in (IS_LT, IS_GT):
        generate_compare(lv, op)
    elif op in MODULAR:
        generate_modular(lv, nv, op)
    else:
        raise ValueError("the requested operation should not be handled by the arithmetic table")


# ---------------------------------------------------------------- the table (this project's definition)
def int_of_words(limbs):
    return sum(int(x) << (32 * j) for j, x in enumerate(limbs))


def ops_from_words(words):
    """[num_ops][25] words -> (op, in0, in1, in2); the limits of gl_arithmetic_table_trace are asserted"""
    ops = []
    for w in words:
        w = [int(x) for x in w]
        assert len(w) == OP_WORDS and w[0] in NAMES and all(0 <= x < 1 << 32 for x in w[1:])
        op, in0, in1, in2 = w[0], int_of_words(w[1:9]), int_of_words(w[9:17]), int_of_words(w[17:25])
        assert in2 == 0 if op in ONE_ROW else True
        assert in1 == 0 if op in (IS_DIV, IS_MOD) else True
        ops.append((op, in0, in1, in2))
    return ops


def rows_of_op(op, in0, in1, in2):
    lv, nv = [0] * NUM_COLUMNS, [0] * NUM_COLUMNS
    lv[op] = 1
    _put(lv, GENERAL_INPUT_0, limbs16(in0))
    _put(lv, GENERAL_INPUT_1, limbs16(in1))
    _put(lv, GENERAL_INPUT_2, limbs16(in2))
    generate(lv, nv)
    return [lv, nv] if op in MODULAR else [lv]


def next_power_of_two(x):
    return 1 if x <= 1 else 1 << (x - 1).bit_length()


def num_rows(words):
    return sum(2 if int(w[0]) in MODULAR else 1 for w in words)


def trace_of_words(words, degree_bits=None):
    """-> [92][n] uint64 columns; degree_bits None: the smallest trace of at least two rows that holds the operations"""
    rows = [row for op in ops_from_words(words) for row in rows_of_op(*op)]
    n = max(2, next_power_of_two(len(rows))) if degree_bits is None else 1 << degree_bits
    assert len(rows) <= n
    rows += [[0] * NUM_COLUMNS for _ in range(n - len(rows))]
    return np.array(rows, dtype=np.uint64).T.copy()


def result_of_rows(op, rows):
    """the 256-bit result as the table holds it"""
    lv = rows[0]
    cols = {IS_DIV: DIV_OUTPUT}.get(op, MODULAR_OUTPUT if op in MODULAR else GENERAL_INPUT_2)
    return value_of([lv[c] for c in cols])


# ---------------------------------------------------------------- the constraints
PLAIN, TRANSITION, LAST_ROW = "constraint", "constraint_transition", "constraint_last_row"
GROUPS = [("add", 16), ("sub", 16), ("mul", 16), ("cmp_bit", 1), ("lt", 17), ("gt", 17), ("mod_last_row", 1), ("mod_is_zero", 2),
          ("mod_reduced", 17), ("mod_high", 15), ("addmod", 32), ("submod", 32), ("mulmod", 32), ("mod_div", 32)]
NUM_CONSTRAINTS = sum(count for _, count in GROUPS)
assert NUM_CONSTRAINTS == 246


def group_of(k):
    for name, count in GROUPS:
        if k < count:
            return name, k
        k -= count
    raise IndexError(k)


class _Base:
    zero, one = 0, 1
    add = staticmethod(lambda x, y: (x + y) % P)
    sub = staticmethod(lambda x, y: (x - y) % P)
    mul = staticmethod(lambda x, y: x * y % P)
    lift = staticmethod(lambda x: int(x) % P)


def _are_equal(F, out, kind, is_op, larger, smaller):
    """eval_packed_generic_are_equal (add.rs:33-62)"""
    overflow = F.lift(BASE)
    overflow_inv = F.lift(pow(BASE, P - 2, P))
    cy = F.zero
    for a, b in zip(larger, smaller):
        t = F.sub(F.add(cy, a), b)
        out.append((kind, F.mul(F.mul(is_op, t), F.sub(overflow, t))))
        cy = F.mul(t, overflow_inv)
    return cy


def _lt(F, out, kind, is_op, input0, input1, aux, output):
    """eval_packed_generic_lt (compare.rs:53-81)"""
    lhs_limbs = [F.sub(a, b) for a, b in zip(input0, input1)]
    cy = _are_equal(F, out, kind, is_op, aux, lhs_limbs)
    out.append((kind, F.mul(is_op, F.sub(cy, output))))


def _f_pol_mul(F, a, b, n):
    res = [F.zero] * n
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            res[i + j] = F.add(res[i + j], F.mul(ai, bj))
    return res


def eval_constraints(lv, nv, F=_Base):
    """[(kind, value)] in the order ArithmeticStark::eval_packed_generic yields them (arithmetic_stark.rs:72-87)"""
    out = []
    rd = lambda row, cols: [row[c] for c in cols]  # noqa: E731
    in0, in1, in2, in3 = (rd(lv, c) for c in (GENERAL_INPUT_0, GENERAL_INPUT_1, GENERAL_INPUT_2, GENERAL_INPUT_3))
    # add.rs:116-140
    _are_equal(F, out, PLAIN, lv[IS_ADD], [F.add(a, b) for a, b in zip(in0, in1)], in2)
    # sub.rs:40-62
    _are_equal(F, out, PLAIN, lv[IS_SUB], in2, [F.sub(a, b) for a, b in zip(in0, in1)])
    # mul.rs:102-146
    constr_poly = [F.zero] * N_LIMBS
    for deg in range(N_LIMBS):
        for i in range(deg + 1):
            constr_poly[deg] = F.add(constr_poly[deg], F.mul(in0[i], in1[deg - i]))
    constr_poly = [F.sub(c, o) for c, o in zip(constr_poly, in2)]
    constr_poly = [F.sub(c, r) for c, r in zip(constr_poly, pol_adjoin_root(F, in3, F.lift(BASE)))]
    for c in constr_poly:
        out.append((PLAIN, F.mul(lv[IS_MUL], c)))
    # compare.rs:83-104
    is_lt, is_gt, output = lv[IS_LT], lv[IS_GT], lv[CMP_OUTPUT]
    out.append((PLAIN, F.mul(F.mul(F.add(is_lt, is_gt), output), F.sub(output, F.one))))
    _lt(F, out, PLAIN, is_lt, in0, in1, in3, output)
    _lt(F, out, PLAIN, is_gt, in1, in0, in3, output)
    # modular.rs:407-459
    flt = F.add(F.add(F.add(F.add(lv[IS_ADDMOD], lv[IS_MULMOD]), lv[IS_MOD]), lv[IS_SUBMOD]), lv[IS_DIV])
    out.append((LAST_ROW, flt))
    # modular_constr_poly (:316-404)
    modulus = list(in2)
    mod_is_zero = nv[MODULAR_MOD_IS_ZERO]
    out.append((TRANSITION, F.mul(flt, F.sub(F.mul(mod_is_zero, mod_is_zero), mod_is_zero))))
    limb_sum = F.zero
    for m in modulus:
        limb_sum = F.add(limb_sum, m)
    out.append((TRANSITION, F.mul(F.mul(flt, limb_sum), mod_is_zero)))
    modulus[0] = F.add(modulus[0], mod_is_zero)
    output = list(in3)
    output[0] = F.add(output[0], F.mul(mod_is_zero, lv[IS_DIV]))
    out_aux_red = rd(nv, MODULAR_OUT_AUX_RED)
    is_less_than = F.sub(F.one, F.mul(mod_is_zero, lv[IS_DIV]))
    _lt(F, out, TRANSITION, flt, output, modulus, out_aux_red, is_less_than)
    output[0] = F.sub(output[0], F.mul(mod_is_zero, lv[IS_DIV]))
    quot = rd(lv, MODULAR_QUO_INPUT_LO) + rd(nv, MODULAR_QUO_INPUT_HI)
    prod = _f_pol_mul(F, quot, modulus, 3 * N_LIMBS - 1)
    for x in prod[2 * N_LIMBS :]:
        out.append((TRANSITION, F.mul(flt, x)))
    constr_poly = prod[: 2 * N_LIMBS]
    for i, o in enumerate(output):
        constr_poly[i] = F.add(constr_poly[i], o)
    aux = rd(nv, MODULAR_AUX_INPUT) + [F.zero]
    for i, r in enumerate(pol_adjoin_root(F, aux, F.lift(BASE))):
        constr_poly[i] = F.add(constr_poly[i], r)
    pad = [F.zero] * (N_LIMBS - 1)
    add_input = [F.add(a, b) for a, b in zip(in0, in1)] + pad
    sub_input = [F.sub(a, b) for a, b in zip(in0, in1)] + pad
    mul_input = _f_pol_mul(F, in0, in1, 2 * N_LIMBS - 1)
    mod_input = list(in0) + pad
    for inp, f in ((add_input, lv[IS_ADDMOD]), (sub_input, lv[IS_SUBMOD]), (mul_input, lv[IS_MULMOD]), (mod_input, F.add(lv[IS_MOD], lv[IS_DIV]))):
        copy = list(constr_poly)
        for i, x in enumerate(inp):
            copy[i] = F.sub(copy[i], x)
        for c in copy:
            out.append((TRANSITION, F.mul(f, c)))
    assert len(out) == NUM_CONSTRAINTS
    return out


def row_values(cols, r, last_row_counts=True):
    """the 246 constraint values on row r of a trace, as the vanishing polynomial sees them: plain as they are, transitions zeroed
    on the last row, last-row constraints zeroed elsewhere. The next row of the last row is row 0."""
    n = len(cols[0])
    lv, nv = [int(col[r]) for col in cols], [int(col[(r + 1) % n]) for col in cols]
    values = []
    for kind, v in eval_constraints(lv, nv):
        if (kind == TRANSITION and r == n - 1) or (kind == LAST_ROW and r != n - 1):
            v = 0
        values.append(v)
    return values


def violations(cols):
    """(row, group, index within the group) of the constraints that do not hold"""
    return [(r,) + group_of(k) for r in range(len(cols[0])) for k, v in enumerate(row_values(cols, r)) if v != 0]


class ArithmeticTableStark:
    """what tests/stark_ref.py and tests/ctl_ref.py take: shape, the register program under test and the closures above"""
    num_columns, num_public_inputs, pairs = NUM_COLUMNS, 0, []

    def __init__(self, instrs, immediates, constraint_degree=5):
        self.instrs, self.immediates = [tuple(int(x) for x in row) for row in instrs], [int(x) for x in immediates]
        self.constraint_degree = constraint_degree

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        for kind, v in eval_constraints(local, nxt, F):
            getattr(consumer, kind)(v)
