"""The Poseidon table on the host (TEST INFRASTRUCTURE ONLY): a restatement of generate_permutation_unit and eval_permutation_unit
(system_zero/src/permutation_unit.rs:56-172) and of the column formulas of system_zero/src/registers/permutation.rs on Python
integers, written from the Rust line by line over the constants oracle/pyref.py holds. Nothing here knows how the device builds
the trace or how the register program is laid out.

The reference's unit is a part of a wider row and has no filter; the table's last column IS_REAL, its records (START / ABSORB)
and its padding rows — generate_permutation_unit of the all-zero input, what the reference's generate_trace_rows writes
everywhere — are this project's (include/plonky2_hip.h "The Poseidon table"). trace_of_words asserts on every row it writes that
OUTPUT is pyref.poseidon(INPUT). There is no Rust toolchain in this project: this model is the truth, and
tests/test_poseidon_table_ref.py holds it against its own constraints."""
import operator

import numpy as np

from oracle import pyref

P = 0xFFFFFFFF00000001
SPONGE_WIDTH, SPONGE_RATE = 12, 8
HALF_N_FULL_ROUNDS, N_PARTIAL_ROUNDS = 4, 22
OP_WORDS = 1 + SPONGE_WIDTH

# registers/permutation.rs, START_PERMUTATION = 0
START_PERMUTATION = 0
START_FULL_FIRST = START_PERMUTATION + SPONGE_WIDTH


def col_full_first_mid_sbox(round_, i):
    assert round_ < HALF_N_FULL_ROUNDS and i < SPONGE_WIDTH
    return START_FULL_FIRST + 2 * round_ * SPONGE_WIDTH + i


def col_full_first_after_mds(round_, i):
    assert round_ < HALF_N_FULL_ROUNDS and i < SPONGE_WIDTH
    return START_FULL_FIRST + (2 * round_ + 1) * SPONGE_WIDTH + i


START_PARTIAL = col_full_first_after_mds(HALF_N_FULL_ROUNDS - 1, SPONGE_WIDTH - 1) + 1


def col_partial_mid_sbox(round_):
    assert round_ < N_PARTIAL_ROUNDS
    return START_PARTIAL + 2 * round_


def col_partial_after_sbox(round_):
    assert round_ < N_PARTIAL_ROUNDS
    return START_PARTIAL + 2 * round_ + 1


START_FULL_SECOND = col_partial_after_sbox(N_PARTIAL_ROUNDS - 1) + 1


def col_full_second_mid_sbox(round_, i):
    assert round_ <= HALF_N_FULL_ROUNDS and i < SPONGE_WIDTH
    return START_FULL_SECOND + 2 * round_ * SPONGE_WIDTH + i


def col_full_second_after_mds(round_, i):
    assert round_ <= HALF_N_FULL_ROUNDS and i < SPONGE_WIDTH
    return START_FULL_SECOND + (2 * round_ + 1) * SPONGE_WIDTH + i


def col_input(i):
    assert i < SPONGE_WIDTH
    return START_PERMUTATION + i


def col_output(i):
    assert i < SPONGE_WIDTH
    return col_full_second_after_mds(HALF_N_FULL_ROUNDS - 1, i)


END = col_output(SPONGE_WIDTH - 1) + 1
IS_REAL = END  # this project's
NUM_COLUMNS = IS_REAL + 1


# ---------------------------------------------------------------- thirty plain rounds (Poseidon::constant_layer, mds_layer)
def constant_layer(state, round_):
    return [(x + pyref.ROUND_CONSTANTS[round_ * SPONGE_WIDTH + i]) % P for i, x in enumerate(state)]


# row r of circ(MDS_CIRC) + diag(MDS_DIAG) (Poseidon::mds_layer): entry j is MDS_CIRC[(j - r) mod 12], and MDS_DIAG[r] more at j = r
_MDS_ROWS = [[pyref.MDS_CIRC[(j - r) % SPONGE_WIDTH] + (pyref.MDS_DIAG[r] if j == r else 0) for j in range(SPONGE_WIDTH)] for r in range(SPONGE_WIDTH)]


def mds_layer(state):
    return [sum(map(operator.mul, row, state)) % P for row in _MDS_ROWS]


def generate_permutation_unit(values):
    """permutation_unit.rs:56-105: fills `values` (a row whose INPUT cells are set) in place"""
    state = [values[col_input(i)] for i in range(SPONGE_WIDTH)]
    for r in range(HALF_N_FULL_ROUNDS):
        state = constant_layer(state, r)
        for i in range(SPONGE_WIDTH):
            state_cubed = pow(state[i], 3, P)
            values[col_full_first_mid_sbox(r, i)] = state_cubed
            state[i] = state[i] * state_cubed * state_cubed % P  # state ** 7
        state = mds_layer(state)
        for i in range(SPONGE_WIDTH):
            values[col_full_first_after_mds(r, i)] = state[i]
    for r in range(N_PARTIAL_ROUNDS):
        state = constant_layer(state, HALF_N_FULL_ROUNDS + r)
        state0_cubed = pow(state[0], 3, P)
        values[col_partial_mid_sbox(r)] = state0_cubed
        state[0] = state[0] * state0_cubed * state0_cubed % P
        values[col_partial_after_sbox(r)] = state[0]
        state = mds_layer(state)
    for r in range(HALF_N_FULL_ROUNDS):
        state = constant_layer(state, HALF_N_FULL_ROUNDS + N_PARTIAL_ROUNDS + r)
        for i in range(SPONGE_WIDTH):
            state_cubed = pow(state[i], 3, P)
            values[col_full_second_mid_sbox(r, i)] = state_cubed
            state[i] = state[i] * state_cubed * state_cubed % P
        state = mds_layer(state)
        for i in range(SPONGE_WIDTH):
            values[col_full_second_after_mds(r, i)] = state[i]


def row_of(input_state, is_real):
    values = [0] * NUM_COLUMNS
    for i in range(SPONGE_WIDTH):
        values[col_input(i)] = int(input_state[i]) % P
    generate_permutation_unit(values)
    values[IS_REAL] = 1 if is_real else 0
    inputs, outputs = [values[col_input(i)] for i in range(SPONGE_WIDTH)], [values[col_output(i)] for i in range(SPONGE_WIDTH)]
    assert outputs == pyref.poseidon(inputs)
    return values


def rows_of_words(words):
    """[num_ops][13] records -> the row of every record; the limits of gl_poseidon_table_trace are asserted. An ABSORB's input is
    the OUTPUT of the row before it — which row_of has held against pyref.poseidon — with its elements overwritten."""
    rows = []
    for k, w in enumerate(words):
        w = [int(x) for x in w]
        assert len(w) == OP_WORDS and 0 <= w[0] <= SPONGE_RATE and all(0 <= x < 1 << 64 for x in w)
        if w[0] == 0:
            state = [x % P for x in w[1:]]
        else:
            assert k > 0, "record 0 continues a sponge that no record starts"
            state = [rows[-1][col_output(i)] for i in range(SPONGE_WIDTH)]
            state[: w[0]] = [x % P for x in w[1 : 1 + w[0]]]
        rows.append(row_of(state, True))
    return rows


def inputs_of_words(words):
    """the input state of every record's row"""
    return [row[:SPONGE_WIDTH] for row in rows_of_words(words)]


_PADDING = []


def padding_row():
    if not _PADDING:
        _PADDING.append(row_of([0] * SPONGE_WIDTH, False))
    return list(_PADDING[0])


def trace_of_words(words, degree_bits=None):
    """-> [249][n] uint64 columns; degree_bits None: the smallest trace of at least two rows that holds the records"""
    rows = rows_of_words(words)
    if degree_bits is None:
        degree_bits = max(1, (max(len(rows), 1) - 1).bit_length())
    n = 1 << degree_bits
    assert len(rows) <= n
    rows += [padding_row() for _ in range(n - len(rows))]
    return np.array(rows, dtype=np.uint64).T.copy()


# ---------------------------------------------------------------- the constraints (permutation_unit.rs:108-172)
GROUPS = []
for _r in range(HALF_N_FULL_ROUNDS):
    GROUPS += [("full_first_mid_sbox_%d" % _r, SPONGE_WIDTH), ("full_first_after_mds_%d" % _r, SPONGE_WIDTH)]
for _r in range(N_PARTIAL_ROUNDS):
    GROUPS += [("partial_mid_sbox_%d" % _r, 1), ("partial_after_sbox_%d" % _r, 1)]
for _r in range(HALF_N_FULL_ROUNDS):
    GROUPS += [("full_second_mid_sbox_%d" % _r, SPONGE_WIDTH), ("full_second_after_mds_%d" % _r, SPONGE_WIDTH)]
GROUPS += [("is_real", 1)]
NUM_CONSTRAINTS = sum(count for _, count in GROUPS)
assert NUM_CONSTRAINTS == 237


class _Base:
    zero, one = 0, 1
    add = staticmethod(lambda x, y: (x + y) % P)
    sub = staticmethod(lambda x, y: (x - y) % P)
    mul = staticmethod(lambda x, y: x * y % P)
    lift = staticmethod(lambda x: int(x) % P)


def _constant_layer(F, state, round_):
    return [F.add(x, F.lift(pyref.ROUND_CONSTANTS[round_ * SPONGE_WIDTH + i])) for i, x in enumerate(state)]


def _mds_layer(F, state):
    out = []
    for r in range(SPONGE_WIDTH):
        acc = F.mul(state[r], F.lift(pyref.MDS_DIAG[r]))
        for i in range(SPONGE_WIDTH):
            acc = F.add(acc, F.mul(state[(i + r) % SPONGE_WIDTH], F.lift(pyref.MDS_CIRC[i])))
        out.append(acc)
    return out


def eval_constraints(lv, F=_Base):
    """the 237 values in the order eval_permutation_unit yields them, IS_REAL's last"""
    out = []
    square = lambda x: F.mul(x, x)  # noqa: E731
    state = [lv[col_input(i)] for i in range(SPONGE_WIDTH)]

    def full_rounds(first_round, mid_sbox, after_mds):
        nonlocal state
        for r in range(HALF_N_FULL_ROUNDS):
            state = _constant_layer(F, state, first_round + r)
            for i in range(SPONGE_WIDTH):
                state_cubed = F.mul(state[i], square(state[i]))
                out.append(F.sub(state_cubed, lv[mid_sbox(r, i)]))
                state_cubed = lv[mid_sbox(r, i)]
                state[i] = F.mul(state[i], square(state_cubed))
            state = _mds_layer(F, state)
            for i in range(SPONGE_WIDTH):
                out.append(F.sub(state[i], lv[after_mds(r, i)]))
                state[i] = lv[after_mds(r, i)]

    full_rounds(0, col_full_first_mid_sbox, col_full_first_after_mds)
    for r in range(N_PARTIAL_ROUNDS):
        state = _constant_layer(F, state, HALF_N_FULL_ROUNDS + r)
        state0_cubed = F.mul(state[0], square(state[0]))
        out.append(F.sub(state0_cubed, lv[col_partial_mid_sbox(r)]))
        state0_cubed = lv[col_partial_mid_sbox(r)]
        state[0] = F.mul(state[0], square(state0_cubed))
        out.append(F.sub(state[0], lv[col_partial_after_sbox(r)]))
        state[0] = lv[col_partial_after_sbox(r)]
        state = _mds_layer(F, state)
    full_rounds(HALF_N_FULL_ROUNDS + N_PARTIAL_ROUNDS, col_full_second_mid_sbox, col_full_second_after_mds)
    out.append(F.mul(lv[IS_REAL], F.sub(lv[IS_REAL], F.one)))
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


class PoseidonTableStark:
    """what tests/stark_ref.py and tests/ctl_ref.py take: shape, the register program under test and the closures above"""
    num_columns, num_public_inputs, constraint_degree, pairs = NUM_COLUMNS, 0, 3, []

    def __init__(self, instrs, immediates):
        self.instrs, self.immediates = [tuple(int(x) for x in row) for row in instrs], [int(x) for x in immediates]

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        for v in eval_constraints(local, F):
            consumer.constraint(v)
