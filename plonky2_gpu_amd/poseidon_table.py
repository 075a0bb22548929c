"""The Poseidon table: the permutation unit of the reference's system_zero crate (system_zero/src/permutation_unit.rs,
system_zero/src/registers/permutation.rs with START_PERMUTATION = 0) as a STARK of this package — 249 columns, one width-12 Poseidon
permutation over Goldilocks per row with every cell constraints of degree 3 need, no lookups of its own. It is the looked table
of one cross-table lookup, "permutation": whoever hashes (Merkle paths, sponges, hash chains) looks its (input, output) pairs up
here.

    column indices      registers/permutation.rs, and IS_REAL behind them
    program()           eval_permutation_unit (permutation_unit.rs:108-172) as one StarkAsm register program, the constraints in
                        the reference's order, then IS_REAL (IS_REAL - 1); gl_poseidon_table_program emits the same words natively
    stark_desc()        the StarkDesc gl_stark_create / gl_stark_tables_create take
    ctl_data() / ctl_filter()   the cross-table lookup's columns
    ops_to_words()      (kind, elements) -> the [num_ops][13] records gl_poseidon_table_trace takes
    generate_trace()    gl_poseidon_table_trace: generate_permutation_unit (permutation_unit.rs:56-105) on every row, built in HBM
    permute_ops() / hash_no_pad_ops() / two_to_one_ops()   the records of plain permutations, of a sponge hash, of a compression

IS_REAL is not the reference's: its unit has no filter because nothing looks into it yet. The rows are this package's as well,
as the arithmetic table's are: one row per record in list order, and behind them the row the reference's generate_trace_rows
writes everywhere — the permutation of the all-zero state — with IS_REAL = 0. A padding row is not a zero row: the constraints
hold on every row.

A record's kind is KIND_START (words 1 .. 12: the whole input state) or k = 1 .. 8 (ABSORB: the row continues the sponge of the row
before it; its input is that row's OUTPUT with elements 0 .. k - 1 overwritten, the overwrite mode of hash_n_to_m_no_pad)."""
import numpy as np

from . import _lib, table
from .device import DeviceBuffer
from .poseidon_tables import TABLES
from .stark import CtlColumn, StarkAsm, StarkDesc

SPONGE_WIDTH, SPONGE_RATE = 12, 8
HALF_N_FULL_ROUNDS, N_PARTIAL_ROUNDS = 4, 22
START_PERMUTATION = 0
INPUT = START_PERMUTATION
START_FULL_FIRST = START_PERMUTATION + SPONGE_WIDTH


def col_input(i):
    return START_PERMUTATION + i


def col_full_first_mid_sbox(r, i):
    return START_FULL_FIRST + 2 * r * SPONGE_WIDTH + i


def col_full_first_after_mds(r, i):
    return START_FULL_FIRST + (2 * r + 1) * SPONGE_WIDTH + i


START_PARTIAL = col_full_first_after_mds(HALF_N_FULL_ROUNDS - 1, SPONGE_WIDTH - 1) + 1


def col_partial_mid_sbox(r):
    return START_PARTIAL + 2 * r


def col_partial_after_sbox(r):
    return START_PARTIAL + 2 * r + 1


START_FULL_SECOND = col_partial_after_sbox(N_PARTIAL_ROUNDS - 1) + 1


def col_full_second_mid_sbox(r, i):
    return START_FULL_SECOND + 2 * r * SPONGE_WIDTH + i


def col_full_second_after_mds(r, i):
    return START_FULL_SECOND + (2 * r + 1) * SPONGE_WIDTH + i


def col_output(i):
    return col_full_second_after_mds(HALF_N_FULL_ROUNDS - 1, i)


OUTPUT = col_output(0)
IS_REAL = col_output(SPONGE_WIDTH - 1) + 1  # this package's: 1 on a row a record made, 0 on padding
NUM_COLUMNS = IS_REAL + 1
assert NUM_COLUMNS == 249 == _lib.GL_POSEIDON_TABLE_COLUMNS
KIND_START = 0  # an ABSORB's kind is the number of elements it overwrites, 1 .. SPONGE_RATE
OP_WORDS = 1 + SPONGE_WIDTH  # a record of gl_poseidon_table_trace
assert OP_WORDS == _lib.GL_POSEIDON_TABLE_OP_WORDS
NUM_CONSTRAINTS = 2 * HALF_N_FULL_ROUNDS * 2 * SPONGE_WIDTH + 2 * N_PARTIAL_ROUNDS + 1
assert NUM_CONSTRAINTS == 237
MAX_DEGREE_BITS = _lib.GL_POSEIDON_TABLE_MAX_DEGREE_BITS


# ---------------------------------------------------------------- the constraints
def program():
    """(instrs [k][4] uint16, immediates): eval_permutation_unit, 236 constraints in the reference's order, then IS_REAL's"""
    a = StarkAsm()
    state = [a.local(col_input(i)) for i in range(SPONGE_WIDTH)]

    def constant_layer(round_):
        for i in range(SPONGE_WIDTH):
            c = a.imm(TABLES["ALL_ROUND_CONSTANTS"][round_ * SPONGE_WIDTH + i])
            a.add(state[i], c, dst=state[i])
            a.free(c)

    def sbox(i, column):
        """state_cubed - mid_sbox; then state * mid_sbox^2 from the column"""
        x2 = a.mul(state[i], state[i])
        a.mul(x2, state[i], dst=x2)
        mid = a.local(column)
        a.emit(a.sub(x2, mid, dst=x2))
        a.mul(mid, mid, dst=x2)
        a.mul(state[i], x2, dst=state[i])
        a.free(x2, mid)

    def mds_layer():
        # row r = MDS_DIAG[r] state[r] + sum_i MDS_CIRC[i] state[(i + r) % 12] through accumulator 0: the weights of a row sum to 264
        new = []
        for r in range(SPONGE_WIDTH):
            terms = [(state[(i + r) % SPONGE_WIDTH], TABLES["MDS_CIRC"][i]) for i in range(SPONGE_WIDTH)]
            if TABLES["MDS_DIAG"][r]:
                terms.append((state[r], TABLES["MDS_DIAG"][r]))
            new.append(a.weighted_sum(terms))
        for i in range(SPONGE_WIDTH):
            a.free(state[i])
            state[i] = new[i]

    def check_against(i, column):
        """state - column; the column from here on"""
        cell = a.local(column)
        a.emit(a.sub(state[i], cell, dst=state[i]))
        a.free(state[i])
        state[i] = cell

    def full_rounds(first_round, mid_sbox, after_mds):
        for r in range(HALF_N_FULL_ROUNDS):
            constant_layer(first_round + r)
            for i in range(SPONGE_WIDTH):
                sbox(i, mid_sbox(r, i))
            mds_layer()
            for i in range(SPONGE_WIDTH):
                check_against(i, after_mds(r, i))

    full_rounds(0, col_full_first_mid_sbox, col_full_first_after_mds)
    for r in range(N_PARTIAL_ROUNDS):
        constant_layer(HALF_N_FULL_ROUNDS + r)
        sbox(0, col_partial_mid_sbox(r))
        check_against(0, col_partial_after_sbox(r))
        mds_layer()
    full_rounds(HALF_N_FULL_ROUNDS + N_PARTIAL_ROUNDS, col_full_second_mid_sbox, col_full_second_after_mds)
    a.release()
    real = a.local(IS_REAL)
    a.emit(a.mul(real, a.sub(real, a.imm(1))))
    return a.program()


def stark_desc(degree_bits, num_challenges, fri_params):
    """the permutation unit as a StarkDesc: constraint_degree 3, no public inputs, no permutation pairs"""
    instrs, immediates = program()
    return StarkDesc(degree_bits, NUM_COLUMNS, 0, 3, num_challenges, fri_params, instrs, immediates)


def ctl_data():
    """the looked entry "permutation": the twelve INPUT and the twelve OUTPUT columns"""
    return [CtlColumn.single(col_input(i)) for i in range(SPONGE_WIDTH)] + [CtlColumn.single(col_output(i)) for i in range(SPONGE_WIDTH)]


def ctl_filter():
    return CtlColumn.single(IS_REAL)


def native_program():
    """gl_poseidon_table_program: (instrs, immediates, number of constraints) as the library emits them — program() word for word"""
    return table.native_program("gl_poseidon_table_program")


# ---------------------------------------------------------------- the records
def _elements(values, count, what):
    out = [int(v) for v in values]
    if len(out) != count:
        raise ValueError("%s takes %d elements, not %d" % (what, count, len(out)))
    if any(not 0 <= v < 1 << 64 for v in out):
        raise ValueError("an element is a word of 64 bits")
    return out


def ops_to_words(ops):
    """`ops`: an iterable of (kind, elements) — (KIND_START, the twelve elements of the input state) or (k, the k elements an
    ABSORB overwrites), k = 1 .. 8; elements are any u64, the device reduces them -> [num_ops][13] uint64"""
    out = []
    for kind, elements in ops:
        kind = int(kind)
        if not 0 <= kind <= SPONGE_RATE:
            raise ValueError("the kind of record %d is not 0 (START) or 1 .. 8 (ABSORB)" % len(out))
        if kind != KIND_START and not out:
            raise ValueError("record 0 is an ABSORB: it continues a sponge that no record starts")
        words = _elements(elements, kind or SPONGE_WIDTH, "a START" if kind == KIND_START else "an ABSORB of kind %d" % kind)
        out.append([kind] + words + [0] * (SPONGE_WIDTH - len(words)))
    return np.array(out, dtype=np.uint64).reshape(-1, OP_WORDS)


def permute_ops(states):
    """one START per state of twelve elements: plain permutations"""
    return [(KIND_START, state) for state in states]


def hash_no_pad_ops(message):
    """hash_n_to_m_no_pad's permutations for a message of at least one element: a START with the first chunk over zeros, then
    ABSORBs of 8 and of the remainder. OUTPUT[0 .. 4] of the last row is the hash."""
    message = list(message)
    if not message:
        raise ValueError("a message has at least one element")
    first = message[:SPONGE_RATE]
    ops = [(KIND_START, first + [0] * (SPONGE_WIDTH - len(first)))]
    for at in range(SPONGE_RATE, len(message), SPONGE_RATE):
        chunk = message[at:at + SPONGE_RATE]
        ops.append((len(chunk), chunk))
    return ops


def two_to_one_ops(left, right):
    """Hasher::two_to_one of two digests of four elements: one START over (left, right, 0, 0, 0, 0); OUTPUT[0 .. 4] is the digest"""
    left, right = _elements(left, 4, "a digest"), _elements(right, 4, "a digest")
    return [(KIND_START, left + right + [0] * 4)]


# ---------------------------------------------------------------- the trace
def generate_trace(ctx, ops, degree_bits=None, trace_stride=None):
    """gl_poseidon_table_trace: the trace of the records `ops` ([num_ops][13] words, host array or DeviceBuffer) with 2^degree_bits
    rows as a DeviceBuffer [249][trace_stride] (default 2^degree_bits), built on the context's stream: the list order is the row
    order, the rows behind the records are the permutation of the all-zero state with IS_REAL = 0. degree_bits=None takes the
    smallest trace that holds them."""
    d_ops, num_ops = table.device_records(ctx, ops, OP_WORDS)
    if degree_bits is None:
        degree_bits = max(1, (max(num_ops, 1) - 1).bit_length())
    scratch = DeviceBuffer(ctx, _lib.GL_POSEIDON_TABLE_SCRATCH_BYTES // 8)
    uploaded = d_ops is not None and d_ops is not ops  # the upload's buffer is released on return: the kernel must have read it
    return table.generate_trace(ctx, "gl_poseidon_table_trace", [table.ptr(d_ops), num_ops], degree_bits, trace_stride, NUM_COLUMNS,
                                scratch=scratch, synchronize=uploaded)
