"""The reference's Keccak sponge table on the host (TEST INFRASTRUCTURE ONLY): a restatement of
KeccakSpongeStark::generate_rows_for_op / generate_trace_rows (evm/src/keccak_sponge/keccak_sponge_stark.rs:190-347) and of
keccak_sponge_log (evm/src/witness/util.rs:178-250) on Python integers, written from the Rust line by line, and the table's
constraints — the reference's list of TODOs (:363-377) — as hand-written closures. Nothing here knows how the device builds the
trace or how the register program is laid out. The permutation is tests/keccak_ref.py's numpy Keccak-f.

The three operation lists are computed from the INPUTS, as keccak_sponge_log does, not from the trace.

The one thing the reference's signature spells differently is `degree_bits`: generate_trace_rows pads to
max(len, min_rows).next_power_of_two() and silently cuts what does not fit; here the caller gives that power's exponent and a trace
that would be cut is an assertion (None: the smallest power of two that holds every row, at least two rows)."""
import numpy as np

import keccak_ref

P = 0xFFFFFFFF00000001

# columns.rs
KECCAK_WIDTH_BYTES = 200
KECCAK_WIDTH_U32S = KECCAK_WIDTH_BYTES // 4
KECCAK_RATE_BYTES = 136
KECCAK_RATE_U32S = KECCAK_RATE_BYTES // 4
KECCAK_CAPACITY_BYTES = 64
KECCAK_CAPACITY_U32S = KECCAK_CAPACITY_BYTES // 4
FIELDS = [("is_full_input_block", 1), ("is_final_block", 1), ("context", 1), ("segment", 1), ("virt", 1), ("timestamp", 1), ("len", 1),
          ("already_absorbed_bytes", 1), ("is_final_input_len", KECCAK_RATE_BYTES), ("original_rate_u32s", KECCAK_RATE_U32S),
          ("original_capacity_u32s", KECCAK_CAPACITY_U32S), ("block_bytes", KECCAK_RATE_BYTES), ("xored_rate_u32s", KECCAK_RATE_U32S),
          ("updated_state_u32s", KECCAK_WIDTH_U32S)]
COL = {}  # name -> range of columns (KECCAK_SPONGE_COL_MAP)
_at = 0
for _name, _count in FIELDS:
    COL[_name] = range(_at, _at + _count)
    _at += _count
NUM_COLUMNS = _at
assert NUM_COLUMNS == 414
OP_WORDS = 5
SEGMENT_CODE = 0  # memory/segments.rs: Segment::Code


def next_power_of_two(x):
    return 1 if x <= 1 else 1 << (x - 1).bit_length()


def keccakf_u32s(state_u32s):
    """keccak_util.rs:6-18"""
    state_u64s = [state_u32s[i * 2] | (state_u32s[i * 2 + 1] << 32) for i in range(25)]
    out = [int(x) for x in keccak_ref.keccak_f1600(np.array(state_u64s, dtype=np.uint64))]
    return [(out[i // 2] >> ((i % 2) * 32)) & 0xFFFFFFFF for i in range(KECCAK_WIDTH_U32S)]


def keccakf_u8s(state_u8s):
    """keccak_util.rs:21-29"""
    state_u64s = [int.from_bytes(bytes(state_u8s[i * 8 : i * 8 + 8]), "little") for i in range(25)]
    out = [int(x) for x in keccak_ref.keccak_f1600(np.array(state_u64s, dtype=np.uint64))]
    return [b for w in out for b in w.to_bytes(8, "little")]


class KeccakSpongeOp:
    def __init__(self, context, segment, virt, timestamp, data):
        self.context, self.segment, self.virt, self.timestamp, self.input = int(context), int(segment), int(virt), int(timestamp), bytes(data)


# ---------------------------------------------------------------- the trace (keccak_sponge_stark.rs:190-347)
def _view():
    return {name: [0] * len(cols) for name, cols in COL.items()}


def _flat(view):
    row = [0] * NUM_COLUMNS
    for name, cols in COL.items():
        row[cols.start : cols.stop] = view[name]
    return row


def generate_common_fields(row, op, already_absorbed_bytes, sponge_state):
    row["context"], row["segment"], row["virt"] = [op.context], [op.segment], [op.virt]
    row["timestamp"], row["len"], row["already_absorbed_bytes"] = [op.timestamp], [len(op.input)], [already_absorbed_bytes]
    sponge_state = list(sponge_state)
    row["original_rate_u32s"] = sponge_state[:KECCAK_RATE_U32S]
    row["original_capacity_u32s"] = sponge_state[KECCAK_RATE_U32S:]
    block_u32s = [int.from_bytes(bytes(row["block_bytes"][i * 4 : (i + 1) * 4]), "little") for i in range(KECCAK_RATE_U32S)]
    for i, block_i in enumerate(block_u32s):
        sponge_state[i] ^= block_i
    row["xored_rate_u32s"] = sponge_state[:KECCAK_RATE_U32S]
    sponge_state = keccakf_u32s(sponge_state)
    row["updated_state_u32s"] = sponge_state


def generate_full_input_row(op, already_absorbed_bytes, sponge_state, block):
    row = _view()
    row["is_full_input_block"] = [1]
    row["block_bytes"] = list(block)
    generate_common_fields(row, op, already_absorbed_bytes, sponge_state)
    return row


def generate_final_row(op, already_absorbed_bytes, sponge_state, final_inputs):
    assert already_absorbed_bytes + len(final_inputs) == len(op.input)
    row = _view()
    row["is_final_block"] = [1]
    for i, b in enumerate(final_inputs):
        row["block_bytes"][i] = b
    if len(final_inputs) == KECCAK_RATE_BYTES - 1:
        row["block_bytes"][len(final_inputs)] = 0b10000001
    else:
        row["block_bytes"][len(final_inputs)] = 1
        row["block_bytes"][KECCAK_RATE_BYTES - 1] = 0b10000000
    row["is_final_input_len"][len(final_inputs)] = 1
    generate_common_fields(row, op, already_absorbed_bytes, sponge_state)
    return row


def generate_rows_for_op(op):
    rows = []
    sponge_state = [0] * KECCAK_WIDTH_U32S
    full = len(op.input) // KECCAK_RATE_BYTES  # chunks_exact
    already_absorbed_bytes = 0
    for k in range(full):
        row = generate_full_input_row(op, already_absorbed_bytes, sponge_state, op.input[k * KECCAK_RATE_BYTES : (k + 1) * KECCAK_RATE_BYTES])
        sponge_state = row["updated_state_u32s"]
        rows.append(_flat(row))
        already_absorbed_bytes += KECCAK_RATE_BYTES
    rows.append(_flat(generate_final_row(op, already_absorbed_bytes, sponge_state, op.input[full * KECCAK_RATE_BYTES :])))
    return rows


def rows_needed(operations):
    return sum(len(op.input) // KECCAK_RATE_BYTES + 1 for op in operations)


def generate_trace_rows(operations, num_rows):
    """flat_map(generate_rows_for_op).chain(repeat(padding)).take(num_rows), for a num_rows that cuts nothing"""
    rows = [row for op in operations for row in generate_rows_for_op(op)]
    assert len(rows) <= num_rows, "the reference would cut an operation in the middle"
    return rows + [[0] * NUM_COLUMNS for _ in range(num_rows - len(rows))]


def trace_of_ops(operations, degree_bits=None):
    """-> [414][n] uint64 columns"""
    n = max(2, next_power_of_two(rows_needed(operations))) if degree_bits is None else 1 << degree_bits
    return np.array(generate_trace_rows(operations, n), dtype=np.uint64).T.copy()


def ops_to_words(operations):
    """-> ([num_ops][5] uint64, uint8 bytes): the input of gl_keccak_sponge_table_trace"""
    words = np.array([[op.context, op.segment, op.virt, op.timestamp, len(op.input)] for op in operations], dtype=np.uint64).reshape(-1, OP_WORDS)
    return words, np.frombuffer(b"".join(op.input for op in operations), dtype=np.uint8).copy()


# ---------------------------------------------------------------- keccak_sponge_log (witness/util.rs:178-250)
class Log:
    """what one call of keccak_sponge_log per operation pushes: the Keccak-f inputs (200 bytes each, as 25 little-endian lanes: the
    records of gl_keccak_table_trace), the logic operations (the [17]-word records of gl_logic_table_trace) and the memory
    operations (the [14]-word records of gl_memory_table_trace)"""

    def __init__(self):
        self.keccak_inputs, self.logic_ops, self.memory_ops = [], [], []

    def push_memory(self, op, address, byte):
        # MemoryOp::new(Code channel, clock, address, Read, byte): timestamp = clock * NUM_CHANNELS + 0 = the sponge op's timestamp
        self.memory_ops.append([1, op.timestamp, 1, op.context, op.segment, address, byte] + [0] * 7)

    def xor_into_sponge(self, sponge_state, block):
        for i in range(0, KECCAK_RATE_BYTES, 32):
            hi = min(KECCAK_RATE_BYTES, i + 32)
            lhs = int.from_bytes(bytes(sponge_state[i:hi]), "little")
            rhs = int.from_bytes(bytes(block[i:hi]), "little")
            self.logic_ops.append([2] + [(lhs >> (32 * j)) & 0xFFFFFFFF for j in range(8)] + [(rhs >> (32 * j)) & 0xFFFFFFFF for j in range(8)])
        for i in range(KECCAK_RATE_BYTES):
            sponge_state[i] ^= block[i]

    def push_keccak_bytes(self, sponge_state):
        self.keccak_inputs.append([int.from_bytes(bytes(sponge_state[8 * j : 8 * j + 8]), "little") for j in range(25)])

    def keccak_sponge_log(self, op):
        address = op.virt
        sponge_state = [0] * KECCAK_WIDTH_BYTES
        full = len(op.input) // KECCAK_RATE_BYTES
        for k in range(full):
            block = list(op.input[k * KECCAK_RATE_BYTES : (k + 1) * KECCAK_RATE_BYTES])
            for byte in block:
                self.push_memory(op, address, byte)
                address += 1
            self.xor_into_sponge(sponge_state, block)
            self.push_keccak_bytes(sponge_state)
            sponge_state = keccakf_u8s(sponge_state)
        remainder = list(op.input[full * KECCAK_RATE_BYTES :])
        for byte in remainder:
            self.push_memory(op, address, byte)
            address += 1
        final_block = [0] * KECCAK_RATE_BYTES
        final_block[: len(remainder)] = remainder
        if len(remainder) == KECCAK_RATE_BYTES - 1:
            final_block[len(remainder)] = 0b10000001
        else:
            final_block[len(remainder)] = 1
            final_block[KECCAK_RATE_BYTES - 1] = 0b10000000
        self.xor_into_sponge(sponge_state, final_block)
        self.push_keccak_bytes(sponge_state)


def log_of_ops(operations):
    """(keccak_inputs [rows][25], logic_ops [5 rows][17], memory_ops [sum of len][14]) as uint64 arrays"""
    log = Log()
    for op in operations:
        log.keccak_sponge_log(op)
    arr = lambda rows, width: np.array(rows, dtype=np.uint64).reshape(-1, width)  # noqa: E731
    return arr(log.keccak_inputs, 25), arr(log.logic_ops, 17), arr(log.memory_ops, 14)


# ---------------------------------------------------------------- the constraints (the list of TODOs, :363-377)
GROUPS = [("flags", 3), ("final_len_boolean", 136), ("final_len_sum", 1), ("first_row", 51), ("after_final", 51), ("same_op", 5), ("state_carried", 50),
          ("absorbed_carried", 1), ("dummy_then_dummy", 1), ("final_len_value", 136)]
KINDS = {"flags": "plain", "final_len_boolean": "plain", "final_len_sum": "plain", "first_row": "first_row", "after_final": "transition",
         "same_op": "transition", "state_carried": "transition", "absorbed_carried": "transition", "dummy_then_dummy": "transition",
         "final_len_value": "plain"}
NUM_CONSTRAINTS = sum(count for _, count in GROUPS)
assert NUM_CONSTRAINTS == 435 and len(GROUPS) == 10


class _Base:
    zero, one = 0, 1
    add = staticmethod(lambda x, y: (x + y) % P)
    sub = staticmethod(lambda x, y: (x - y) % P)
    mul = staticmethod(lambda x, y: x * y % P)
    lift = staticmethod(lambda x: int(x) % P)


def eval_constraints(lv, nv, F=_Base):
    """[(kind, value)] for the 435 constraints in order; kind is "plain", "first_row" or "transition" """
    out = []
    c = lambda name, i=0: COL[name][i]  # noqa: E731
    full, final = lv[c("is_full_input_block")], lv[c("is_final_block")]
    # each flag (full-input block, final block or implied dummy flag) must be boolean
    out.append(("plain", F.mul(full, F.sub(full, F.one))))
    out.append(("plain", F.mul(final, F.sub(final, F.one))))
    out.append(("plain", F.mul(full, final)))
    # is_final_input_len must contain booleans
    for i in range(KECCAK_RATE_BYTES):
        d = lv[c("is_final_input_len", i)]
        out.append(("plain", F.mul(d, F.sub(d, F.one))))
    # sum of is_final_input_len should equal is_final_block
    total = F.zero
    for i in range(KECCAK_RATE_BYTES):
        total = F.add(total, lv[c("is_final_input_len", i)])
    out.append(("plain", F.sub(total, final)))
    state = list(COL["original_rate_u32s"]) + list(COL["original_capacity_u32s"])
    # if this is the first row, the original sponge state should be 0 and already_absorbed_bytes = 0
    for col in state + [c("already_absorbed_bytes")]:
        out.append(("first_row", lv[col]))
    # if this is a final block, the next row's original sponge state should be 0 and already_absorbed_bytes = 0
    for col in state + [c("already_absorbed_bytes")]:
        out.append(("transition", F.mul(final, nv[col])))
    # if this is a full-input block, the next row's address, time and len must match
    for name in ("context", "segment", "virt", "timestamp", "len"):
        out.append(("transition", F.mul(full, F.sub(nv[c(name)], lv[c(name)]))))
    # if this is a full-input block, the next row's "before" should match our "after" state
    for j, col in enumerate(state):
        out.append(("transition", F.mul(full, F.sub(nv[col], lv[c("updated_state_u32s", j)]))))
    # if this is a full-input block, the next row's already_absorbed_bytes should be ours plus 136
    absorbed = c("already_absorbed_bytes")
    out.append(("transition", F.mul(full, F.sub(F.sub(nv[absorbed], lv[absorbed]), F.lift(KECCAK_RATE_BYTES)))))
    # a dummy row is always followed by another dummy row
    dummy = F.sub(F.sub(F.one, full), final)
    out.append(("transition", F.mul(dummy, F.add(nv[c("is_full_input_block")], nv[c("is_final_block")]))))
    # is_final_input_len implies len - already_absorbed == i
    for i in range(KECCAK_RATE_BYTES):
        diff = F.sub(F.sub(lv[c("len")], lv[absorbed]), F.lift(i))
        out.append(("plain", F.mul(lv[c("is_final_input_len", i)], diff)))
    assert len(out) == NUM_CONSTRAINTS
    return out


def group_of(k):
    for name, count in GROUPS:
        if k < count:
            return name, k
        k -= count
    raise IndexError(k)


def violated(cols, r):
    """(group, index within the group) of the constraints that do not hold on row r of the cyclic trace: first-row constraints count
    on row 0 alone, transitions everywhere but on the last row"""
    n = len(cols[0])
    lv, nv = [int(col[r]) for col in cols], [int(col[(r + 1) % n]) for col in cols]
    bad = []
    for k, (kind, v) in enumerate(eval_constraints(lv, nv)):
        applies = kind == "plain" or (kind == "first_row" and r == 0) or (kind == "transition" and r != n - 1)
        if applies and v != 0:
            bad.append(group_of(k))
    return bad


def violations(cols):
    return [(r,) + g for r in range(len(cols[0])) for g in violated(cols, r)]


class KeccakSpongeTableStark:
    """what tests/stark_ref.py and tests/ctl_ref.py take: shape, the register program under test and the closures above"""
    num_columns, num_public_inputs, constraint_degree, pairs = NUM_COLUMNS, 0, 3, []

    def __init__(self, instrs, immediates):
        self.instrs, self.immediates = [tuple(int(x) for x in row) for row in instrs], [int(x) for x in immediates]

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        emit = {"plain": consumer.constraint, "first_row": consumer.constraint_first_row, "transition": consumer.constraint_transition}
        for kind, v in eval_constraints(local, nxt, F):
            emit[kind](v)
