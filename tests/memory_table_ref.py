"""The reference's memory table on the host (TEST INFRASTRUCTURE ONLY): a LITERAL restatement of MemoryStark::generate_trace
(evm/src/memory/memory_stark.rs:122-236) with MemoryOp (evm/src/witness/memory.rs:70-115) and of eval_packed_generic (:242-319),
written from the Rust line by line. Nothing here knows how the device builds the trace: two stable sorts, the fill_gaps loop over
the windows of a clone with its mutated `curr`, pad_memory_ops from last(), the flags with the reference's assert, COUNTER, and
permuted_cols from tests/lookup_ref.py.

The one thing the reference does not have is `degree_bits` in generate_trace: pad_memory_ops pads to next_power_of_two of the
vector's length; with degree_bits it pads to 2^degree_bits instead (more padding rows; max_rc is taken before, from the number of
operations, and stays). There is no Rust toolchain in this project: this model is the truth, and tests/test_memory_table_ref.py
holds it against a hand-worked example and against its own constraints."""
import numpy as np

import lookup_ref

P = 0xFFFFFFFF00000001

# memory/columns.rs
NUM_CHANNELS = 6
VALUE_LIMBS = 8
FILTER = 0
TIMESTAMP = FILTER + 1
IS_READ = TIMESTAMP + 1
ADDR_CONTEXT = IS_READ + 1
ADDR_SEGMENT = ADDR_CONTEXT + 1
ADDR_VIRTUAL = ADDR_SEGMENT + 1
VALUE_START = ADDR_VIRTUAL + 1


def value_limb(i):
    assert i < VALUE_LIMBS
    return VALUE_START + i


CONTEXT_FIRST_CHANGE = VALUE_START + VALUE_LIMBS
SEGMENT_FIRST_CHANGE = CONTEXT_FIRST_CHANGE + 1
VIRTUAL_FIRST_CHANGE = SEGMENT_FIRST_CHANGE + 1
RANGE_CHECK = VIRTUAL_FIRST_CHANGE + NUM_CHANNELS
COUNTER = RANGE_CHECK + 1
RANGE_CHECK_PERMUTED = COUNTER + 1
COUNTER_PERMUTED = RANGE_CHECK_PERMUTED + 1
NUM_COLUMNS = COUNTER_PERMUTED + 1
OP_WORDS = VALUE_START + VALUE_LIMBS


def next_power_of_two(x):
    return 1 if x <= 1 else 1 << (x - 1).bit_length()


# ---------------------------------------------------------------- witness/memory.rs
class MemoryOp:
    """Copy, like the Rust struct: `replace` gives the changed copy"""
    __slots__ = ("filter", "timestamp", "is_read", "context", "segment", "virt", "value")

    def __init__(self, filter, timestamp, is_read, context, segment, virt, value):  # noqa: A002
        self.filter, self.timestamp, self.is_read = bool(filter), int(timestamp), bool(is_read)
        self.context, self.segment, self.virt = int(context), int(segment), int(virt)
        self.value = tuple(int(v) for v in value)  # the eight 32-bit limbs of the U256, least significant first

    def replace(self, **changes):
        fields = {k: getattr(self, k) for k in self.__slots__}
        fields.update(changes)
        return MemoryOp(**fields)

    @classmethod
    def new_dummy_read(cls, context, segment, virt, timestamp):  # memory.rs:97-105
        return cls(False, timestamp, True, context, segment, virt, (0,) * VALUE_LIMBS)

    def sorting_key(self):  # :107-114
        return (self.context, self.segment, self.virt, self.timestamp)

    def into_row(self):  # memory_stark.rs:51-68
        row = [0] * NUM_COLUMNS
        row[FILTER] = int(self.filter)
        row[TIMESTAMP] = self.timestamp
        row[IS_READ] = int(self.is_read)
        row[ADDR_CONTEXT] = self.context
        row[ADDR_SEGMENT] = self.segment
        row[ADDR_VIRTUAL] = self.virt
        for j in range(VALUE_LIMBS):
            row[value_limb(j)] = self.value[j]
        return row


def ops_from_words(words):
    """[num_ops][14] words (into_row()[0..14]) -> MemoryOps; the limits of gl_memory_table_trace are asserted"""
    ops = []
    for w in words:
        w = [int(x) for x in w]
        assert len(w) == OP_WORDS and w[FILTER] in (0, 1) and w[IS_READ] in (0, 1) and all(0 <= x < 1 << 32 for x in w)
        ops.append(MemoryOp(w[FILTER], w[TIMESTAMP], w[IS_READ], w[ADDR_CONTEXT], w[ADDR_SEGMENT], w[ADDR_VIRTUAL], w[VALUE_START:]))
    return ops


# ---------------------------------------------------------------- memory_stark.rs:72-236
def generate_first_change_flags_and_rc(trace_rows):
    num_ops = len(trace_rows)
    for idx in range(num_ops - 1):
        row = trace_rows[idx]
        next_row = trace_rows[idx + 1]

        context = row[ADDR_CONTEXT]
        segment = row[ADDR_SEGMENT]
        virt = row[ADDR_VIRTUAL]
        timestamp = row[TIMESTAMP]
        next_context = next_row[ADDR_CONTEXT]
        next_segment = next_row[ADDR_SEGMENT]
        next_virt = next_row[ADDR_VIRTUAL]
        next_timestamp = next_row[TIMESTAMP]

        context_changed = context != next_context
        segment_changed = segment != next_segment
        virtual_changed = virt != next_virt

        context_first_change = context_changed
        segment_first_change = segment_changed and not context_first_change
        virtual_first_change = virtual_changed and not segment_first_change and not context_first_change

        row[CONTEXT_FIRST_CHANGE] = int(context_first_change)
        row[SEGMENT_FIRST_CHANGE] = int(segment_first_change)
        row[VIRTUAL_FIRST_CHANGE] = int(virtual_first_change)

        if context_first_change:
            row[RANGE_CHECK] = (next_context - context - 1) % P
        elif segment_first_change:
            row[RANGE_CHECK] = (next_segment - segment - 1) % P
        elif virtual_first_change:
            row[RANGE_CHECK] = (next_virt - virt - 1) % P
        else:
            row[RANGE_CHECK] = (next_timestamp - timestamp) % P

        assert row[RANGE_CHECK] < num_ops, "Range check of %d is too large. Bug in fill_gaps?" % row[RANGE_CHECK]


def fill_gaps(memory_ops):
    max_rc = next_power_of_two(len(memory_ops)) - 1
    clone = list(memory_ops)
    for curr, nxt in zip(clone, clone[1:]):  # tuple_windows; `curr` is mutable in the loop body
        if curr.context != nxt.context or curr.segment != nxt.segment:
            pass  # no check of context or segment gaps
        elif curr.virt != nxt.virt:
            while nxt.virt - curr.virt - 1 > max_rc:
                dummy_read = MemoryOp.new_dummy_read(curr.context, curr.segment, curr.virt + max_rc + 1, 0)
                memory_ops.append(dummy_read)
                curr = dummy_read
        else:
            while nxt.timestamp - curr.timestamp > max_rc:
                dummy_read = MemoryOp.new_dummy_read(curr.context, curr.segment, curr.virt, curr.timestamp + max_rc)
                memory_ops.append(dummy_read)
                curr = dummy_read


def pad_memory_ops(memory_ops, num_ops_padded=None):
    last_op = memory_ops[-1]
    padding_op = last_op.replace(filter=False, is_read=True)
    num_ops = len(memory_ops)
    if num_ops_padded is None:
        num_ops_padded = next_power_of_two(num_ops)
    assert num_ops_padded >= num_ops
    for _ in range(num_ops, num_ops_padded):
        memory_ops.append(padding_op)


def generate_trace_row_major(memory_ops, degree_bits=None):
    memory_ops = list(memory_ops)
    memory_ops.sort(key=MemoryOp.sorting_key)  # stable, as sort_by_key
    fill_gaps(memory_ops)
    rows_needed = len(memory_ops)
    pad_memory_ops(memory_ops, None if degree_bits is None else 1 << degree_bits)
    memory_ops.sort(key=MemoryOp.sorting_key)
    trace_rows = [op.into_row() for op in memory_ops]
    generate_first_change_flags_and_rc(trace_rows)
    return trace_rows, rows_needed


def generate_trace_col_major(trace_col_vecs):
    height = len(trace_col_vecs[0])
    trace_col_vecs[COUNTER] = list(range(height))
    permuted_inputs, permuted_table = lookup_ref.permuted_cols(trace_col_vecs[RANGE_CHECK], trace_col_vecs[COUNTER])
    trace_col_vecs[RANGE_CHECK_PERMUTED] = permuted_inputs
    trace_col_vecs[COUNTER_PERMUTED] = permuted_table


def generate_trace(memory_ops, degree_bits=None):
    """-> ([26][n] columns of ints, operations + dummies)"""
    trace_rows, rows_needed = generate_trace_row_major(memory_ops, degree_bits)
    trace_col_vecs = [[row[c] for row in trace_rows] for c in range(NUM_COLUMNS)]  # transpose
    generate_trace_col_major(trace_col_vecs)
    return trace_col_vecs, rows_needed


def trace_of_words(words, degree_bits=None):
    """-> ([26][n] uint64 array, operations + dummies)"""
    cols, rows_needed = generate_trace(ops_from_words(words), degree_bits)
    return np.array(cols, dtype=np.uint64), rows_needed


def rows_needed(words):
    ops = sorted(ops_from_words(words), key=MemoryOp.sorting_key)
    fill_gaps(ops)
    return len(ops)


# ---------------------------------------------------------------- the constraints (memory_stark.rs:242-319, lookup.rs:13-34)
ALL, TRANSITION, LAST_ROW = "constraint", "transition", "last_row"
GROUPS = [("filter_boolean", 1), ("dummy_is_read", 1), ("flags_boolean", 4), ("no_change_before", 6), ("range_check", 1), ("values", 8), ("lookup", 2)]
NUM_CONSTRAINTS = sum(count for _, count in GROUPS)
assert NUM_CONSTRAINTS == 23


class _Base:
    zero, one = 0, 1
    add = staticmethod(lambda x, y: (x + y) % P)
    sub = staticmethod(lambda x, y: (x - y) % P)
    mul = staticmethod(lambda x, y: x * y % P)


def eval_constraints(local, nxt, F=_Base):
    """[(kind, value)] in the order eval_packed_generic yields them"""
    out = []
    one = F.one

    timestamp = local[TIMESTAMP]
    addr_context = local[ADDR_CONTEXT]
    addr_segment = local[ADDR_SEGMENT]
    addr_virtual = local[ADDR_VIRTUAL]
    values = [local[value_limb(i)] for i in range(8)]

    next_timestamp = nxt[TIMESTAMP]
    next_is_read = nxt[IS_READ]
    next_addr_context = nxt[ADDR_CONTEXT]
    next_addr_segment = nxt[ADDR_SEGMENT]
    next_addr_virtual = nxt[ADDR_VIRTUAL]
    next_values = [nxt[value_limb(i)] for i in range(8)]

    filter_ = local[FILTER]
    out.append((ALL, F.mul(filter_, F.sub(filter_, one))))

    is_dummy = F.sub(one, filter_)
    is_write = F.sub(one, local[IS_READ])
    out.append((ALL, F.mul(is_dummy, is_write)))

    context_first_change = local[CONTEXT_FIRST_CHANGE]
    segment_first_change = local[SEGMENT_FIRST_CHANGE]
    virtual_first_change = local[VIRTUAL_FIRST_CHANGE]
    address_unchanged = F.sub(F.sub(F.sub(one, context_first_change), segment_first_change), virtual_first_change)

    range_check = local[RANGE_CHECK]

    not_context_first_change = F.sub(one, context_first_change)
    not_segment_first_change = F.sub(one, segment_first_change)
    not_virtual_first_change = F.sub(one, virtual_first_change)
    not_address_unchanged = F.sub(one, address_unchanged)

    out.append((ALL, F.mul(context_first_change, not_context_first_change)))
    out.append((ALL, F.mul(segment_first_change, not_segment_first_change)))
    out.append((ALL, F.mul(virtual_first_change, not_virtual_first_change)))
    out.append((ALL, F.mul(address_unchanged, not_address_unchanged)))

    out.append((TRANSITION, F.mul(segment_first_change, F.sub(next_addr_context, addr_context))))
    out.append((TRANSITION, F.mul(virtual_first_change, F.sub(next_addr_context, addr_context))))
    out.append((TRANSITION, F.mul(virtual_first_change, F.sub(next_addr_segment, addr_segment))))
    out.append((TRANSITION, F.mul(address_unchanged, F.sub(next_addr_context, addr_context))))
    out.append((TRANSITION, F.mul(address_unchanged, F.sub(next_addr_segment, addr_segment))))
    out.append((TRANSITION, F.mul(address_unchanged, F.sub(next_addr_virtual, addr_virtual))))

    computed_range_check = F.add(
        F.add(
            F.add(F.mul(context_first_change, F.sub(F.sub(next_addr_context, addr_context), one)),
                  F.mul(segment_first_change, F.sub(F.sub(next_addr_segment, addr_segment), one))),
            F.mul(virtual_first_change, F.sub(F.sub(next_addr_virtual, addr_virtual), one))),
        F.mul(address_unchanged, F.sub(next_timestamp, timestamp)))
    out.append((TRANSITION, F.sub(range_check, computed_range_check)))

    for i in range(8):
        out.append((ALL, F.mul(F.mul(next_is_read, address_unchanged), F.sub(next_values[i], values[i]))))

    # eval_lookups(vars, yield_constr, RANGE_CHECK_PERMUTED, COUNTER_PERMUTED)
    local_perm_input = local[RANGE_CHECK_PERMUTED]
    next_perm_table = nxt[COUNTER_PERMUTED]
    next_perm_input = nxt[RANGE_CHECK_PERMUTED]
    diff_input_prev = F.sub(next_perm_input, local_perm_input)
    diff_input_table = F.sub(next_perm_input, next_perm_table)
    out.append((ALL, F.mul(diff_input_prev, diff_input_table)))
    out.append((LAST_ROW, diff_input_table))
    assert len(out) == NUM_CONSTRAINTS
    return out


def group_of(k):
    for name, count in GROUPS:
        if k < count:
            return name, k
        k -= count
    raise IndexError(k)


def violated(cols, r):
    """(group, index within the group) of the constraints that do not hold on row r of the columns `cols` (next row r + 1,
    wrapping): transition constraints are not checked on the last row, last-row constraints only there"""
    n = len(cols[0])
    local, nxt = [int(col[r]) for col in cols], [int(col[(r + 1) % n]) for col in cols]
    bad = []
    for k, (kind, v) in enumerate(eval_constraints(local, nxt)):
        if kind == TRANSITION and r == n - 1:
            continue
        if kind == LAST_ROW and r != n - 1:
            continue
        if v != 0:
            bad.append(group_of(k))
    return bad


def violations(cols):
    return [(r,) + g for r in range(len(cols[0])) for g in violated(cols, r)]


def satisfies_its_constraints(cols):
    """every constraint on every row, the wrap-around row included, and the lookup argument between RANGE_CHECK and COUNTER"""
    if violations(cols):
        return False
    lookup_ref.check_lookup_argument(cols[RANGE_CHECK], cols[COUNTER], cols[RANGE_CHECK_PERMUTED], cols[COUNTER_PERMUTED])
    return True


class MemoryTableStark:
    """what tests/stark_ref.py and tests/ctl_ref.py take: shape, pairs, the register program under test and the closures above"""
    num_columns, num_public_inputs, constraint_degree = NUM_COLUMNS, 0, 3
    pairs = [[(RANGE_CHECK, RANGE_CHECK_PERMUTED)], [(COUNTER, COUNTER_PERMUTED)]]  # memory_stark.rs:452-456

    def __init__(self, instrs, immediates):
        self.instrs, self.immediates = [tuple(int(x) for x in row) for row in instrs], [int(x) for x in immediates]

    @staticmethod
    def closure(F, local, nxt, pis, consumer):
        for kind, v in eval_constraints(local, nxt, F):
            getattr(consumer, kind)(v) if kind == ALL else getattr(consumer, "constraint_" + kind)(v)
