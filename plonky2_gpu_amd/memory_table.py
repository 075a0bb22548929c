"""The reference's memory table (evm/src/memory/: memory_stark.rs, columns.rs) as a STARK of this package: 26 columns, one row per
memory operation, dummy read or padding row, constraints of degree 3, one lookup (the range check against COUNTER).

    column indices      columns.rs (NUM_CHANNELS = 6: columns 17 .. 21 are unused and zero)
    program()           eval_packed_generic (memory_stark.rs:242-319) as one StarkAsm register program, the constraints in the
                        reference's order; gl_memory_table_program emits the same words natively
    stark_desc()        the StarkDesc gl_stark_create / gl_stark_tables_create take, with the two permutation pairs
    ctl_data() / ctl_filter()   the cross-table lookup's columns (memory_stark.rs:29-39)
    ops_to_words()      operations -> the [num_ops][14] records gl_memory_table_trace takes: MemoryOp::into_row()[0..14]
    rows()              gl_memory_table_trace without a trace: operations + the dummy reads fill_gaps adds
    generate_trace()    gl_memory_table_trace: generate_trace (memory_stark.rs:122-236) from the unsorted list, built in HBM"""
import ctypes

import numpy as np

from . import _lib, table
from .stark import CtlColumn, StarkAsm, StarkDesc

NUM_CHANNELS = 6
VALUE_LIMBS = 8
FILTER = 0
TIMESTAMP = FILTER + 1
IS_READ = TIMESTAMP + 1
ADDR_CONTEXT = IS_READ + 1
ADDR_SEGMENT = ADDR_CONTEXT + 1
ADDR_VIRTUAL = ADDR_SEGMENT + 1
VALUE_START = ADDR_VIRTUAL + 1
CONTEXT_FIRST_CHANGE = VALUE_START + VALUE_LIMBS
SEGMENT_FIRST_CHANGE = CONTEXT_FIRST_CHANGE + 1
VIRTUAL_FIRST_CHANGE = SEGMENT_FIRST_CHANGE + 1
RANGE_CHECK = VIRTUAL_FIRST_CHANGE + NUM_CHANNELS
COUNTER = RANGE_CHECK + 1
RANGE_CHECK_PERMUTED = COUNTER + 1
COUNTER_PERMUTED = RANGE_CHECK_PERMUTED + 1
NUM_COLUMNS = COUNTER_PERMUTED + 1
assert NUM_COLUMNS == 26
OP_WORDS = VALUE_START + VALUE_LIMBS  # a record of gl_memory_table_trace
NUM_CONSTRAINTS = 23
PAIRS = [[(RANGE_CHECK, RANGE_CHECK_PERMUTED)], [(COUNTER, COUNTER_PERMUTED)]]  # memory_stark.rs:452-456


def value_limb(i):
    assert 0 <= i < VALUE_LIMBS
    return VALUE_START + i


# ---------------------------------------------------------------- the constraints
def program():
    """(instrs [k][4] uint16, immediates): eval_packed_generic, 23 constraints in the reference's order"""
    a = StarkAsm()
    one = a.imm(1)
    # the filter is 0 or 1
    filter_ = a.local(FILTER)
    t = a.sub(filter_, one)
    a.mul(filter_, t, dst=t)
    a.emit(t)
    a.free(t)
    # a dummy row (filter off) is a read
    is_dummy = a.sub(one, filter_)
    is_read = a.local(IS_READ)
    is_write = a.sub(one, is_read)
    t = a.mul(is_dummy, is_write)
    a.emit(t)
    a.free(t, is_dummy, is_write, is_read, filter_)
    # first set of ordering constraints: the first_change flags and address_unchanged are boolean
    context_first_change = a.local(CONTEXT_FIRST_CHANGE)
    segment_first_change = a.local(SEGMENT_FIRST_CHANGE)
    virtual_first_change = a.local(VIRTUAL_FIRST_CHANGE)
    address_unchanged = a.sub(one, context_first_change)
    a.sub(address_unchanged, segment_first_change, dst=address_unchanged)
    a.sub(address_unchanged, virtual_first_change, dst=address_unchanged)
    for flag in (context_first_change, segment_first_change, virtual_first_change, address_unchanged):
        t = a.sub(one, flag)
        a.mul(flag, t, dst=t)
        a.emit(t)
        a.free(t)
    # second set: no change before the column of the flag that is set
    diffs = []
    for column in (ADDR_CONTEXT, ADDR_SEGMENT, ADDR_VIRTUAL, TIMESTAMP):
        nxt = a.next(column)
        local = a.local(column)
        a.sub(nxt, local, dst=nxt)
        a.free(local)
        diffs.append(nxt)
    d_context, d_segment, d_virtual, d_timestamp = diffs
    for flag, diff in ((segment_first_change, d_context), (virtual_first_change, d_context), (virtual_first_change, d_segment),
                       (address_unchanged, d_context), (address_unchanged, d_segment), (address_unchanged, d_virtual)):
        t = a.mul(flag, diff)
        a.emit_transition(t)
        a.free(t)
    # third set: the range check is the difference of the column that should be increasing
    computed = a.sub(d_context, one)
    a.mul(context_first_change, computed, dst=computed)
    for flag, diff in ((segment_first_change, d_segment), (virtual_first_change, d_virtual)):
        t = a.sub(diff, one)
        a.mul(flag, t, dst=t)
        a.add(computed, t, dst=computed)
        a.free(t)
    t = a.mul(address_unchanged, d_timestamp)
    a.add(computed, t, dst=computed)
    a.free(t)
    range_check = a.local(RANGE_CHECK)
    a.sub(range_check, computed, dst=computed)
    a.emit_transition(computed)
    a.free(computed, range_check)
    # the purportedly ordered log: a read of an unchanged address sees the value of the row before
    gate = a.next(IS_READ)
    a.mul(gate, address_unchanged, dst=gate)
    for i in range(VALUE_LIMBS):
        nxt = a.next(value_limb(i))
        local = a.local(value_limb(i))
        a.sub(nxt, local, dst=nxt)
        a.mul(gate, nxt, dst=nxt)
        a.emit(nxt)
        a.free(nxt, local)
    a.release()
    a.eval_lookups(RANGE_CHECK_PERMUTED, COUNTER_PERMUTED)
    return a.program()


def stark_desc(degree_bits, num_challenges, fri_params):
    """MemoryStark as a StarkDesc: constraint_degree 3, no public inputs, the pairs of the range check's lookup"""
    instrs, immediates = program()
    return StarkDesc(degree_bits, NUM_COLUMNS, 0, 3, num_challenges, fri_params, instrs, immediates, PAIRS)


def ctl_data():
    """memory_stark.rs:29-35: IS_READ, the three address parts, the eight limbs, TIMESTAMP"""
    columns = [IS_READ, ADDR_CONTEXT, ADDR_SEGMENT, ADDR_VIRTUAL] + [value_limb(i) for i in range(VALUE_LIMBS)] + [TIMESTAMP]
    return [CtlColumn.single(c) for c in columns]


def ctl_filter():
    """memory_stark.rs:37-39"""
    return CtlColumn.single(FILTER)


def native_program():
    """gl_memory_table_program: (instrs, immediates, number of constraints) as the library emits them — program() word for word"""
    return table.native_program("gl_memory_table_program")


# ---------------------------------------------------------------- the trace
def ops_to_words(ops):
    """`ops`: an iterable of (filter, timestamp, is_read, context, segment, virt, value) with `value` an integer below 2^256 (or a
    sequence of its eight 32-bit limbs, least significant first) -> [num_ops][14] uint64, MemoryOp::into_row()[0..14]"""
    out = []
    for filter_, timestamp, is_read, context, segment, virt, value in ops:
        limbs = [(int(value) >> (32 * j)) & 0xFFFFFFFF for j in range(VALUE_LIMBS)] if isinstance(value, (int, np.integer)) else [int(v) for v in value]
        if len(limbs) != VALUE_LIMBS or (isinstance(value, (int, np.integer)) and not 0 <= int(value) < 1 << 256):
            raise ValueError("a value has eight 32-bit limbs")
        out.append([int(filter_), int(timestamp), int(is_read), int(context), int(segment), int(virt)] + limbs)
    return np.array(out, dtype=np.uint64).reshape(-1, OP_WORDS)


def _device_ops(ctx, ops):
    """(DeviceBuffer, number of operations)"""
    return table.device_records(ctx, ops, OP_WORDS, min_ops=2, too_few="the memory table takes at least two operations")


def _scratch(ctx, num_ops, degree_bits):
    return table.scratch(ctx, "gl_memory_table_scratch_bytes", num_ops, degree_bits,
                         "gl_memory_table_scratch_bytes: num_ops must be in 2 ..= 2^30 and degree_bits in 1 ..= 23")


def _count(ctx, d_ops, num_ops):
    rows = ctypes.c_uint64()
    scratch = _scratch(ctx, num_ops, 1)
    _lib.call("gl_memory_table_trace", d_ops.ptr, num_ops, 1, None, 0, scratch.ptr, ctypes.byref(rows), ctx.ptr)
    return int(rows.value)


def rows(ctx, ops):
    """operations + the dummy reads fill_gaps adds: the rows the trace needs before its padding. `ops`: host [num_ops][14] words or
    a DeviceBuffer of them."""
    d_ops, num_ops = _device_ops(ctx, ops)
    return _count(ctx, d_ops, num_ops)  # the call has waited for the stream: an upload of this call may go


def generate_trace(ctx, ops, degree_bits=None, trace_stride=None):
    """gl_memory_table_trace: the trace of the unsorted operations `ops` ([num_ops][14] words, host array or DeviceBuffer) with
    2^degree_bits rows as a DeviceBuffer [26][trace_stride] (default 2^degree_bits), built on the context's stream.
    degree_bits=None asks for the count first and takes the smallest trace that holds it, the reference's. The rows needed are
    left in the buffer's attribute `rows`."""
    d_ops, num_ops = _device_ops(ctx, ops)
    if degree_bits is None:
        degree_bits = max(1, (_count(ctx, d_ops, num_ops) - 1).bit_length())
    # synchronised: the scratch and an upload of this call are released on return
    return table.generate_trace(ctx, "gl_memory_table_trace", [d_ops.ptr, num_ops], degree_bits, trace_stride, NUM_COLUMNS,
                                scratch=_scratch(ctx, num_ops, degree_bits), counted=True)

