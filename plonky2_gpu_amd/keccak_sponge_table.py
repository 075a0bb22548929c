"""The reference's Keccak sponge table (evm/src/keccak_sponge/) as a STARK of this package: 414 columns, len / 136 + 1 rows per
hashed byte string, zero rows behind them. It ties the Keccak-f, logic and memory tables together: it is the only looker of
ctl_keccak, supplies five lookers of ctl_logic and 136 of ctl_memory, and is the looked table of ctl_keccak_sponge.

    column indices      columns.rs:15-60
    program()           the reference's eval_packed_generic for this table is a list of TODOs (keccak_sponge_stark.rs:363-377); this
                        is that list written out as one StarkAsm register program, 435 constraints in the list's order — the
                        reference's to-do list, NOT a soundness claim: nothing here ties xored_rate_u32s to the block, for example,
                        which is the logic lookup's job. gl_keccak_sponge_table_program emits the same words natively
    stark_desc()        the StarkDesc gl_stark_create / gl_stark_tables_create take
    ops_to_words()      (context, segment, virt, timestamp, bytes) -> the [num_ops][5] records and the byte buffer
    rows()              the rows the operations take
    generate_trace()    gl_keccak_sponge_table_trace: generate_trace_rows (keccak_sponge_stark.rs:190-347) built in HBM
    derive_ops()        gl_keccak_sponge_table_ops: the records the sponge makes the Keccak-f, logic and memory tables take
    ctl_*               the reference's lookup descriptions (keccak_sponge_stark.rs:26-146), word for word

Three of those descriptions cannot hold as written (all_stark.rs:93-98 leaves the sponge's lookups disabled):
  - ctl_looking_keccak() sends original_rate_u32s, but Keccak-f receives the state after the XOR: xored=True substitutes
    xored_rate_u32s;
  - ctl_logic filters logic lookup i with ctl_looking_memory_filter(i), which turns lookup i off on a final row whose remainder
    is shorter than i bytes, while generation still pushes all five XORs: ctl_looking_logic_filter() is
    is_full_input_block + is_final_block;
  - ctl_looking_memory_filter(i) sums is_final_input_len[i..], which reads byte i on a final row whose remainder is exactly i
    bytes — its first padding byte, which memory never saw: strict=True sums is_final_input_len[i + 1..]."""
import ctypes

import numpy as np

from . import _lib, table
from .device import DeviceBuffer
from .stark import CtlColumn, StarkAsm, StarkDesc

KECCAK_WIDTH_BYTES = 200
KECCAK_WIDTH_U32S = KECCAK_WIDTH_BYTES // 4
KECCAK_RATE_BYTES = 136
KECCAK_RATE_U32S = KECCAK_RATE_BYTES // 4
KECCAK_CAPACITY_BYTES = 64
KECCAK_CAPACITY_U32S = KECCAK_CAPACITY_BYTES // 4
IS_FULL_INPUT_BLOCK = 0
IS_FINAL_BLOCK = 1
CONTEXT = 2
SEGMENT = 3
VIRT = 4
TIMESTAMP = 5
LEN = 6
ALREADY_ABSORBED_BYTES = 7
IS_FINAL_INPUT_LEN = 8  # the first of 136
ORIGINAL_RATE_U32S = IS_FINAL_INPUT_LEN + KECCAK_RATE_BYTES  # the first of 34
ORIGINAL_CAPACITY_U32S = ORIGINAL_RATE_U32S + KECCAK_RATE_U32S  # the first of 16
BLOCK_BYTES = ORIGINAL_CAPACITY_U32S + KECCAK_CAPACITY_U32S  # the first of 136
XORED_RATE_U32S = BLOCK_BYTES + KECCAK_RATE_BYTES  # the first of 34
UPDATED_STATE_U32S = XORED_RATE_U32S + KECCAK_RATE_U32S  # the first of 50
NUM_COLUMNS = UPDATED_STATE_U32S + KECCAK_WIDTH_U32S
assert NUM_COLUMNS == 414 == _lib.GL_KECCAK_SPONGE_TABLE_COLUMNS
OP_WORDS = 5  # a record of gl_keccak_sponge_table_trace: context, segment, virt, timestamp, len
assert OP_WORDS == _lib.GL_KECCAK_SPONGE_TABLE_OP_WORDS
NUM_CONSTRAINTS = 3 + 136 + 1 + 51 + 51 + 5 + 50 + 1 + 1 + 136
KECCAK_INPUT_WORDS, LOGIC_OP_WORDS, MEMORY_OP_WORDS = 25, 17, 14  # the records of the three neighbouring trace calls


# ---------------------------------------------------------------- the constraints
def program():
    """(instrs [k][4] uint16, immediates): the reference's list of TODOs written out, 435 constraints in its order"""
    a = StarkAsm()

    def boolean(column):
        a.release()
        flag = a.local(column)
        one = a.imm(1)
        t = a.sub(flag, one)
        a.emit(a.mul(flag, t))

    # each flag is boolean, and so is the implied dummy flag 1 - F - L: F L = 0
    boolean(IS_FULL_INPUT_BLOCK)
    boolean(IS_FINAL_BLOCK)
    a.release()
    full = a.local(IS_FULL_INPUT_BLOCK)
    fin = a.local(IS_FINAL_BLOCK)
    a.emit(a.mul(full, fin))
    # is_final_input_len contains booleans
    for i in range(KECCAK_RATE_BYTES):
        boolean(IS_FINAL_INPUT_LEN + i)
    # their sum equals is_final_block
    a.release()
    for i in range(KECCAK_RATE_BYTES):
        t = a.local(IS_FINAL_INPUT_LEN + i)
        a.acc(t, 1)
        a.free(t)
    total = a.accr()
    fin = a.local(IS_FINAL_BLOCK)
    a.emit(a.sub(total, fin))
    # the columns that are zero where a sponge starts: the original state, then already_absorbed_bytes
    fresh = [ORIGINAL_RATE_U32S + j for j in range(KECCAK_WIDTH_U32S)] + [ALREADY_ABSORBED_BYTES]
    # the first row starts a sponge
    for column in fresh:
        a.release()
        a.emit_first_row(a.local(column))
    # behind a final block the next row starts one
    for column in fresh:
        a.release()
        fin = a.local(IS_FINAL_BLOCK)
        nxt = a.next(column)
        a.emit_transition(a.mul(fin, nxt))
    # behind a full-input block the next row's address, time and len match
    for column in (CONTEXT, SEGMENT, VIRT, TIMESTAMP, LEN):
        a.release()
        full = a.local(IS_FULL_INPUT_BLOCK)
        nxt = a.next(column)
        local = a.local(column)
        diff = a.sub(nxt, local)
        a.emit_transition(a.mul(full, diff))
    # ... its "before" is our "after"
    for j in range(KECCAK_WIDTH_U32S):
        a.release()
        full = a.local(IS_FULL_INPUT_BLOCK)
        nxt = a.next(ORIGINAL_RATE_U32S + j)
        updated = a.local(UPDATED_STATE_U32S + j)
        diff = a.sub(nxt, updated)
        a.emit_transition(a.mul(full, diff))
    # ... and its already_absorbed_bytes is ours plus 136
    a.release()
    full = a.local(IS_FULL_INPUT_BLOCK)
    nxt = a.next(ALREADY_ABSORBED_BYTES)
    local = a.local(ALREADY_ABSORBED_BYTES)
    diff = a.sub(nxt, local)
    rate = a.imm(KECCAK_RATE_BYTES)
    a.sub(diff, rate, dst=diff)
    a.emit_transition(a.mul(full, diff))
    # a dummy row is followed by a dummy row
    a.release()
    dummy = a.imm(1)
    full = a.local(IS_FULL_INPUT_BLOCK)
    a.sub(dummy, full, dst=dummy)
    fin = a.local(IS_FINAL_BLOCK)
    a.sub(dummy, fin, dst=dummy)
    next_full = a.next(IS_FULL_INPUT_BLOCK)
    next_fin = a.next(IS_FINAL_BLOCK)
    next_used = a.add(next_full, next_fin)
    a.emit_transition(a.mul(dummy, next_used))
    # is_final_input_len[i] implies len - already_absorbed_bytes == i
    for i in range(KECCAK_RATE_BYTES):
        a.release()
        flag = a.local(IS_FINAL_INPUT_LEN + i)
        length = a.local(LEN)
        absorbed = a.local(ALREADY_ABSORBED_BYTES)
        diff = a.sub(length, absorbed)
        index = a.imm(i)
        a.sub(diff, index, dst=diff)
        a.emit(a.mul(flag, diff))
    return a.program()


def stark_desc(degree_bits, num_challenges, fri_params):
    """KeccakSpongeStark as a StarkDesc: constraint_degree 3, no public inputs, no permutation pairs"""
    instrs, immediates = program()
    return StarkDesc(degree_bits, NUM_COLUMNS, 0, 3, num_challenges, fri_params, instrs, immediates)


def native_program():
    """gl_keccak_sponge_table_program: (instrs, immediates, number of constraints) as the library emits them — program() word for
    word"""
    return table.native_program("gl_keccak_sponge_table_program")

# ---------------------------------------------------------------- the lookups (keccak_sponge_stark.rs:26-146)
def ctl_looked_data():
    """:26-38, what the CPU table looks up: context, segment, virt, len, timestamp, then the first eight limbs of the output"""
    return [CtlColumn.single(c) for c in (CONTEXT, SEGMENT, VIRT, LEN, TIMESTAMP)] + [CtlColumn.single(UPDATED_STATE_U32S + i) for i in range(8)]


def ctl_looked_filter():
    """:128-132: the final-block rows carry the sponge's output"""
    return CtlColumn.single(IS_FINAL_BLOCK)


def ctl_looking_keccak(xored=False):
    """:40-51 with xored=False, the reference's words: original_rate_u32s, original_capacity_u32s, updated_state_u32s. AS WRITTEN IT
    CANNOT HOLD on a row that absorbs anything: Keccak-f receives the state after the XOR (witness/util.rs:218,243).
    xored=True sends xored_rate_u32s in place of original_rate_u32s, which is what generation feeds the Keccak-f table."""
    rate = XORED_RATE_U32S if xored else ORIGINAL_RATE_U32S
    cols = [rate + j for j in range(KECCAK_RATE_U32S)] + [ORIGINAL_CAPACITY_U32S + j for j in range(KECCAK_CAPACITY_U32S)]
    return [CtlColumn.single(c) for c in cols + [UPDATED_STATE_U32S + j for j in range(KECCAK_WIDTH_U32S)]]


def ctl_looking_keccak_filter():
    """:143-146"""
    return CtlColumn.sum([IS_FULL_INPUT_BLOCK, IS_FINAL_BLOCK])


def ctl_looking_memory(i):
    """:53-79: is_read = 1, context, segment, virt + already_absorbed_bytes + i, block_bytes[i], seven zero limbs, timestamp"""
    res = [CtlColumn.constant(1), CtlColumn.single(CONTEXT), CtlColumn.single(SEGMENT)]
    res.append(CtlColumn.linear_combination([(VIRT, 1), (ALREADY_ABSORBED_BYTES, 1)], i))
    res.append(CtlColumn.single(BLOCK_BYTES + i))
    res += [CtlColumn.constant(0) for _ in range(7)]
    res.append(CtlColumn.single(TIMESTAMP))
    return res


def ctl_looking_memory_filter(i, strict=False):
    """:134-141 with strict=False, the reference's words: is_full_input_block + sum of is_final_input_len[i..]. AS WRITTEN IT CANNOT
    HOLD on a final row: the sum includes a remainder of exactly i bytes, whose byte i is the first padding byte, which no memory
    operation reads (the comment there says "of length i or greater"; byte i is an input byte from length i + 1 on).
    strict=True sums is_final_input_len[i + 1..]: byte i is looked up where generation pushed its read."""
    return CtlColumn.sum([IS_FULL_INPUT_BLOCK] + [IS_FINAL_INPUT_LEN + k for k in range(i + 1 if strict else i, KECCAK_RATE_BYTES)])


def num_logic_ctls():
    """:81-84"""
    return -(-KECCAK_RATE_BYTES // 32)


def ctl_looking_logic(i):
    """:88-126: is_and = 0, is_or = 0, is_xor = 1; eight limbs of original_rate_u32s from 8 i on, the little-endian u32s of
    block_bytes from 32 i on, eight limbs of xored_rate_u32s from 8 i on; the last lookup carries two limbs and six zeros"""
    assert 0 <= i < num_logic_ctls()
    zero = lambda: CtlColumn.constant(0)  # noqa: E731
    res = [zero(), zero(), CtlColumn.constant(1)]
    limbs = range(8 * i, min(8 * i + 8, KECCAK_RATE_U32S))
    pad = [zero() for _ in range(8 - len(limbs))]
    res += [CtlColumn.single(ORIGINAL_RATE_U32S + k) for k in limbs] + [zero() for _ in pad]
    res += [CtlColumn([(BLOCK_BYTES + 4 * k + j, 1 << (8 * j)) for j in range(4)]) for k in limbs] + [zero() for _ in pad]
    res += [CtlColumn.single(XORED_RATE_U32S + k) for k in limbs] + [zero() for _ in pad]
    return res


def ctl_looking_logic_filter():
    """is_full_input_block + is_final_block: every row that absorbs a block pushes all five XORs (xor_into_sponge,
    witness/util.rs:178-194). The REFERENCE's choice for logic lookup i is ctl_looking_memory_filter(i) (all_stark.rs, ctl_logic),
    which switches lookup i off on a final row whose remainder is shorter than i bytes although its XOR was pushed; pass that
    where the reference's own words are wanted."""
    return CtlColumn.sum([IS_FULL_INPUT_BLOCK, IS_FINAL_BLOCK])


# ---------------------------------------------------------------- the trace
def ops_to_words(ops):
    """`ops`: an iterable of (context, segment, virt, timestamp, data) with `data` bytes-like ->
    ([num_ops][5] uint64 records, the inputs concatenated as a uint8 array)"""
    words, chunks = [], []
    for context, segment, virt, timestamp, data in ops:
        data = bytes(data)
        words.append([int(context), int(segment), int(virt), int(timestamp), len(data)])
        chunks.append(data)
    return np.array(words, dtype=np.uint64).reshape(-1, OP_WORDS), np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()


def upload_bytes(ctx, data, offset=0):
    """`data` (uint8 array) in HBM, starting `offset` bytes into an 8-byte aligned buffer: (DeviceBuffer, device address of byte 0)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    padded = np.zeros((offset + data.size + 7) // 8 * 8 or 8, dtype=np.uint8)
    padded[offset : offset + data.size] = data
    buf = DeviceBuffer.from_host(ctx, padded.view(np.uint64))
    return buf, buf.ptr + offset


def _device_ops(ctx, ops, data):
    """(records DeviceBuffer or None, num_ops, bytes DeviceBuffer or None, address of the first byte or None)"""
    d_ops, num_ops = table.device_records(ctx, ops, OP_WORDS)
    if data is None or isinstance(data, int):
        return d_ops, num_ops, None, data
    if isinstance(data, DeviceBuffer):
        return d_ops, num_ops, data, data.ptr
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if not data.size:
        return d_ops, num_ops, None, None
    buf, ptr = upload_bytes(ctx, data)
    return d_ops, num_ops, buf, ptr


def _scratch(ctx, num_ops, degree_bits):
    return table.scratch(ctx, "gl_keccak_sponge_table_scratch_bytes", num_ops, degree_bits,
                         "gl_keccak_sponge_table_scratch_bytes: num_ops must be at most 2^30 and degree_bits in 1 ..= 23")


def _count(ctx, d_ops, num_ops):
    count = ctypes.c_uint64()
    scratch = _scratch(ctx, num_ops, 1)
    _lib.call("gl_keccak_sponge_table_trace", table.ptr(d_ops), num_ops, None, 1, None, 0, scratch.ptr, ctypes.byref(count), ctx.ptr)
    return int(count.value)


def rows(ctx, ops):
    """the rows the operations take: sum of len / 136 + 1. `ops`: host [num_ops][5] words or a DeviceBuffer of them; the bytes are
    not read for the count."""
    d_ops, num_ops, _, _ = _device_ops(ctx, ops, None)
    return _count(ctx, d_ops, num_ops)  # the call has waited for the stream: an upload of this call may go


def generate_trace(ctx, ops, data=None, degree_bits=None, trace_stride=None):
    """gl_keccak_sponge_table_trace: the trace of the operations `ops` ([num_ops][5] words, host array or DeviceBuffer; or the
    iterable ops_to_words takes, with data=None) over the concatenated input bytes `data` (uint8 host array, a DeviceBuffer that
    starts with them, or a device address) with 2^degree_bits rows as a DeviceBuffer [414][trace_stride] (default 2^degree_bits),
    built on the context's stream. degree_bits=None asks for the count first and takes the smallest trace that holds it. The rows
    the operations take are left in the buffer's attribute `rows`."""
    if data is None and not isinstance(ops, (DeviceBuffer, np.ndarray)):
        ops, data = ops_to_words(ops)
    d_ops, num_ops, d_bytes, bytes_ptr = _device_ops(ctx, ops, data)  # d_bytes: an upload of this call lives until the return
    if degree_bits is None:
        degree_bits = max(1, (max(_count(ctx, d_ops, num_ops), 1) - 1).bit_length())
    # synchronised: the scratch and the uploads of this call are released on return
    return table.generate_trace(ctx, "gl_keccak_sponge_table_trace", [table.ptr(d_ops), num_ops, bytes_ptr], degree_bits, trace_stride,
                                NUM_COLUMNS, scratch=_scratch(ctx, num_ops, degree_bits), counted=True)


def derive_ops(ctx, d_trace, degree_bits, rows, num_bytes=None, trace_stride=None, keccak=True, logic=True, memory=True):
    """gl_keccak_sponge_table_ops: from rows 0 .. rows of the finished trace `d_trace` the records the sponge makes the other
    tables take, as DeviceBuffers (None where not asked for): (keccak_inputs [rows][25], logic_ops [5 rows][17], memory_ops
    [num_bytes][14]). `num_bytes`: the sum of the operations' lengths; None reads is_final_block and len back from the trace."""
    n = 1 << degree_bits
    stride = n if trace_stride is None else int(trace_stride)
    if memory and num_bytes is None:
        final = d_trace.download(IS_FINAL_BLOCK * stride, rows)
        num_bytes = int(d_trace.download(LEN * stride, rows)[final == 1].sum())
    d_keccak = DeviceBuffer(ctx, max(rows * KECCAK_INPUT_WORDS, 1)) if keccak else None
    d_logic = DeviceBuffer(ctx, max(rows * num_logic_ctls() * LOGIC_OP_WORDS, 1)) if logic else None
    d_memory = DeviceBuffer(ctx, max(num_bytes * MEMORY_OP_WORDS, 1)) if memory else None
    scratch = _scratch(ctx, 0, degree_bits)
    _lib.call("gl_keccak_sponge_table_ops", d_trace.ptr, stride, degree_bits, rows, d_keccak.ptr if keccak else None, d_logic.ptr if logic else None,
              d_memory.ptr if memory else None, scratch.ptr, ctx.ptr)
    ctx.synchronize()  # the scratch is released here
    for buf, count in ((d_keccak, rows * KECCAK_INPUT_WORDS), (d_logic, rows * num_logic_ctls() * LOGIC_OP_WORDS), (d_memory, (num_bytes or 0) * MEMORY_OP_WORDS)):
        if buf is not None:
            buf.n = count  # the records, without the word that keeps an empty buffer allocatable
    return d_keccak, d_logic, d_memory
