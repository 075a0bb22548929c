"""What the table modules (keccak_table, memory_table, logic_table, keccak_sponge_table) share around the library's calls: a
GlGatePrograms result unpacked once, a record list brought to the device, the scratch a call asks for, and the tail of every
generate_trace. What a table is — columns, program(), lookups, its own refusals' words — stays in its module."""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceBuffer


def call_programs(symbol, *args):
    """`symbol(*args, &GlGatePrograms)`, unpacked and freed: (instrs [k][4] uint16, gates [g][6] uint32 or None where the result
    has no gate descriptors, immediates as a list of ints, num_gate_constraints)"""
    out = _lib.GlGatePrograms()
    _lib.call(symbol, *args, ctypes.byref(out))
    try:
        instrs = np.ctypeslib.as_array(ctypes.cast(out.instrs, ctypes.POINTER(ctypes.c_uint16)), shape=(out.num_instrs, 4)).copy()
        gates = None
        if out.gates or out.num_gates:
            gates = np.ctypeslib.as_array(ctypes.cast(out.gates, ctypes.POINTER(ctypes.c_uint32)), shape=(out.num_gates, 6)).copy()
        imms = []
        if out.num_immediates:
            imms = [int(v) for v in np.ctypeslib.as_array(ctypes.cast(out.immediates, ctypes.POINTER(ctypes.c_uint64)), shape=(out.num_immediates,))]
        return instrs, gates, imms, int(out.num_gate_constraints)
    finally:
        _lib.load().gl_gate_programs_free(ctypes.byref(out))


def native_program(symbol):
    """a table's gl_*_table_program: (instrs, immediates, number of constraints) as the library emits them"""
    instrs, gates, imms, num_constraints = call_programs(symbol)
    if gates is not None:
        raise RuntimeError("%s: a STARK program has no gate descriptors" % symbol)
    return instrs, imms, num_constraints


def device_records(ctx, ops, op_words, min_ops=0, too_few=None):
    """`ops` ([num_ops][op_words] words, host array or DeviceBuffer) on the device: (DeviceBuffer, or None for an empty host list;
    num_ops). A host list shorter than `min_ops` is a ValueError(`too_few`) before anything is uploaded. A buffer this call
    uploaded is the caller's to keep alive until the stream has read it."""
    if isinstance(ops, DeviceBuffer):
        return ops, ops.n // op_words
    host = np.ascontiguousarray(np.asarray(ops, dtype=np.uint64).reshape(-1, op_words))
    num_ops = host.shape[0]
    if num_ops < min_ops:
        raise ValueError(too_few)
    return (DeviceBuffer.from_host(ctx, host) if num_ops else None), num_ops


def ptr(buf):
    return buf.ptr if buf is not None else None


def scratch(ctx, symbol, num_ops, degree_bits, refusal):
    """a DeviceBuffer of the bytes `symbol(num_ops, degree_bits)` names; 0 bytes is the library's refusal: ValueError(`refusal`)"""
    size = getattr(_lib.load(), symbol)(num_ops, degree_bits)
    if not size:
        raise ValueError(refusal)
    return DeviceBuffer(ctx, size // 8)


def generate_trace(ctx, symbol, head, degree_bits, trace_stride, columns, scratch=None, counted=False, synchronize=True):
    """The tail of a table's generate_trace: allocates [columns][trace_stride] (default 2^degree_bits) and calls
    `symbol(*head, degree_bits, d_trace, stride, [scratch], [&rows], ctx)` on the context's stream. `counted`: the call reports the
    rows it needed, left in the buffer's attribute `rows`. `synchronize`: wait for the stream, where buffers of this call (the
    scratch, an upload) are released when the caller returns: the kernels must have finished with them."""
    stride = (1 << degree_bits) if trace_stride is None else int(trace_stride)
    d_trace = DeviceBuffer(ctx, columns * max(stride, 1))
    tail = [] if scratch is None else [scratch.ptr]
    rows = ctypes.c_uint64()
    if counted:
        tail.append(ctypes.byref(rows))
    _lib.call(symbol, *head, degree_bits, d_trace.ptr, stride, *tail, ctx.ptr)
    if synchronize:
        ctx.synchronize()
    if counted:
        d_trace.rows = int(rows.value)
    return d_trace
