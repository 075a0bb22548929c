"""The lookup columns of a STARK trace on the device (gl_sort_canonical / gl_lookup_permuted_cols / gl_stark_fill_lookups,
csrc/lookup.hip): the Halo2-style lookup argument of the reference's STARKs (evm/src/lookup.rs).

A lookup is four trace columns (input, table, permuted input, permuted table). The device fills the last two with
`permuted_cols(input, table)` (lookup.rs:67-131), bit for bit; `StarkAsm.eval_lookups` emits their constraints and `lookup_pairs`
gives the permutation pairs that tie them to the first two (memory_stark.rs:452-456). Everything is queued on the context's stream:
a prove() of the same context that follows sees the filled columns, and nothing waits for the device here."""
import numpy as np

from . import _lib
from .device import DeviceBuffer

MAX_N = 1 << 30


def scratch_words(n):
    """gl_lookup_scratch_bytes(n) in 64-bit words: the size of the scratch DeviceBuffer of the calls below"""
    if not 1 <= int(n) <= MAX_N:
        raise ValueError("n must be in 1 ..= 2^30")
    return _lib.load().gl_lookup_scratch_bytes(int(n)) // 8


def _scratch(ctx, n, scratch):
    return scratch if scratch is not None else DeviceBuffer(ctx, scratch_words(n))


def _ptr(b):
    return b.ptr if isinstance(b, DeviceBuffer) else b


def sort_canonical(ctx, buf, n, out=None, scratch=None):
    """The canonical values of buf[0..n) in ascending order -> `out` (default: in place). Returns `out`."""
    out = buf if out is None else out
    s = _scratch(ctx, n, scratch)
    _lib.call("gl_sort_canonical", _ptr(buf), _ptr(out), int(n), _ptr(s), ctx.ptr)
    if scratch is None:
        ctx.synchronize()  # the scratch buffer of this call is freed on return
    return out


def permuted_cols(ctx, inputs, table, n, permuted_inputs=None, permuted_table=None, scratch=None):
    """permuted_cols(inputs, table) over DeviceBuffers (or device pointers): (permuted_inputs, permuted_table), allocated here
    unless given."""
    pi = permuted_inputs if permuted_inputs is not None else DeviceBuffer(ctx, n)
    pt = permuted_table if permuted_table is not None else DeviceBuffer(ctx, n)
    s = _scratch(ctx, n, scratch)
    _lib.call("gl_lookup_permuted_cols", _ptr(inputs), _ptr(table), int(n), _ptr(pi), _ptr(pt), _ptr(s), ctx.ptr)
    if scratch is None:
        ctx.synchronize()
    return pi, pt


def fill_lookups(ctx, trace_buf, n, num_columns, lookups, trace_stride=None, scratch=None):
    """`trace_buf`: [num_columns][pitch trace_stride, default n] value columns; `lookups`: (input, table, permuted input, permuted
    table) column numbers. Writes the two permuted columns of every lookup and nothing else."""
    flat = np.ascontiguousarray([c for lk in lookups for c in lk], dtype=np.uint32)
    if flat.size != 4 * len(lookups):
        raise ValueError("a lookup is four columns: input, table, permuted input, permuted table")
    s = _scratch(ctx, n, scratch)
    _lib.call("gl_stark_fill_lookups", _ptr(trace_buf), int(trace_stride if trace_stride is not None else n), int(n), int(num_columns),
              flat if flat.size else None, len(lookups), _ptr(s), ctx.ptr)
    if scratch is None:
        ctx.synchronize()


def lookup_pairs(lookups):
    """The permutation pairs of the lookups (memory_stark.rs:452-456): per lookup PermutationPair::singletons(input, permuted input)
    and singletons(table, permuted table), in the form of StarkDesc.pairs."""
    pairs = []
    for col_in, col_table, col_perm_in, col_perm_table in lookups:
        pairs.append([(int(col_in), int(col_perm_in))])
        pairs.append([(int(col_table), int(col_perm_table))])
    return pairs
