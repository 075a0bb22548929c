"""The one-sort construction of csrc/memory_table.hip on the host (TEST INFRASTRUCTURE): the kernels' arithmetic restated step by
step — four stable rounds over `field << 32 | position`, the per-pair dummy counts, their exclusive prefix sums, the place of the
padding rows, and one binary search per row of the trace — so that the decomposition DESIGN.md §3.7.5 derives can be held against
the literal model of tests/memory_table_ref.py without a GPU. The lookup columns are not part of it."""
import numpy as np

import memory_table_ref as mr

M32 = (1 << 32) - 1


def sorted_positions(words):
    """the rounds of lookup_sort_by_upper_half: timestamp first, context last, each stable in the order the round before left"""
    order = list(range(len(words)))
    for field in (mr.TIMESTAMP, mr.ADDR_VIRTUAL, mr.ADDR_SEGMENT, mr.ADDR_CONTEXT):
        keys = [(int(words[i][field]) & M32) << 32 | i for i in order]
        keys.sort(key=lambda k: k >> 32)  # stable, by the upper half alone
        order = [k & M32 for k in keys]
    return order


def pair_counts(words, order):
    num_ops = len(order)
    log_step = (num_ops - 1).bit_length()
    max_rc = (1 << log_step) - 1
    counts, last_pair, largest_gap = [0] * (num_ops + 1), 0, 0
    for j in range(num_ops - 1):
        a, b = [int(x) for x in words[order[j]]], [int(x) for x in words[order[j + 1]]]
        if a[mr.ADDR_CONTEXT] != b[mr.ADDR_CONTEXT]:
            largest_gap = max(largest_gap, b[mr.ADDR_CONTEXT] - a[mr.ADDR_CONTEXT] - 1)
        elif a[mr.ADDR_SEGMENT] != b[mr.ADDR_SEGMENT]:
            largest_gap = max(largest_gap, b[mr.ADDR_SEGMENT] - a[mr.ADDR_SEGMENT] - 1)
        elif a[mr.ADDR_VIRTUAL] != b[mr.ADDR_VIRTUAL]:
            counts[j] = (b[mr.ADDR_VIRTUAL] - a[mr.ADDR_VIRTUAL] - 1) >> log_step
        else:
            dts = b[mr.TIMESTAMP] - a[mr.TIMESTAMP]
            counts[j] = (dts - 1) // max_rc if dts else 0
        if counts[j]:
            last_pair = j + 1
    return counts, last_pair, largest_gap, log_step


def rows_needed(words):
    order = sorted_positions(words)
    return len(order) + sum(pair_counts(words, order)[0])


def trace_rows(words, degree_bits):
    """[n][14] rows as mt_rows writes them, then the flags as mt_flags does: [26][n] with the lookup columns left at zero"""
    order = sorted_positions(words)
    num_ops, n = len(order), 1 << degree_bits
    counts, last_pair, largest_gap, log_step = pair_counts(words, order)
    max_rc = (1 << log_step) - 1
    sums = [0] * (num_ops + 1)
    for j in range(num_ops):
        sums[j + 1] = sums[j] + counts[j]
    rows = num_ops + sums[num_ops]
    assert rows <= n and largest_gap < n
    padding = n - rows
    pad_start = last_pair + sums[last_pair] if last_pair else rows
    cols = np.zeros((mr.NUM_COLUMNS, n), dtype=np.uint64)
    for r in range(n):
        is_padding = pad_start <= r < pad_start + padding
        q = pad_start - 1 if is_padding else (r if r < pad_start else r - padding)
        lo, hi = 0, num_ops - 1
        while lo < hi:
            mid = lo + (hi - lo + 1) // 2
            if mid + sums[mid] <= q:
                lo = mid
            else:
                hi = mid - 1
        k = q - (lo + sums[lo])
        w = [int(x) for x in words[order[lo]]]
        if k:
            assert k <= counts[lo]
            if int(words[order[lo + 1]][mr.ADDR_VIRTUAL]) != w[mr.ADDR_VIRTUAL]:
                w[mr.ADDR_VIRTUAL] += k << log_step
                w[mr.TIMESTAMP] = 0
            else:
                w[mr.TIMESTAMP] += k * max_rc
            w[mr.VALUE_START:] = [0] * 8
        if k or is_padding:
            w[mr.FILTER], w[mr.IS_READ] = 0, 1
        cols[: mr.OP_WORDS, r] = w
        cols[mr.COUNTER, r] = r
    for r in range(n - 1):
        c, s, v, t = (int(cols[x, r]) for x in (mr.ADDR_CONTEXT, mr.ADDR_SEGMENT, mr.ADDR_VIRTUAL, mr.TIMESTAMP))
        nc, ns, nv, nt = (int(cols[x, r + 1]) for x in (mr.ADDR_CONTEXT, mr.ADDR_SEGMENT, mr.ADDR_VIRTUAL, mr.TIMESTAMP))
        cfc = c != nc
        sfc = s != ns and not cfc
        vfc = v != nv and not sfc and not cfc
        cols[mr.CONTEXT_FIRST_CHANGE, r], cols[mr.SEGMENT_FIRST_CHANGE, r], cols[mr.VIRTUAL_FIRST_CHANGE, r] = int(cfc), int(sfc), int(vfc)
        cols[mr.RANGE_CHECK, r] = nc - c - 1 if cfc else ns - s - 1 if sfc else nv - v - 1 if vfc else nt - t
    return cols
