"""Operation lists for the memory table's tests (TEST INFRASTRUCTURE): [num_ops][14] uint64 records, MemoryOp::into_row()[0..14],
in an order that is NOT sorted unless the family says so. Every family stays inside what the reference itself accepts (its
assert on context and segment gaps) and keeps the number of rows small enough for the serial model of tests/memory_table_ref.py."""
import numpy as np

import memory_table_ref as mr

M32 = (1 << 32) - 1


def words(filter_, timestamp, is_read, context, segment, virt, values):
    n = len(timestamp)
    out = np.zeros((n, mr.OP_WORDS), dtype=np.uint64)
    for c, col in ((mr.FILTER, filter_), (mr.TIMESTAMP, timestamp), (mr.IS_READ, is_read), (mr.ADDR_CONTEXT, context),
                   (mr.ADDR_SEGMENT, segment), (mr.ADDR_VIRTUAL, virt)):
        out[:, c] = np.asarray(col, dtype=np.uint64)
    out[:, mr.VALUE_START:] = np.asarray(values, dtype=np.uint64).reshape(n, 8)
    return out


def _values(rng, n):
    return rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64)


def small_keys(num_ops, seed=1):
    """2 contexts x 3 segments x 4 addresses x 4 timestamps: from 100 operations on most keys occur several times, with differing
    values, filters and kinds — only a stable sort puts them in list order"""
    rng = np.random.default_rng([seed, num_ops])
    return words(rng.integers(0, 2, num_ops), rng.integers(0, 4, num_ops), rng.integers(0, 2, num_ops), rng.integers(0, 2, num_ops),
                 rng.integers(0, 3, num_ops), rng.integers(0, 4, num_ops), _values(rng, num_ops))


def mixed(num_ops, seed=2):
    """a few contexts and segments, addresses and timestamps spread over about 6 max_rc: dummies of both kinds in many pairs"""
    rng = np.random.default_rng([seed, num_ops])
    span = 6 * mr.next_power_of_two(num_ops)
    addresses = max(1, num_ops // 3)  # about three operations per address: timestamp gaps too
    virt = rng.integers(0, span, addresses)[rng.integers(0, addresses, num_ops)]
    return words(rng.integers(0, 2, num_ops), rng.integers(0, span, num_ops), rng.integers(0, 2, num_ops), rng.integers(0, 3, num_ops),
                 rng.integers(0, 2, num_ops), virt, _values(rng, num_ops))


def in_order(num_ops, reverse=False):
    """`mixed` already sorted by its key, or in the reverse order (equal keys then stand in reversed list order: the tie-break shows)"""
    w = mixed(num_ops, seed=3)
    order = sorted(range(num_ops), key=lambda i: tuple(int(w[i, c]) for c in (mr.ADDR_CONTEXT, mr.ADDR_SEGMENT, mr.ADDR_VIRTUAL, mr.TIMESTAMP)))
    return np.ascontiguousarray(w[order[::-1] if reverse else order])


def one_address(num_ops, seed=4):
    """one address, timestamps rising in list order by 1 .. 3 max_rc"""
    rng = np.random.default_rng([seed, num_ops])
    ts = np.cumsum(rng.integers(1, 3 * mr.next_power_of_two(num_ops), num_ops))
    return words(np.ones(num_ops), ts, rng.integers(0, 2, num_ops), np.full(num_ops, 7), np.full(num_ops, 2), np.full(num_ops, 1000), _values(rng, num_ops))


def at_the_top(num_ops, seed=5):
    """context and segment 2^32 - 1, addresses and timestamps in the last few values below 2^32, limbs of 2^32 - 1"""
    rng = np.random.default_rng([seed, num_ops])
    span = 3 * mr.next_power_of_two(num_ops)
    values = _values(rng, num_ops)
    values[::2] = M32
    return words(rng.integers(0, 2, num_ops), M32 - rng.integers(0, span, num_ops), rng.integers(0, 2, num_ops), np.full(num_ops, M32),
                 np.full(num_ops, M32), M32 - rng.integers(0, span, num_ops), values)


def wide(num_ops, seed=6):
    """every radix pass of every field: 300 contexts `num_ops` apart (a gap of num_ops - 1 is the largest the reference accepts in a
    trace of num_ops rows), in context 0 300 segments as far apart, in (0, 0) distinct addresses below 64 max_rc (64 dummies or
    so), elsewhere distinct small ones; timestamps uniform below 2^32 — no address occurs twice, so none of them asks for a dummy"""
    rng = np.random.default_rng([seed, num_ops])
    group = rng.integers(0, 600, num_ops)
    context = np.where(group < 300, 0, (group - 299) * num_ops)
    segment = np.where(group < 300, group * num_ops, 0)
    virt = np.zeros(num_ops, dtype=np.uint64)
    for g in range(600):
        idx = np.flatnonzero(group == g)
        span = 64 * mr.next_power_of_two(num_ops) if g == 0 else 1 << 12
        virt[idx] = rng.choice(span, size=len(idx), replace=False)
    return words(rng.integers(0, 2, num_ops), rng.integers(0, 1 << 32, num_ops), rng.integers(0, 2, num_ops), context, segment, virt, _values(rng, num_ops))


def one_long_gap():
    """4 operations, a virtual gap of 12 000 under max_rc = 3: 2999 dummies in one pair, more than a scan block of 2048 holds"""
    return words([1, 1, 0, 1], [5, 9, 2, 7], [0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0], [12000, 0, 0, 12000], [[k + 1] * 8 for k in range(4)])


def no_gap(num_ops, seed=7):
    """addresses 0 .. num_ops / 2 all used, timestamps a permutation of 0 .. num_ops: no dummy anywhere"""
    rng = np.random.default_rng([seed, num_ops])
    virt = np.concatenate([np.arange((num_ops + 1) // 2), np.arange(num_ops // 2)])
    w = words(rng.integers(0, 2, num_ops), np.arange(num_ops), rng.integers(0, 2, num_ops), np.zeros(num_ops), np.zeros(num_ops), virt, _values(rng, num_ops))
    return np.ascontiguousarray(w[rng.permutation(num_ops)])


def gaps_in_the_first_half(num_ops, seed=8):
    """`mixed` in contexts 0 .. 2 and `no_gap` in context 3, shuffled together: the last pair with a gap lies in the middle of the
    sorted list, and so does the padding"""
    rng = np.random.default_rng([seed, num_ops])
    a, b = mixed(num_ops // 2, seed), no_gap(num_ops - num_ops // 2, seed)
    b[:, mr.ADDR_CONTEXT] = 3
    return np.ascontiguousarray(np.concatenate([a, b])[rng.permutation(num_ops)])


def provable(seed=0, extra=0):
    """A list whose trace satisfies the reference's constraints, with dummies of both kinds and the padding rows in the middle.
    What makes a trace violate them: a timestamp-gap dummy (a read of 0) at an address that holds something else; a read that
    does not see the write before it; a first row that is a read of another value than the last row's. Here: every address
    starts with a write or holds 0, reads repeat the value before them, timestamp gaps only where the value is 0, and the
    smallest key is a write. 10 + extra operations, max_rc 15 (extra <= 6): 6 virtual-address dummies between 0 and 100, 2
    timestamp dummies at address 100 — the LAST pair with a gap, so the padding stands behind timestamp 33 — and operations in
    segment 1 and context 1 behind it. In list order after a shuffle by `seed`."""
    rng = np.random.default_rng([11, seed])
    v = [[int(x) for x in rng.integers(1, 1 << 32, 8)] for _ in range(4)]
    zero = [0] * 8
    ops = [  # filter, timestamp, is_read, context, segment, virt, value
        (1, 1, 0, 0, 0, 0, v[0]), (1, 2, 1, 0, 0, 0, v[0]), (1, 4, 1, 0, 0, 0, v[0]),
        (1, 3, 1, 0, 0, 100, zero), (1, 43, 1, 0, 0, 100, zero), (1, 50, 0, 0, 0, 100, v[1]),
        (1, 6, 0, 0, 1, 5, v[2]), (1, 8, 1, 0, 1, 5, v[2]),
        (1, 10, 0, 1, 0, 7, v[3]), (1, 12, 1, 1, 0, 7, v[3]),
    ]
    for k in range(extra):  # further reads of the last write, in context 1
        ops.append((1, 13 + k, 1, 1, 0, 7, v[3]))
    ops = [ops[i] for i in rng.permutation(len(ops))]
    return words(*[[op[c] for op in ops] for c in range(7)])
