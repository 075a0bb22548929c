"""The steps of csrc/lookup.hip's permuted_cols in plain Python (TEST INFRASTRUCTURE): the decomposition of DESIGN.md §3.7.2, array by
array as the kernels compute them — flags and their packed exclusive scan, events ordered by value, the (sum, min) scan, levels, the
stable sort by level, the assignment and the deferred positions — so that the restatement of the serial loop (tests/lookup_ref.py)
can be held against the decomposition without a device. Sorting itself is Python's."""
from bisect import bisect_left as lb
from bisect import bisect_right as ub

import lookup_ref as lr

POP = 0x80000000


def lo(x):
    return x & 0xFFFFFFFF


def hi(x):
    return x >> 32


def permuted_cols_by_events(inputs, table):
    """(permuted_inputs, permuted_table); the assertions are the invariants the kernels rely on"""
    n = len(inputs)
    S = lr.sort_canonical(inputs)
    T = lr.sort_canonical(table)
    PT = [None] * n
    tl = T[n - 1]
    post_start = lb(S, tl) + min(ub(S, tl) - lb(S, tl), ub(T, tl) - lb(T, tl))
    F = [0] * (n + 1)
    for i in range(n):
        v = S[i]
        f = 0
        if i - lb(S, v) < ub(T, v) - lb(T, v):
            PT[i] = v
        elif v < tl:
            f |= 1
        else:
            assert i >= post_start
        v = T[i]
        if i - lb(T, v) >= ub(S, v) - lb(S, v):
            f |= 1 << 32
        F[i] = f
    for i in range(post_start, n):
        assert PT[i] is None
    E = [0] * (n + 1)
    a = 0
    for i in range(n + 1):
        E[i] = a
        a += F[i]
    ne = lo(E[n]) + hi(E[n])
    ev = [0] * (2 * n)
    X = [(0, 0)] * (2 * n)
    for i in range(n):
        f = E[i + 1] - E[i]
        if f & 1:
            k = lo(E[i]) + hi(E[lb(T, S[i])])
            ev[k] = i | POP
            X[k] = (-1, -1)
        if f >> 32:
            k = hi(E[i]) + lo(E[lb(S, T[i])])
            ev[k] = i
            X[k] = (1, 0)
    PM = []
    acc = (0, 0)
    for k in range(2 * n):
        acc = (acc[0] + X[k][0], min(acc[1], acc[0] + X[k][1]))
        PM.append(acc)
    keys = [0] * (2 * n)
    defpos = [None] * n
    for k in range(2 * n):
        keys[k] = k
        if k >= ne:
            continue
        p, m = PM[k]
        mp = PM[k - 1][1] if k else 0
        e = ev[k]
        if e & POP:
            if m < mp:
                defpos[-m - 1] = e & (POP - 1)
                continue
            level = p - m + 1
        else:
            level = p - m
        assert level >= 1
        keys[k] = level << 32 | k
    numdef = -PM[ne - 1][1] if ne else 0
    keys.sort(key=lambda x: x >> 32)  # stable
    stack = [None] * n
    for q in range(2 * n):
        key = keys[q]
        level = key >> 32
        if level == 0:
            continue
        e = ev[key & 0xFFFFFFFF]
        if e & POP:
            prev = keys[q - 1]
            assert prev >> 32 == level
            ep = ev[prev & 0xFFFFFFFF]
            assert not ep & POP
            PT[e & (POP - 1)] = T[ep]
        else:
            taken = q + 1 < 2 * n and keys[q + 1] >> 32 == level
            if not taken:
                assert stack[level - 1] is None
                stack[level - 1] = T[e]
    numpost = n - post_start
    for r in range(n):
        if r < numdef:
            pos = defpos[r]
        elif r < numdef + numpost:
            pos = post_start + r - numdef
        else:
            assert stack[r] is None
            continue
        assert PT[pos] is None
        PT[pos] = stack[r]
    return S, PT
