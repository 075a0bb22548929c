"""The Halo2-style lookup argument of the reference's STARKs on the host (TEST INFRASTRUCTURE): a literal, serial restatement of
`permuted_cols` (evm/src/lookup.rs:67-131) written from the Rust, line by line, and a checker of the argument itself. Nothing here
knows how the device computes the columns."""

P = 0xFFFFFFFF00000001


def canonical(x):
    """to_canonical of any u64 representative: p is 0, 2^64 - 1 is 2^32 - 2"""
    x = int(x)
    assert 0 <= x < 1 << 64
    return x - P if x >= P else x


def sort_canonical(values):
    return sorted(canonical(x) for x in values)


def permuted_cols(inputs, table):
    """(permuted_inputs, permuted_table) as lists of canonical ints"""
    n = len(inputs)
    assert len(table) == n
    sorted_inputs = sorted(canonical(x) for x in inputs)  # lookup.rs:79-83
    sorted_table = sorted(canonical(x) for x in table)  # :84-88

    unused_table_inds = []
    unused_table_vals = []
    permuted_table = [0] * n
    i = 0
    j = 0
    while j < n and i < n:  # :95
        input_val = sorted_inputs[i]
        table_val = sorted_table[j]
        if input_val > table_val:  # Ordering::Greater
            unused_table_vals.append(sorted_table[j])
            j += 1
        elif input_val < table_val:  # Ordering::Less
            if unused_table_vals:
                permuted_table[i] = unused_table_vals.pop()
            else:
                unused_table_inds.append(i)
            i += 1
        else:  # Ordering::Equal
            permuted_table[i] = sorted_table[j]
            i += 1
            j += 1

    for jj in range(j, n):  # :120-122
        unused_table_vals.append(sorted_table[jj])
    for ii in range(i, n):  # :123-125
        unused_table_inds.append(ii)
    assert len(unused_table_inds) == len(unused_table_vals)  # zip_eq
    for ind, val in zip(unused_table_inds, unused_table_vals):  # :126-128
        permuted_table[ind] = val

    return sorted_inputs, permuted_table


def check_lookup_argument(inputs, table, permuted_inputs, permuted_table):
    """What the constraints of eval_lookups (lookup.rs:13-34) and the two permutation pairs (memory_stark.rs:452-456) accept: raises
    AssertionError with the reason otherwise."""
    n = len(inputs)
    assert len(table) == n and len(permuted_inputs) == n and len(permuted_table) == n, "lengths"
    assert all(0 <= int(x) < P for x in permuted_inputs) and all(0 <= int(x) < P for x in permuted_table), "outputs are canonical"
    pi, pt = [int(x) for x in permuted_inputs], [int(x) for x in permuted_table]
    assert sorted(pi) == sort_canonical(inputs), "permuted_inputs is a permutation of the inputs"
    assert sorted(pt) == sort_canonical(table), "permuted_table is a permutation of the table"
    assert pi[0] == pt[0], "row 0: the permuted input equals the permuted table value"
    for r in range(1, n):
        assert pi[r] == pi[r - 1] or pi[r] == pt[r], "row %d: neither a repeat of the row above nor the table value beside it" % r
