"""Record lists for the Poseidon table's tests (TEST INFRASTRUCTURE): [num_ops][13] uint64 records of gl_poseidon_table_trace — the
kind (0 = START: words 1 .. 12 are the input state; k = 1 .. 8 = ABSORB: words 1 .. k overwrite elements 0 .. k - 1 of the OUTPUT
of the row before), then twelve element words, any u64. Every family is a function of the number of records; a list cut to a
prefix is still valid, it only shortens its last run."""
import numpy as np

P = 0xFFFFFFFF00000001
ONES = (1 << 64) - 1
OP_WORDS = 13
NONCANONICAL = [P, P + 1, ONES, (1 << 32) - 1]  # the last is canonical: 2^64 mod p, what the others' reduction involves


def _elements(rng, shape):
    """canonical elements: whatever is ignored or overwritten is random as well, which a kernel that reads too far shows"""
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _with_kinds(kinds, rng):
    out = np.zeros((len(kinds), OP_WORDS), dtype=np.uint64)
    out[:, 0] = np.asarray(kinds, dtype=np.uint64)
    out[:, 1:] = _elements(rng, (len(kinds), 12))
    return out


def starts(num_ops, seed=1):
    """plain permutations"""
    return _with_kinds([0] * num_ops, np.random.default_rng([seed, num_ops]))


def pairs(num_ops, seed=2):
    """two-to-one compressions: two digests of four elements over four zeros"""
    out = starts(num_ops, seed)
    out[:, 9:] = 0
    return out


def runs(num_ops, lengths, last_kind=lambda length: 8, seed=3):
    """runs of the given lengths (cycled), cut at num_ops: a START whose capacity is zero, then ABSORBs of 8, the run's last of
    last_kind(length)"""
    kinds, k = [], 0
    while len(kinds) < num_ops:
        length = lengths[k % len(lengths)]
        kinds += [0] + [8] * max(length - 2, 0) + ([last_kind(length)] if length > 1 else [])
        k += 1
    out = _with_kinds(kinds[:num_ops], np.random.default_rng([seed, num_ops]))
    out[out[:, 0] == 0, 9:] = 0
    return out


def leaves135(num_ops, seed=4):
    """the sponge of a 135-element leaf: 17-row runs whose last ABSORB has 135 - 16 * 8 = 7 elements"""
    return runs(num_ops, [17], lambda length: 7, seed)


def mixed(num_ops, seed=5):
    """random run lengths 1 .. 40, the kinds of the ABSORBs cycling through 1 .. 8: every kind 0 .. 8 is present from 10 records on
    whatever the lengths are, because the first run is given 9 rows"""
    rng = np.random.default_rng([seed, 0])  # the same lengths and kinds for every num_ops: a shorter list is a prefix's shape
    kinds, absorb = [], 0
    first = True
    while len(kinds) < num_ops:
        length = 9 if first else int(rng.integers(1, 41))
        first = False
        kinds.append(0)
        for _ in range(length - 1):
            kinds.append(1 + absorb % 8)
            absorb += 1
    return _with_kinds(kinds[:num_ops], np.random.default_rng([seed, 1, num_ops]))


def one_run(num_ops, seed=6):
    """one run as long as the list"""
    return runs(num_ops, [max(num_ops, 1)], seed=seed)


def noncanonical(num_ops, seed=7):
    """the words p, p + 1, 2^64 - 1 and 2^32 - 1 in every position, in STARTs and in ABSORBs: record k is a START where k is a
    multiple of 3 and an ABSORB of 8 otherwise, and carries NONCANONICAL[(k // 3) % 4] at element (k // 12) % 12 (an ABSORB:
    modulo 8); from 144 records on every word has stood in every position of either kind"""
    kinds = [0 if k % 3 == 0 else 8 for k in range(num_ops)]
    out = _with_kinds(kinds, np.random.default_rng([seed, num_ops]))
    for k in range(num_ops):
        word = NONCANONICAL[(k // 3) % 4]
        position = (k // 12) % 12
        out[k, 1 + (position if kinds[k] == 0 else position % 8)] = word
    return out


FAMILIES = {"starts": starts, "pairs": pairs, "leaves135": leaves135, "mixed": mixed, "one_run": one_run, "noncanonical": noncanonical}
