"""Operation lists for the logic table's tests (TEST INFRASTRUCTURE): [num_ops][17] uint64 records of gl_logic_table_trace — the
operator (0 = AND, 1 = OR, 2 = XOR), the eight 32-bit limbs of input0, the eight of input1, least significant first."""
import numpy as np

import logic_table_ref as lr

M32 = (1 << 32) - 1
EDGE_LIMBS = np.array([0, M32, 1 << 31], dtype=np.uint64)


def words(operators, input0, input1):
    n = len(operators)
    out = np.zeros((n, lr.OP_WORDS), dtype=np.uint64)
    out[:, 0] = np.asarray(operators, dtype=np.uint64)
    out[:, 1:9] = np.asarray(input0, dtype=np.uint64).reshape(n, 8)
    out[:, 9:17] = np.asarray(input1, dtype=np.uint64).reshape(n, 8)
    return out


def _limbs(rng, n):
    return rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64)


def random_ops(num_ops, seed=1):
    """random operations over all three operators"""
    rng = np.random.default_rng([seed, num_ops])
    return words(rng.integers(0, 3, num_ops), _limbs(rng, num_ops), _limbs(rng, num_ops))


def edge_limbs(num_ops, seed=2):
    """every limb is 0, 2^32 - 1 or has only bit 31 set"""
    rng = np.random.default_rng([seed, num_ops])
    return words(rng.integers(0, 3, num_ops), EDGE_LIMBS[rng.integers(0, 3, (num_ops, 8))], EDGE_LIMBS[rng.integers(0, 3, (num_ops, 8))])


def equal_inputs(num_ops, seed=3):
    """input0 == input1: AND and OR give the input, XOR gives zero"""
    rng = np.random.default_rng([seed, num_ops])
    x = _limbs(rng, num_ops)
    return words(rng.integers(0, 3, num_ops), x, x)


def one_operator(num_ops, operator, seed=4):
    rng = np.random.default_rng([seed, num_ops, operator])
    return words(np.full(num_ops, operator), _limbs(rng, num_ops), _limbs(rng, num_ops))


def mixed(num_ops, seed=5):
    """record k is of family k mod 6: random, edge limbs, equal inputs, AND only, OR only, XOR only — neighbours differ in every
    column, which a row written to the wrong place shows"""
    parts = [random_ops(num_ops, seed), edge_limbs(num_ops, seed), equal_inputs(num_ops, seed)] + [one_operator(num_ops, op, seed) for op in range(3)]
    out = np.zeros((num_ops, lr.OP_WORDS), dtype=np.uint64)
    for k in range(num_ops):
        out[k] = parts[k % 6][k]
    return out


FAMILIES = {"random": random_ops, "edge_limbs": edge_limbs, "equal_inputs": equal_inputs, "and_only": lambda n: one_operator(n, 0),
            "or_only": lambda n: one_operator(n, 1), "xor_only": lambda n: one_operator(n, 2), "mixed": mixed}
