"""Non-canonical representatives of Goldilocks elements, for the tests of the header's promise (include/plonky2_hip.h,
Conventions): every input may be any u64 representative, every output is canonical.

plonky2's own field arithmetic does not reduce its results (goldilocks_field.rs: Add returns Self(sum), reduce128 returns
GoldilocksField(t2)), so words in [p, 2^64) reach the library from a Rust host. Only x < 2^32 - 1 has a second
representative x + p below 2^64: data meant to be lifted are mostly small values (see field_data)."""
import numpy as np

P = 0xFFFFFFFF00000001
LIFTABLE = (1 << 32) - 1  # x + p < 2^64 exactly when x < LIFTABLE

# canonical values where field arithmetic goes wrong first
EDGES = [0, 1, 2, 3, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, P - 2, P - 1]
# lift() gives the small ones their second representative x + p: p, p + 1, .., 2^64 - 1 (= 2^32 - 2)


def lift_scalar(x):
    """x + p where that fits 64 bits, else x itself (x canonical)"""
    x = int(x) % P
    return x + P if x < LIFTABLE else x


def lift(a, rng, frac=0.5):
    """(copy of the uint64 array `a` in which a fraction `frac` of the entries with x < 2^32 - 1 became x + p,
    number of entries lifted)"""
    a = np.array(a, dtype=np.uint64)
    mask = (a < np.uint64(LIFTABLE)) & (rng.random(a.shape) < frac)
    out = a.copy()
    out[mask] += np.uint64(P)
    return out, int(mask.sum())


def field_data(rng, shape, small=0.7, edges=0.1):
    """canonical uint64 data: mostly values below 2^32 - 1 (liftable), some of EDGES, the rest uniform in [0, p)"""
    u = rng.random(shape)
    small_v = rng.integers(0, LIFTABLE, size=shape, dtype=np.uint64)
    edge_v = np.array(EDGES, dtype=np.uint64)[rng.integers(0, len(EDGES), size=shape)]
    rand_v = rng.integers(0, P, size=shape, dtype=np.uint64)
    return np.where(u < small, small_v, np.where(u < small + edges, edge_v, rand_v)).astype(np.uint64)


def all_canonical(a):
    return bool((np.asarray(a, dtype=np.uint64) < np.uint64(P)).all())
