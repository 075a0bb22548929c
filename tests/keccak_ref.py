"""The truth for the Keccak Merkle tests: a vectorised numpy Keccak (a batch of states as uint64[.., 25]) with the padding byte
as a parameter, plonky2's KeccakHash<25> on top of it (plonky2/src/hash/keccak.rs:53-83, plonk/config.rs:54-67) and a Merkle
tree in the reference's digest layout (hash/merkle_tree.rs:46-54, 283-319). Pinned by tests/test_keccak_ref.py against
hashlib.sha3_256 (same permutation and rate, padding byte 0x06) and the published Keccak-256 values.

Hashes are uint8[.., 25]; `slots` turns them into the device layout (4 u64 per digest: bytes 0..24 the hash, 25..31 zero)."""
import numpy as np

P = 0xFFFFFFFF00000001
RATE = 136  # bytes: Keccak-256
N = 25  # KeccakHash<25>

_RC = np.array([0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
                0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
                0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
                0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008],
               dtype=np.uint64)


def _rho_offsets():
    """rotation of lane (x, y), from the walk (x, y) -> (y, 2x + 3y) with offsets (t + 1)(t + 2) / 2 (FIPS 202, 3.2.2)"""
    r = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


_RHO = _rho_offsets()


def _rotl(a, n):
    n %= 64
    return a if n == 0 else (a << np.uint64(n)) | (a >> np.uint64(64 - n))


def keccak_f1600(states):
    """keccak-f[1600] on every state of uint64[.., 25] (lane x + 5 y), returns a new array"""
    a = np.array(states, dtype=np.uint64)
    A = [[a[..., x + 5 * y].copy() for y in range(5)] for x in range(5)]
    for rnd in range(24):
        C = [A[x][0] ^ A[x][1] ^ A[x][2] ^ A[x][3] ^ A[x][4] for x in range(5)]
        D = [C[(x - 1) % 5] ^ _rotl(C[(x + 1) % 5], 1) for x in range(5)]
        B = [[None] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                B[y][(2 * x + 3 * y) % 5] = _rotl(A[x][y] ^ D[x], _RHO[x][y])
        A = [[B[x][y] ^ (~B[(x + 1) % 5][y] & B[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        A[0][0] = A[0][0] ^ _RC[rnd]
    out = np.empty_like(a)
    for x in range(5):
        for y in range(5):
            out[..., x + 5 * y] = A[x][y]
    return out


def keccak256_batch(messages, pad_byte=0x01):
    """messages uint8[count, length] (all of one length) -> uint8[count, 32]: the sponge with rate 136 and capacity 512, pad10*1 with
    `pad_byte` as the first padding byte (0x01: Keccak-256 as plonky2's keccak_hash crate computes it; 0x06: SHA3-256)"""
    m = np.ascontiguousarray(messages, dtype=np.uint8)
    count, length = m.shape
    blocks = length // RATE + 1
    padded = np.zeros((count, blocks * RATE), dtype=np.uint8)
    padded[:, :length] = m
    padded[:, length] ^= np.uint8(pad_byte)
    padded[:, -1] ^= np.uint8(0x80)
    words = padded.view("<u8").reshape(count, blocks, RATE // 8)
    state = np.zeros((count, 25), dtype=np.uint64)
    for b in range(blocks):
        state[:, : RATE // 8] ^= words[:, b, :]
        state = keccak_f1600(state)
    return np.ascontiguousarray(state[:, :4]).astype("<u8").view(np.uint8).reshape(count, 32)


def keccak256(data, pad_byte=0x01):
    """bytes -> 32 bytes"""
    return keccak256_batch(np.frombuffer(bytes(data), dtype=np.uint8).reshape(1, -1), pad_byte)[0].tobytes()


def canon(x):
    x = np.asarray(x, dtype=np.uint64)
    return np.where(x >= np.uint64(P), x - np.uint64(P), x)


def field_bytes(x):
    """uint64[count, len] -> uint8[count, 8 len]: to_canonical_u64 of every element, little endian (util/serialization.rs:492-509)"""
    x = np.asarray(x, dtype=np.uint64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    return np.ascontiguousarray(canon(x)).astype("<u8").view(np.uint8).reshape(x.shape[0], 8 * x.shape[1])


def hash_no_pad(x):
    """KeccakHash<25>::hash_no_pad of every row of uint64[count, len] (or of one vector) -> uint8[count, 25]"""
    return keccak256_batch(field_bytes(x))[:, :N].copy()


def hash_or_noop(x):
    """plonk/config.rs:54-67: rows of at most 3 elements are their own bytes, zero padded to 25; the reference panics at 4"""
    x = np.asarray(x, dtype=np.uint64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    if x.shape[1] == 4:
        raise ValueError("KeccakHash<25>::hash_or_noop panics for 4 elements (32 bytes into a 25-byte hash)")
    if x.shape[1] * 8 <= N:
        out = np.zeros((x.shape[0], N), dtype=np.uint8)
        out[:, : 8 * x.shape[1]] = field_bytes(x)
        return out
    return hash_no_pad(x)


def two_to_one(left, right):
    """uint8[count, 25] each -> uint8[count, 25]: Keccak-256 of the 50 bytes l || r"""
    l, r = np.asarray(left, dtype=np.uint8).reshape(-1, N), np.asarray(right, dtype=np.uint8).reshape(-1, N)
    return keccak256_batch(np.concatenate([l, r], axis=1))[:, :N].copy()


def slots(hashes):
    """uint8[count, 25] -> uint64[count, 4]: the device layout of a digest"""
    h = np.asarray(hashes, dtype=np.uint8).reshape(-1, N)
    buf = np.zeros((h.shape[0], 32), dtype=np.uint8)
    buf[:, :N] = h
    return buf.view("<u8").astype(np.uint64).reshape(-1, 4)


def hash_bytes(slot_words):
    """uint64[.., 4] -> uint8[.., 25]; asserts that bytes 25..31 of every slot are zero"""
    s = np.ascontiguousarray(slot_words, dtype=np.uint64)
    b = s.astype("<u8").view(np.uint8).reshape(s.shape[:-1] + (32,))
    assert not b[..., N:].any(), "bytes 25..31 of a digest slot are not zero"
    return b[..., :N].copy()


def _digest_slot(idx, layer):
    """index of node `idx` of layer `layer` inside a cap subtree's digest array (the closed form of MerkleTree::prove,
    merkle_tree.rs:424-435)"""
    q, parity = idx >> 1, idx & 1
    return 2 * ((q << (layer + 1)) + (1 << layer) - 1) + parity


def merkle_tree(leaves, cap_height):
    """MerkleTree::new(leaves, cap_height) -> (digests uint8[2 (n - 2^cap_height), 25], cap uint8[2^cap_height, 25]), digests in the
    reference's "left subtree | left digest | right digest | right subtree" order (merkle_tree.rs:46-54, 210-244)"""
    return merkle_tree_from_leaf_hashes(hash_or_noop(leaves), cap_height)


def merkle_tree_from_leaf_hashes(level, cap_height):
    n = level.shape[0]
    lg = n.bit_length() - 1
    assert n == 1 << lg and cap_height <= lg
    log_sub = lg - cap_height
    n_sub = 1 << cap_height
    sub_digests = 2 * ((1 << log_sub) - 1)
    digests = np.zeros((n_sub * sub_digests, N), dtype=np.uint8)
    for layer in range(log_sub):
        per_sub = 1 << (log_sub - layer)
        g = np.arange(level.shape[0])
        sub, idx = g // per_sub, g % per_sub
        digests[sub * sub_digests + _digest_slot(idx, layer)] = level
        level = two_to_one(level[0::2], level[1::2])
    return digests, level


def merkle_verify(leaf, leaf_index, cap, siblings):
    """verify_merkle_proof_to_cap (hash/merkle_proofs.rs:57-86): leaf uint64[len], siblings uint8[layers, 25], cap uint8[.., 25]"""
    cur = hash_or_noop(np.asarray(leaf, dtype=np.uint64).reshape(1, -1))
    idx = int(leaf_index)
    for sib in np.asarray(siblings, dtype=np.uint8).reshape(-1, N):
        cur = two_to_one(cur, sib) if idx & 1 == 0 else two_to_one(sib, cur)
        idx >>= 1
    return bool((cur[0] == np.asarray(cap, dtype=np.uint8).reshape(-1, N)[idx]).all())


def merkle_verify_batch(leaves, indices, cap, siblings):
    """the same for many openings at once: leaves uint64[count, len], siblings uint8[count, layers, 25] -> bool[count]"""
    cur = hash_or_noop(leaves)
    idx = np.asarray(indices, dtype=np.int64).copy()
    sib = np.asarray(siblings, dtype=np.uint8)
    for l in range(sib.shape[1]):
        odd = (idx & 1).astype(bool)[:, None]
        cur = two_to_one(np.where(odd, sib[:, l], cur), np.where(odd, cur, sib[:, l]))
        idx >>= 1
    return (cur == np.asarray(cap, dtype=np.uint8).reshape(-1, N)[idx]).all(axis=1)
