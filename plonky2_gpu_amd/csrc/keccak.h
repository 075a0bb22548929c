// keccak.h — internal interface of the Keccak-256 Merkle kernels (see keccak.hip): plonky2's KeccakHash<25>
// (plonky2/src/hash/keccak.rs:53-83) as the tree hasher of KeccakGoldilocksConfig (plonk/config.rs:110-128).
// A digest is a 32-byte slot (4 u64): bytes 0..24 the hash, bytes 25..31 zero; every index is merkle_layout.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

// out[i][4] = hash_no_pad(inputs[i*stride .. i*stride + len)) for i < count (always hashed: len <= 4 included).
hipError_t keccak_hash_no_pad_batch(const uint64_t *inputs, uint32_t len, uint64_t stride, uint64_t count, uint64_t *out, hipStream_t stream);
// MerkleTree::new with hash_or_noop leaves; element j of leaf i at leaves[i*row_stride + j*elem_stride] (columns: (1, col_stride),
// leaf-major rows: (leaf_len, 1)). leaf_len == 4 has no hash_or_noop (the reference panics): hipErrorInvalidValue, nothing launched.
hipError_t keccak_merkle_tree(const uint64_t *leaves, uint64_t row_stride, uint64_t elem_stride, uint32_t leaf_len, uint64_t n_leaves,
                              uint32_t cap_height, uint64_t *digests, uint64_t *cap, hipStream_t stream);

}  // namespace plonky2_hip
