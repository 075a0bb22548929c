// merkle_layout.h — where a digest lives: the one piece of the Merkle code that does not depend on the hasher.
//
// A digest occupies one SLOT of 4 u64 (32 bytes): a Poseidon HashOut fills it, a 25-byte Keccak hash fills bytes 0..24 and
// leaves bytes 25..31 zero. `digests` is the reference's recursive "left subtree | left digest | right digest | right
// subtree" array (plonky2/src/hash/merkle_tree.rs:46-54), one such array of 2 * (2^log_sub_leaves - 1) slots per cap
// entry, back to back; `cap` holds the 2^cap_height subtree roots. merkle.hip (Poseidon, and the openings of either hasher:
// merkle_open_kernel) and keccak.hip both take digest_slot from here, so that openings, MerkleTree::prove and every buffer size
// hold for either hasher. leaf_digest and layer_node spell out what merkle.hip's kernels compute inline around digest_slot;
// keccak.hip uses them, the Poseidon kernels keep their own text (rewriting them onto these helpers changes their compiled code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

// hash index (in units of 4 u64) of node `idx` of layer L inside a cap subtree
__device__ __forceinline__ uint64_t digest_slot(uint64_t idx, uint32_t L) {
    uint64_t q = idx >> 1, parity = idx & 1;
    return 2 * ((q << (L + 1)) + (1ull << L) - 1) + parity;
}

// slots of one cap subtree's digest array
__device__ __forceinline__ uint64_t subtree_slots(uint32_t log_sub_leaves) { return 2 * ((1ull << log_sub_leaves) - 1); }

// the slot of leaf i's hash: in its subtree's digest array, or the cap itself when the subtrees are single leaves
__device__ __forceinline__ uint64_t *leaf_digest(uint64_t *digests, uint64_t *cap, uint64_t i, uint32_t log_sub_leaves) {
    if (log_sub_leaves == 0) return cap + 4 * i;
    const uint64_t sub = i >> log_sub_leaves, idx = i & ((1ull << log_sub_leaves) - 1);
    return digests + 4 * (sub * subtree_slots(log_sub_leaves) + digest_slot(idx, 0));
}

// Pair g of layer L, counted over all cap subtrees (2^(log_sub_leaves - L - 1) pairs each): `children` = its left digest,
// the right one in the next slot; `parent` = where two_to_one of them goes, layer L + 1 or the cap.
struct LayerNode {
    const uint64_t *children;
    uint64_t *parent;
};
__device__ __forceinline__ LayerNode layer_node(uint64_t *digests, uint64_t *cap, uint64_t g, uint32_t L, uint32_t log_sub_leaves) {
    const uint32_t log_pairs = log_sub_leaves - L - 1;
    const uint64_t sub = g >> log_pairs, q = g & ((1ull << log_pairs) - 1);
    uint64_t *tree = digests + 4 * sub * subtree_slots(log_sub_leaves);
    return LayerNode{tree + 4 * digest_slot(2 * q, L), log_pairs == 0 ? cap + 4 * sub : tree + 4 * digest_slot(q, L + 1)};
}

}  // namespace plonky2_hip
