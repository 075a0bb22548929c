// keccak.hip — Keccak-256 leaf hashing and Merkle-cap construction: MerkleTree::new (plonky2/src/hash/merkle_tree.rs:283-319)
// with H = KeccakHash<25> (plonky2/src/hash/keccak.rs:53-83), the tree hasher of KeccakGoldilocksConfig.
//
//   hash_no_pad(x)   = first 25 bytes of Keccak-256 (original padding 0x01 .. 0x80, rate 136 bytes = 17 field elements) over the
//                      canonical words of x, little endian (util/serialization.rs:492-509)
//   two_to_one(l, r) = first 25 bytes of Keccak-256 of the 50 bytes l || r
//   hash_or_noop(x)  = the canonical words themselves, zero padded to 25 bytes, for len <= 3; hash_no_pad for len >= 5
//                      (plonk/config.rs:54-67; len == 4 panics there and is refused by the host code here)
//
// A digest is a 32-byte slot, bytes 25..31 zero, at the index merkle_layout.h gives it: the digest array, the cap and the
// openings are laid out exactly as the Poseidon trees of merkle.hip.
//
// keccak-f[1600] runs with the whole state in registers (keccak_f1600.h, shared with the Keccak sponge table). One lane hashes one
// leaf (or one parent), so a wave reads 64 consecutive words of a column per load.
#include "keccak.h"

#include "gl_field.h"
#include "keccak_f1600.h"
#include "merkle_layout.h"

namespace plonky2_hip {

namespace {

constexpr int RATE_WORDS = 17;  // 136 bytes

struct alignas(16) u64x2 {
    uint64_t x, y;
};

__device__ __forceinline__ void clear(KeccakState &s) {
#pragma unroll
    for (int k = 0; k < 25; k++) s.lo[k] = s.hi[k] = 0;
}

__device__ __forceinline__ void absorb_word(KeccakState &s, int k, uint64_t w) {
    s.lo[k] ^= (uint32_t)w;
    s.hi[k] ^= (uint32_t)(w >> 32);
}

// the first 25 bytes of the state into a digest slot, bytes 25..31 zero
__device__ __forceinline__ void store_digest(uint64_t *dst, const KeccakState &s) {
    reinterpret_cast<u64x2 *>(dst)[0] = u64x2{(uint64_t)s.hi[0] << 32 | s.lo[0], (uint64_t)s.hi[1] << 32 | s.lo[1]};
    reinterpret_cast<u64x2 *>(dst)[1] = u64x2{(uint64_t)s.hi[2] << 32 | s.lo[2], (uint64_t)(s.lo[3] & 0xffu)};
}

// The hash of every leaf: element j of leaf i at leaves[i * row_stride + j * elem_stride]. With the columns of an LDE
// (row_stride 1) the 64 lanes of a wave read 512 contiguous bytes of one column per load, whatever the column pitch.
// OR_NOOP: leaves of up to three elements are copied, not hashed (hash_or_noop); without it everything is hashed (hash_no_pad).
template <bool OR_NOOP>
__global__ __launch_bounds__(256) void keccak_leaves_kernel(const uint64_t *__restrict__ leaves, uint64_t row_stride, uint64_t elem_stride,
                                                            uint32_t leaf_len, uint64_t n_leaves, uint64_t *__restrict__ digests,
                                                            uint64_t *__restrict__ cap, uint32_t log_sub_leaves) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_leaves) return;
    const uint64_t *leaf = leaves + i * row_stride;
    uint64_t *dst = leaf_digest(digests, cap, i, log_sub_leaves);
    if (OR_NOOP && leaf_len <= 3) {
        uint64_t w[3];
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = (uint32_t)k < leaf_len ? gl::canon(leaf[(uint64_t)k * elem_stride]) : 0;
        reinterpret_cast<u64x2 *>(dst)[0] = u64x2{w[0], w[1]};
        reinterpret_cast<u64x2 *>(dst)[1] = u64x2{w[2], 0};
        return;
    }
    KeccakState s;
    clear(s);
    for (uint32_t j = 0;; j += RATE_WORDS) {
        const uint32_t r = leaf_len - j;  // words left; a block takes 17 of them, the last block the rest (0..16) and the padding
        uint64_t w[RATE_WORDS];
        if (r >= RATE_WORDS) {
#pragma unroll
            for (int k = 0; k < RATE_WORDS; k++) w[k] = leaf[(uint64_t)(j + k) * elem_stride];
        } else {
#pragma unroll
            for (int k = 0; k < RATE_WORDS; k++) w[k] = (uint32_t)k < r ? leaf[(uint64_t)(j + k) * elem_stride] : 0;
        }
#pragma unroll
        for (int k = 0; k < RATE_WORDS; k++) absorb_word(s, k, gl::canon(w[k]));
        if (r < RATE_WORDS) {  // pad10*1 with Keccak's domain byte: 0x01 behind the message, 0x80 in the block's last byte
#pragma unroll
            for (int k = 0; k < RATE_WORDS; k++)
                if ((uint32_t)k == r) s.lo[k] ^= 1u;
            s.hi[RATE_WORDS - 1] ^= 0x80000000u;
        }
        keccak_f1600(s);
        if (r < RATE_WORDS) break;
    }
    store_digest(dst, s);
}

// One tree layer for all cap subtrees: parent = two_to_one(left, right), the Keccak-256 of the two 25-byte hashes back to
// back. Lane g handles pair g of layer L (merkle_layout.h). 50 bytes and the padding fit one block: one permutation.
__global__ __launch_bounds__(256) void keccak_tree_layer_kernel(uint64_t *__restrict__ digests, uint64_t *__restrict__ cap, uint32_t L,
                                                                uint32_t log_sub_leaves, uint64_t total_pairs) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total_pairs) return;
    const LayerNode node = layer_node(digests, cap, g, L, log_sub_leaves);
    const u64x2 *pair = reinterpret_cast<const u64x2 *>(node.children);
    const u64x2 a = pair[0], b = pair[1], c = pair[2], d = pair[3];
    // bytes 0..24 the left hash, 25..49 the right one: the right slot's words move up by one byte
    const uint64_t l3 = b.y & 0xff, r3 = d.y & 0xff;
    KeccakState s;
    clear(s);
    absorb_word(s, 0, a.x);
    absorb_word(s, 1, a.y);
    absorb_word(s, 2, b.x);
    absorb_word(s, 3, l3 | c.x << 8);
    absorb_word(s, 4, c.x >> 56 | c.y << 8);
    absorb_word(s, 5, c.y >> 56 | d.x << 8);
    absorb_word(s, 6, d.x >> 56 | r3 << 8 | 0x01ull << 16);  // byte 50: the padding's first byte
    s.hi[RATE_WORDS - 1] ^= 0x80000000u;
    keccak_f1600(s);
    store_digest(node.parent, s);
}

unsigned grid_for(uint64_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

int log2_exact(uint64_t n) {
    int l = 0;
    while (l < 63 && (1ull << l) < n) l++;
    return (1ull << l) == n ? l : -1;
}

}  // namespace

hipError_t keccak_hash_no_pad_batch(const uint64_t *inputs, uint32_t len, uint64_t stride, uint64_t count, uint64_t *out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (count > 0xFFFFFFFFull * 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keccak_leaves_kernel<false>, dim3(grid_for(count, 256)), dim3(256), 0, stream, inputs, stride, (uint64_t)1, len, count,
                       (uint64_t *)nullptr, out, 0u);
    return hipGetLastError();
}

hipError_t keccak_merkle_tree(const uint64_t *leaves, uint64_t row_stride, uint64_t elem_stride, uint32_t leaf_len, uint64_t n_leaves,
                              uint32_t cap_height, uint64_t *digests, uint64_t *cap, hipStream_t stream) {
    const int lg = log2_exact(n_leaves);
    if (lg < 0 || (int)cap_height > lg || leaf_len == 4) return hipErrorInvalidValue;
    const uint32_t log_sub = (uint32_t)lg - cap_height;
    hipLaunchKernelGGL(keccak_leaves_kernel<true>, dim3(grid_for(n_leaves, 256)), dim3(256), 0, stream, leaves, row_stride, elem_stride, leaf_len,
                       n_leaves, digests, cap, log_sub);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint64_t n_sub = n_leaves >> log_sub;
    for (uint32_t L = 0; L < log_sub; L++) {
        const uint64_t total = n_sub << (log_sub - L - 1);
        hipLaunchKernelGGL(keccak_tree_layer_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, digests, cap, L, log_sub, total);
    }
    return hipGetLastError();
}

}  // namespace plonky2_hip
