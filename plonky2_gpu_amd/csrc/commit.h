// commit.h — the one commit behind gl_commit_from_{coeffs,values}[_h] and the reference symbol merkle_tree_from_coeffs (commit.hip).
#pragma once
#include "ctx.h"

namespace plonky2_hip {

extern const char *const KECCAK_LEAF_LEN_4;  // why no Keccak tree takes a leaf of four elements

// What commit_from_coeffs refuses, or null: checked before anything is launched, and by gl_commit_from_values[_h] before d_values
// is transformed in place, so that a refused call leaves the caller's buffers as they were.
const char *commit_argument_error(uint32_t hasher, const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                                  uint32_t cap_height, uint32_t salt_size, const uint64_t *d_lde, const uint64_t *d_digests,
                                  const uint64_t *d_cap, const void *ctx);

// gl_commit_from_coeffs_h (include/plonky2_hip.h) on the context's streams; its device is current.
GlError commit_from_coeffs(uint32_t hasher, const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                           uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde, uint64_t *d_leaves,
                           uint64_t *d_digests, uint64_t *d_cap, Streams *s);

// dst[i] = the canonical representative of src[i], i < n; dst == src reduces in place
hipError_t canon_copy(uint64_t *dst, const uint64_t *src, uint64_t n, hipStream_t stream);

}  // namespace plonky2_hip
