// commit.hip — PolynomialBatch::from_coeffs on the device: LDE, leaf-major copy, Merkle tree, for both hashers (commit.h).
#include "commit.h"

#include <algorithm>

#include <stdlib.h>

#include "gl_field.h"
#include "keccak.h"
#include "knobs.h"
#include "merkle.h"

namespace plonky2_hip {

const char *const KECCAK_LEAF_LEN_4 = "KeccakHash<25>::hash_or_noop is undefined for leaves of 4 elements (plonk/config.rs:58-63 panics)";

namespace {

bool knob_on(const char *value) { return !(value && value[0] == '0'); }  // on unless the variable starts with '0'; read once

__global__ __launch_bounds__(256) void canon_copy_kernel(uint64_t *dst, const uint64_t *src, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) dst[i] = gl::canon(src[i]);
}

}  // namespace

hipError_t canon_copy(uint64_t *dst, const uint64_t *src, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(canon_copy_kernel, dim3((unsigned)std::min<uint64_t>(blocks, 8192)), dim3(256), 0, stream, dst, src, n);
    return hipGetLastError();
}

// The two hashers differ in exactly two rules. A Keccak tree that is all cap writes no digest, so it takes a null d_digests; the
// Poseidon kernels are handed the pointer in every shape. And Keccak has no leaf of four elements.
const char *commit_argument_error(uint32_t hasher, const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                                  uint32_t cap_height, uint32_t salt_size, const uint64_t *d_lde, const uint64_t *d_digests,
                                  const uint64_t *d_cap, const void *ctx) {
    if (hasher != GL_HASHER_POSEIDON && hasher != GL_HASHER_KECCAK25) return "unknown hasher";
    const bool keccak = hasher == GL_HASHER_KECCAK25;
    if (!d_coeffs || !d_lde || !d_cap || !ctx) return "null pointer";
    if (log_n > 24) return "log_n > 24 is not supported by this build";
    if (log_n + rate_bits > 32 || cap_height > log_n + rate_bits) return "cap_height should be at most log2(leaves.len())";
    if (!d_digests && !(keccak && cap_height == log_n + rate_bits)) return "null pointer";
    if (poly_num + salt_size == 0 || poly_num + salt_size > 0xFFFFFFFFull) return "bad poly_num";
    if (keccak && poly_num + salt_size == 4) return KECCAK_LEAF_LEN_4;
    return nullptr;
}

GlError commit_from_coeffs(uint32_t hasher, const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                           uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde, uint64_t *d_leaves,
                           uint64_t *d_digests, uint64_t *d_cap, Streams *s) {
    if (const char *why = commit_argument_error(hasher, d_coeffs, poly_num, log_n, rate_bits, cap_height, salt_size, d_lde, d_digests, d_cap, s))
        return fail(GL_E_INVALID, why);
    const bool keccak = hasher == GL_HASHER_KECCAK25;
    const uint64_t n = 1ull << log_n, n_ext = n << rate_bits;
    const uint32_t leaf_len = (uint32_t)(poly_num + salt_size);
    const NttTables *tb;
    CosetLease ct;
    HIP_TRY(get_tables(s, &tb));
    HIP_TRY(get_coset_tables(log_n, rate_bits, shift, s->stream, &ct));
    // The caller's salt columns in d_lde, reduced in place: the tree hashes any representative alike, but d_lde and the leaf-major
    // copies of it (fused row stores, transpositions) are outputs and hold canonical words
    // (tests/test_gpu_representatives.py::test_commit_from_values_and_coeffs, lifted salts with leaf_major). On the caller's stream,
    // ahead of everything below that reads the salt columns (the hash stream starts behind it).
    HIP_TRY(canon_copy(d_lde + poly_num * n_ext, d_lde + poly_num * n_ext, (uint64_t)salt_size * n_ext, s->stream));

    // An error after work has been queued on the hash stream or on stream2 must not leave those kernels running behind
    // the caller's back (its gl_ctx_synchronize and frees only cover its own stream): the failing call waits for both.
    hipStream_t hs = nullptr;
    bool on_stream2 = false;

    // tree() beside the leaf-major copy of d_lde into `leaves` (null: no copy, just the tree). The copy is pure HBM traffic and
    // the hashing pure integer ALU work, so the transposition runs on stream2, concurrently with the tree. It starts after the
    // LDE (event) and after whatever the caller queued on stream2 before this call — the reference's caller has its D2H of the
    // coefficients there (oracle.rs:403-407), which is exactly what must finish before region A is overwritten
    // (plonky2_gpu.cu:586), now by stream order instead of a host-side stream synchronise. `leaves` may overlap d_coeffs: the
    // last LDE launch, the last reader of d_coeffs, is ahead of the event. The caller's stream continues after the tree and the leaves.
    auto beside_leaf_major_copy = [&](uint64_t *leaves, auto tree) -> GlError {
        if (!leaves) return tree();
        hipEvent_t ev_lde = nullptr, ev_tr = nullptr;
        HIP_TRY(get_events(s, &ev_lde, &ev_tr));
        HIP_TRY(hipEventRecord(ev_lde, s->stream));
        HIP_TRY(hipStreamWaitEvent(s->stream2, ev_lde, 0));
        on_stream2 = true;
        HIP_TRY(transpose_to_leaf_major(d_lde, leaves, leaf_len, n_ext, n_ext, s->stream2));
        HIP_TRY(hipEventRecord(ev_tr, s->stream2));
        TRY(tree());
        HIP_TRY(hipStreamWaitEvent(s->stream, ev_tr, 0));
        return ok();
    };

    // Fused leaves: the hashing lanes on `writer` write d_leaves, which may still be read by what the caller queued on stream2
    // (the same D2H of the reference's caller)
    auto wait_for_stream2 = [&](hipStream_t writer) -> GlError {
        hipEvent_t ev_a = nullptr, ev_b = nullptr;
        HIP_TRY(get_events(s, &ev_a, &ev_b));
        HIP_TRY(hipEventRecord(ev_a, s->stream2));
        if (!PLONKY2_KNOB("PLONKY2_DROP_STREAM2_WAIT"))  // diagnostic build: shows that tests/test_gpu_stream2.py notices the loss
            HIP_TRY(hipStreamWaitEvent(writer, ev_a, 0));
        return ok();
    };
    // The leaf-major copy of a commit is written by the leaf-hashing lanes themselves (merkle.h); PLONKY2_FUSED_LEAVES=0 (diagnostic
    // build) goes back to the separate transposition on stream2.
    static const bool fused_leaves = knob_on(PLONKY2_KNOB("PLONKY2_FUSED_LEAVES"));
    const bool fused = !keccak && d_leaves && fused_leaves;

    uint64_t CHUNK = 16;  // columns per pipeline step: two rate blocks
    if (const char *e = PLONKY2_KNOB("PLONKY2_COMMIT_CHUNK")) {  // diagnostic build: another multiple of 8
        const unsigned long v = strtoul(e, nullptr, 10);
        if (v >= 8 && v <= 1024 && v % 8 == 0) CHUNK = v;
    }

    // Pipelined commit (large commitments): the columns are extended chunk by chunk on the caller's stream while a second,
    // lower-priority stream absorbs the finished chunks into the leaves' sponges (hash_leaves_chunk). The LDE passes are
    // latency-bound and leave half of the vector ALU idle; the hashing is ALU-bound: running them side by
    // side hides most of the LDE. PLONKY2_COMMIT_PIPELINE=0 turns it off (A/B measurements).
    auto pipelined = [&]() -> GlError {
        const size_t n_chunks = (size_t)((poly_num + CHUNK - 1) / CHUNK);
        std::vector<hipEvent_t> *evs;
        HIP_TRY(get_hash_stream(s, &hs, &evs, n_chunks + 2));
        // the hash stream starts behind whatever the caller has queued (the buffers may still be in use by earlier work)
        HIP_TRY(hipEventRecord((*evs)[n_chunks], s->stream));
        HIP_TRY(hipStreamWaitEvent(hs, (*evs)[n_chunks], 0));
        // The reference's caller passes ONE region as coefficients and as leaves (merkle_tree_from_coeffs(values_device,
        // values_device, ..), fri/oracle.rs:409-422): the coefficients [poly_num][n] occupy the slots of the first
        // ceil(poly_num*n / leaf_len) leaf rows, and the LDE of chunk c+1.. still reads them while chunk c is hashed. The
        // hashing lanes therefore leave those rows alone; one transposition of just these rows (1/2^rate_bits of the copy)
        // runs on the hash stream after the last chunk, i.e. behind the last LDE launch.
        uint64_t rows_from = 0;
        if (fused) {
            const uintptr_t c_lo = (uintptr_t)d_coeffs, c_hi = (uintptr_t)(d_coeffs + poly_num * n);
            const uintptr_t l_lo = (uintptr_t)d_leaves, l_hi = (uintptr_t)(d_leaves + (uint64_t)leaf_len * n_ext);
            if (c_lo < l_hi && l_lo < c_hi) {
                const uint64_t past = (uint64_t)(c_hi - l_lo) / 8;  // u64 slots of the leaf region up to the end of the coefficients
                rows_from = std::min<uint64_t>(n_ext, (past + leaf_len - 1) / leaf_len);
            }
            TRY(wait_for_stream2(hs));
        }
        // A launch that starts in the middle of the leaf (c0 != 0) carries only the capacity, so its first block must be a
        // full one: if the last chunk (with the salt columns and a trailing partial block) would be shorter than a rate
        // block, the chunk before it is not absorbed on its own but together with the last.
        const uint64_t last_c0 = (n_chunks - 1) * CHUNK;
        const bool merge_last_two = (leaf_len & 7) && leaf_len - last_c0 < 8;
        uint64_t absorbed = 0;
        for (size_t c = 0; c < n_chunks; c++) {
            const bool last = c + 1 == n_chunks;
            const uint64_t c0 = c * CHUNK, c1 = last ? poly_num : c0 + CHUNK;
            HIP_TRY(coset_lde_batch(*tb, *ct, d_coeffs + c0 * n, d_lde + c0 * n_ext, c1 - c0, n, n_ext, s->stream));
            HIP_TRY(hipEventRecord((*evs)[c], s->stream));
            HIP_TRY(hipStreamWaitEvent(hs, (*evs)[c], 0));
            if (!last && merge_last_two && c + 2 == n_chunks) continue;
            const uint64_t upto = last ? leaf_len : c1;  // the last launch also takes the salt columns (already in d_lde)
            HIP_TRY(hash_leaves_chunk(d_lde, (uint32_t)absorbed, (uint32_t)upto, leaf_len, n_ext, n_ext, cap_height, d_digests, d_cap, hs,
                                      fused ? d_leaves : nullptr, rows_from));
            absorbed = upto;
        }
        if (rows_from) HIP_TRY(transpose_to_leaf_major(d_lde, d_leaves, leaf_len, rows_from, n_ext, hs));
        return beside_leaf_major_copy(fused ? nullptr : d_leaves, [&]() -> GlError {
            HIP_TRY(merkle_tree_layers(d_digests, d_cap, n_ext, cap_height, hs));
            HIP_TRY(hipEventRecord((*evs)[n_chunks + 1], hs));
            HIP_TRY(hipStreamWaitEvent(s->stream, (*evs)[n_chunks + 1], 0));  // the caller's stream continues after the tree
            return ok();
        });
    };

    // The LDE of all columns on the caller's stream, then the tree. Always for Keccak: its leaf kernel is shorter than the LDE
    // (DESIGN.md 3.3.1), so hashing is not what an overlap could hide, and a Keccak sponge cut between launches would have to
    // carry 25 lanes per leaf.
    auto one_shot = [&]() -> GlError {
        HIP_TRY(coset_lde_batch(*tb, *ct, d_coeffs, d_lde, poly_num, n, n_ext, s->stream));
        if (fused) TRY(wait_for_stream2(s->stream));
        return beside_leaf_major_copy(fused ? nullptr : d_leaves, [&]() -> GlError {
            if (keccak)
                HIP_TRY(keccak_merkle_tree(d_lde, 1, n_ext, leaf_len, n_ext, cap_height, d_digests, d_cap, s->stream));
            else
                HIP_TRY(merkle_tree_from_columns(d_lde, leaf_len, n_ext, n_ext, cap_height, d_digests, d_cap, s->stream, fused ? d_leaves : nullptr));
            return ok();
        });
    };

    static const bool commit_pipeline = knob_on(PLONKY2_KNOB("PLONKY2_COMMIT_PIPELINE"));
    const bool pipeline = !keccak && commit_pipeline && poly_num >= 3 * CHUNK && n_ext >= (1ull << 16);
    const GlError r = pipeline ? pipelined() : one_shot();
    if (r.code != 0) {
        if (hs) (void)hipStreamSynchronize(hs);
        if (on_stream2) (void)hipStreamSynchronize(s->stream2);
    }
    return r;
}

}  // namespace plonky2_hip
