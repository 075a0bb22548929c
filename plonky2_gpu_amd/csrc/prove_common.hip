// prove_common.hip — what the provers share behind prove_common.h: the commit of a batch, the host-side hashes of
// gl_circuit_create, the FRI half of a proof and its wire format, and the refusals the handles have in common.
#include <cstdlib>
#include <cstring>

#include "prove_common.h"

namespace plonky2_hip {

GlError hash_no_pad(const uint64_t *in, size_t n, uint64_t out[4], void *ctx) {
    uint64_t st[12] = {0};
    std::vector<uint64_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = in[i] % P;
    const size_t full = n / 8 * 8;
    if (full) TRY(gl_sponge_absorb(st, v.data(), (uint32_t)(full / 8), ctx));
    if (full < n) {  // a short last chunk leaves the old lanes in place
        for (size_t i = full; i < n; i++) st[i - full] = v[i];
        uint64_t block[8];
        memcpy(block, st, sizeof block);
        TRY(gl_sponge_absorb(st, block, 1, ctx));
    }
    memcpy(out, st, 32);
    return ok();
}

void keccak_to_vec(const uint64_t slot[4], uint64_t out[4]) {
    uint8_t b[32];
    memcpy(b, slot, 32);
    for (int c = 0; c < 4; c++) {
        out[c] = 0;
        for (int i = 0; i < (c < 3 ? 7 : 4); i++) out[c] |= (uint64_t)b[7 * c + i] << (8 * i);
    }
}
GlError keccak_hash_no_pad(const std::vector<uint64_t> &in, uint64_t out[4], void *ctx) {
    void *d = nullptr;
    TRY(gl_malloc(&d, (in.size() + 4) * 8));  // the slot first: 16-byte aligned
    uint64_t *p = static_cast<uint64_t *>(d);
    GlError e = gl_memcpy_h2d(p + 4, in.data(), in.size() * 8, ctx);
    if (e.code == 0) e = gl_keccak_hash_no_pad_batch(p + 4, (uint32_t)in.size(), in.size(), 1, p, ctx);
    if (e.code == 0) e = gl_memcpy_d2h(out, p, 32, ctx);
    (void)gl_free(d);
    return e;
}

GlError commit(Batch *b, DevBuf &&polys, bool from_values, uint32_t n_polys, const ProverShape &c, void *ctx, const uint64_t *d_salt, bool fetch_cap) {
    const uint64_t n_ext = 1ull << (c.degree_bits + c.rate_bits);
    const uint32_t salt = d_salt ? SALT_SIZE : 0;
    b->coeffs = std::move(polys);
    b->n_polys = n_polys;
    b->leaf_len = n_polys + salt;
    TRY(b->lde.alloc((uint64_t)b->leaf_len * n_ext));
    TRY(b->digests.alloc(8 * (n_ext - (1ull << c.cap_height))));
    TRY(b->cap_d.alloc(4ull << c.cap_height));
    // the salt columns sit behind the LDE's columns and are hashed with them (gl_commit_from_* reads them as given). They also go into
    // the proof verbatim (fri/prover.rs:203-210), where every word must be canonical like the reference's F::rand_vec output
    // (fri/oracle.rs:998-1002): a caller who fills d_salts with raw 64-bit randoms gets them reduced here, not >= p words on the wire.
    if (salt)
        if (hipError_t e = canon_copy(b->lde.p + (uint64_t)n_polys * n_ext, d_salt, (uint64_t)salt * n_ext, ctx_stream(ctx)); e != hipSuccess)
            return fail(GL_E_INVALID, hipGetErrorString(e));
    if (from_values)
        TRY(gl_commit_from_values_h(c.hasher, b->coeffs.p, n_polys, c.degree_bits, c.rate_bits, c.cap_height, salt, 7, b->lde.p, nullptr, b->digests.p,
                                    b->cap_d.p, ctx));
    else
        TRY(gl_commit_from_coeffs_h(c.hasher, b->coeffs.p, n_polys, c.degree_bits, c.rate_bits, c.cap_height, salt, 7, b->lde.p, nullptr, b->digests.p,
                                    b->cap_d.p, ctx));
    b->cap.resize(4ull << c.cap_height);
    if (!fetch_cap) return ok();  // gl_prove: the transcript reads the cap where it lies; the host copy is fetched with the rest of the proof
    return gl_memcpy_d2h(b->cap.data(), b->cap_d.p, b->cap.size() * 8, ctx);
}

GlError commit_copy(Batch *b, const uint64_t *d_src, uint32_t n_polys, const ProverShape &c, void *ctx, const uint64_t *d_salt) {
    DevBuf w;
    TRY(w.alloc((uint64_t)n_polys << c.degree_bits));
    TRY(gl_memcpy_d2d(w.p, d_src, (8ull * n_polys) << c.degree_bits, ctx));
    return commit(b, std::move(w), true, n_polys, c, ctx, d_salt, false);
}

GlError commit_quotient_chunks(Batch *b, DevBuf &&quotient, uint32_t nch, uint32_t qdf, uint32_t qdb, const ProverShape &c, void *ctx, const uint64_t *d_salt) {
    const uint32_t db = c.degree_bits;
    const uint64_t n = 1ull << db;
    DevBuf chunks;
    if (qdf == (1u << qdb)) {
        chunks = std::move(quotient);  // [nch][n << qdb] read flat is [nch * qdf][n]
    } else {
        TRY(chunks.alloc((uint64_t)nch * qdf * n));
        std::vector<uint64_t> tail((n << qdb) - (uint64_t)qdf * n);
        for (uint32_t k = 0; k < nch; k++) {
            TRY(gl_memcpy_d2h(tail.data(), quotient.p + ((uint64_t)k << (db + qdb)) + (uint64_t)qdf * n, tail.size() * 8, ctx));
            for (uint64_t t : tail)
                if (t) return fail(GL_E_INVALID, "Quotient has failed, the vanishing polynomial is not divisible by Z_H");
            TRY(gl_memcpy_d2d(chunks.p + (uint64_t)k * qdf * n, quotient.p + ((uint64_t)k << (db + qdb)), 8ull * qdf * n, ctx));
        }
    }
    return commit(b, std::move(chunks), false, nch * qdf, c, ctx, d_salt, false);
}

GlError keccak_leaf_error(uint32_t hasher, std::initializer_list<std::pair<const char *, uint32_t>> names_and_leaf_lens, const GlFriParams &fri) {
    if (hasher != GL_HASHER_KECCAK25) return ok();
    for (const auto &cm : names_and_leaf_lens)
        if (cm.second == 4)
            return fail(GL_E_INVALID, std::string("KeccakHash<25> cannot hash a Merkle leaf of 4 elements (plonk/config.rs:56-63) and the leaves of the ") + cm.first +
                        " commitment have 4");
    for (uint32_t li = 0; li < fri.num_reductions; li++)
        if (fri.reduction_arity_bits[li] == 1)
            return fail(GL_E_INVALID, "KeccakHash<25> cannot hash a Merkle leaf of 4 elements (plonk/config.rs:56-63) and FRI reduction " + std::to_string(li) +
                        " has arity_bits = 1: its leaves are 2 extension elements");
    return ok();
}

GlError struct_size_error(const char *name) {
    return fail(GL_E_INVALID, std::string(name) + ".struct_size does not equal sizeof(" + name +
                ") of this library: the caller was compiled against another version of include/plonky2_hip.h");
}

GlError copy_async(void *dst, const void *src, uint64_t bytes, bool to_host, void *ctx) {
    if (!bytes) return ok();
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, ctx_stream(ctx));
    if (e != hipSuccess) return fail(GL_E_INVALID, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    return ok();
}
GlError stream_sync(void *ctx) {
    const hipError_t e = hipStreamSynchronize(ctx_stream(ctx));
    if (e != hipSuccess) return fail(GL_E_INVALID, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return ok();
}

GlError fri_shapes(const ProverShape &c, FriLayout *L) {
    const uint64_t n = 1ull << c.degree_bits;
    L->n_fri = (uint32_t)c.arity_bits.size();
    L->init_layers = c.degree_bits + c.rate_bits - c.cap_height;
    L->fs.resize(L->n_fri);
    uint64_t len = n;
    uint32_t shift = 0;
    for (uint32_t li = 0; li < L->n_fri; li++) {
        const uint32_t ab = c.arity_bits[li];
        L->fs[li].n_leaves = (len << c.rate_bits) >> ab, L->fs[li].leaf_len = 2u << ab;
        if (L->fs[li].n_leaves < (1ull << c.cap_height)) return fail(GL_E_INVALID, "FRI layer smaller than the Merkle cap");
        L->fs[li].layers = glh::log2_ceil(L->fs[li].n_leaves) - c.cap_height;
        shift += ab;
        L->fs[li].shift = shift;
        len >>= ab;
    }
    L->final_len = len;
    return ok();
}

void fri_layout(const ProverShape &c, const std::vector<uint32_t> &leaf_len, SmallData *sd, FriLayout *L) {
    const uint64_t cap_words = 4ull << c.cap_height, nq = c.num_queries;
    L->alpha_fri_s = sd->take(2), L->fri_betas = sd->take(2ull * L->n_fri), L->pow_w = sd->take(1), L->resp_idx = sd->take(1 + nq);
    L->fri_caps = sd->take(cap_words * L->n_fri), L->final_s = sd->take(2 * L->final_len);
    for (uint32_t ll : leaf_len) L->q_leaves.push_back(sd->take(nq * ll)), L->q_sib.push_back(sd->take(nq * L->init_layers * 4));
    for (uint32_t li = 0; li < L->n_fri; li++)
        L->s_leaves.push_back(sd->take(nq * L->fs[li].leaf_len)), L->s_sib.push_back(sd->take(nq * L->fs[li].layers * 4));
}

GlError fri_prove(const ProverShape &c, const FriLayout &L, ProofSession &s, const Span &T, const std::vector<const Batch *> &oracles,
                  const std::vector<GlObserveSrc> &opening_srcs, const std::vector<FriBatch> &batches, uint64_t *pow_witness) {
    const uint64_t n = 1ull << c.degree_bits, n_ext = n << c.rate_bits, cap_words = 4ull << c.cap_height;
    const uint32_t n_fri = L.n_fri, nq = c.num_queries;
    const std::vector<FriShape> &fs = L.fs;
    uint64_t *const D = s.D, *const H = s.H;
    void *const ctx = s.ctx;
    TRY(s.step(T, opening_srcs, 2, L.alpha_fri_s));
    TRY(s.fetch(L.alpha_fri_s));
    TRY(s.sync());
    const E2 alpha{H[L.alpha_fri_s.off], H[L.alpha_fri_s.off + 1]};
    DevBuf final_poly;  // planar [2][n]
    TRY(final_poly.alloc(2 * n));
    {
        std::vector<const uint64_t *> ptrs;
        for (const FriBatch &b : batches) ptrs.insert(ptrs.end(), b.polys.begin(), b.polys.end());
        DevBuf d_ptrs, comp;
        TRY(d_ptrs.alloc(ptrs.size()));
        TRY(gl_memcpy_h2d(d_ptrs.p, ptrs.data(), ptrs.size() * 8, ctx));
        TRY(comp.alloc(2 * n));
        const uint64_t al[2] = {alpha.a, alpha.b};
        uint64_t off = 0;
        for (size_t b = 0; b < batches.size(); b++) {
            const uint32_t m = (uint32_t)batches[b].polys.size();
            TRY(gl_fri_reduce_polys_base(reinterpret_cast<const uint64_t *const *>(d_ptrs.p) + off, m, n, al, comp.p, ctx));
            const E2 sc = e2_pow(alpha, m);  // alpha.shift_poly (util/reducing.rs:103-106)
            const uint64_t pt[2] = {batches[b].point.a, batches[b].point.b}, scale[2] = {sc.a, sc.b};
            TRY(gl_fri_divide_by_linear(comp.p, n, pt, scale, b != 0, final_poly.p, ctx));
            off += m;
        }
        // d_ptrs / comp return to the pool here while their kernels may still be queued: stream order
    }
    TRY(s.st.mark(6));
    // ---- fri_committed_trees (fri/prover.rs:77-120): no host synchronisation inside — the betas stay on the device ----
    struct Layer {
        DevBuf rows, digests, cap_d;
    };
    std::vector<Layer> layers(n_fri);
    DevBuf final_coeffs_d;
    {
        DevBuf coeffs = std::move(final_poly), vals;
        uint64_t len = n, shift = 7;
        auto lde = [&](DevBuf *dst) -> GlError {
            const uint32_t lg = glh::log2_ceil(len);
            TRY(dst->alloc(2 * (len << c.rate_bits)));
            return gl_coset_lde_batch(coeffs.p, dst->p, 2, lg, c.rate_bits, shift, len, len << c.rate_bits, ctx);
        };
        if (!layers.empty()) TRY(lde(&vals));
        for (uint32_t li = 0; li < n_fri; li++) {
            const uint32_t ab = c.arity_bits[li];
            const uint64_t lde_len = len << c.rate_bits;
            Layer &Ly = layers[li];
            TRY(Ly.rows.alloc(2 * lde_len));
            TRY(gl_ext2_interleave(vals.p, lde_len, Ly.rows.p, ctx));
            TRY(Ly.digests.alloc(8 * (fs[li].n_leaves - (1ull << c.cap_height)) + 4));
            TRY(Ly.cap_d.alloc(cap_words));
            TRY(gl_merkle_tree_from_leaves_h(c.hasher, Ly.rows.p, fs[li].leaf_len, fs[li].n_leaves, c.cap_height, Ly.digests.p, Ly.cap_d.p, ctx));
            TRY(gl_memcpy_d2d(D + L.fri_caps.off + li * cap_words, Ly.cap_d.p, cap_words * 8, ctx));
            TRY(s.step(T, {c.hashes(Ly.cap_d.p, cap_words)}, 2, Span{L.fri_betas.off + 2ull * li, 2}));
            DevBuf next;
            TRY(next.alloc(2 * (len >> ab)));
            TRY(gl_fri_fold_device(coeffs.p, len, ab, D + L.fri_betas.off + 2ull * li, next.p, ctx));
            coeffs = std::move(next);  // the old coefficients return to the pool (stream order keeps them valid)
            len >>= ab;
            shift = glh::pow(shift, 1ull << ab);
            if (li + 1 < n_fri) TRY(lde(&vals));
        }
        // observe_extension_elements(final_poly.coeffs) (fri/prover.rs:117): the two planes read interleaved
        TRY(s.step(T, {GlObserveSrc{coeffs.p, 2 * len, len}}, 0, Span{}));
        final_coeffs_d = std::move(coeffs);
    }
    TRY(s.st.mark(7));
    // ---- fri_proof_of_work (fri/prover.rs:122-171) ----
    *pow_witness = 0;
    TRY(gl_fri_proof_of_work_device(D + T.off, c.pow_bits, D + L.pow_w.off, pow_witness, ctx));  // F::order() has 64 bits: leading zeros of the u64 response
    // observe the witness, draw the response, then the query indices (fri/prover.rs:163-170, 181-190)
    TRY(s.step(T, {GlObserveSrc{D + L.pow_w.off, 1, 0}}, 1 + nq, L.resp_idx));
    TRY(s.st.mark(8));
    // ---- fri_prover_query_rounds (fri/prover.rs:173-260): the indices never leave the device ----
    const uint64_t *d_idx = D + L.resp_idx.off + 1;
    for (size_t o = 0; o < oracles.size(); o++)  // salted leaves go into the proof whole (fri/prover.rs:203-210)
        TRY(gl_merkle_open_batch_device(oracles[o]->lde.p, 1, n_ext, oracles[o]->leaf_len, n_ext, c.cap_height, oracles[o]->digests.p, d_idx, nq, 0,
                                        D + L.q_leaves[o].off, D + L.q_sib[o].off, ctx));
    for (uint32_t li = 0; li < n_fri; li++)
        TRY(gl_merkle_open_batch_device(layers[li].rows.p, fs[li].leaf_len, 1, fs[li].leaf_len, fs[li].n_leaves, c.cap_height, layers[li].digests.p,
                                        d_idx, nq, fs[li].shift, D + L.s_leaves[li].off, D + L.s_sib[li].off, ctx));
    return gl_memcpy_d2d(D + L.final_s.off, final_coeffs_d.p, 2 * L.final_len * 8, ctx);
}

GlError fri_check_pow(const ProverShape &c, const FriLayout &L, const uint64_t *H, uint64_t pow_witness) {
    if (c.pow_bits && (H[L.resp_idx.off] >> (64 - c.pow_bits)) != 0) return fail(GL_E_INVALID, "proof-of-work response does not have the required leading zeros");
    if (H[L.pow_w.off] != pow_witness) return fail(GL_E_INVALID, "proof-of-work witness changed between the search and the transcript");
    return ok();
}

void fri_write(Bytes &out, const ProverShape &c, const FriLayout &L, const uint64_t *H, const std::vector<const Batch *> &oracles, uint64_t pow_witness) {
    const uint64_t cap_words = 4ull << c.cap_height;
    for (uint32_t li = 0; li < L.n_fri; li++) out.hashes(H + L.fri_caps.off + li * cap_words, cap_words / 4);
    for (uint32_t q = 0; q < c.num_queries; q++) {
        for (size_t o = 0; o < oracles.size(); o++) {
            const uint32_t ll = oracles[o]->leaf_len;
            out.fields(H + L.q_leaves[o].off + (uint64_t)q * ll, ll);
            out.merkle_proof(H + L.q_sib[o].off + (uint64_t)q * L.init_layers * 4, L.init_layers);
        }
        for (uint32_t li = 0; li < L.n_fri; li++) {
            out.fields(H + L.s_leaves[li].off + (uint64_t)q * L.fs[li].leaf_len, L.fs[li].leaf_len);
            out.merkle_proof(H + L.s_sib[li].off + (uint64_t)q * L.fs[li].layers * 4, L.fs[li].layers);
        }
    }
    for (uint64_t i = 0; i < L.final_len; i++) out.field(H[L.final_s.off + i]), out.field(H[L.final_s.off + L.final_len + i]);  // interleaved (a_i, b_i)
    out.field(pow_witness);
}

GlError bytes_out(const Bytes &out, uint8_t **proof, uint64_t *proof_len) {
    uint8_t *buf = static_cast<uint8_t *>(malloc(out.v.size() ? out.v.size() : 1));
    if (!buf) return fail(GL_E_INVALID, "out of memory");
    memcpy(buf, out.v.data(), out.v.size());
    *proof = buf;
    *proof_len = out.v.size();
    return ok();
}

}  // namespace plonky2_hip
