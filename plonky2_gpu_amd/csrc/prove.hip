// prove.hip — the provers' HOST logic in native code: gl_circuit_create / gl_prove, and gl_stark_create / gl_stark_prove (starky's
// prove(), at the end of this file) over the same commitments, transcript and FRI half.
//
// prove() (plonky2/src/plonk/prover.rs:40-233) from the full witness on, with PolynomialBatch::prove_openings
// (plonky2/src/fri/oracle.rs:1047-1112), fri_proof (plonky2/src/fri/prover.rs:24-260), the Challenger
// (plonky2/src/iop/challenger.rs) and the proof wire format (plonky2/src/util/serialization.rs:466-700).
// Everything data-parallel is a kernel behind the gl_* entry points of this library; what lives here is
// the serial glue a Rust host would otherwise write against those entry points — the transcript's
// buffers, challenge arithmetic on single field elements, buffer management, serialisation — so that a
// host in any language needs exactly two calls. No polynomial, LDE, tree or witness column is touched
// by the CPU; the transcript lives on the device (gl_challenger_step): its sponge state, input buffer and challenges.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/plonky2_hip.h"
#include "commit.h"
#include "gate_jit.h"
#include "gl_field.h"
#include "jit.h"
#include "stark.h"
#include "stark_jit.h"
#include "stark_split.h"

using namespace plonky2_hip;

namespace {

using glh::P;

struct E2 {  // a + bX, X^2 = 7 (field/src/goldilocks_extensions.rs:13-26)
    uint64_t a, b;
};
E2 e2_mul(E2 x, E2 y) {
    return E2{glh::add(glh::mul(x.a, y.a), glh::mul(7, glh::mul(x.b, y.b))), glh::add(glh::mul(x.a, y.b), glh::mul(x.b, y.a))};
}
E2 e2_pow(E2 x, uint64_t e) {
    E2 acc{1, 0};
    while (e) {
        if (e & 1) acc = e2_mul(acc, x);
        x = e2_mul(x, x);
        e >>= 1;
    }
    return acc;
}

// Device buffers of one circuit's proofs are recycled: every proof of a circuit allocates the same ~50
// sizes, hipMalloc/hipFree of multi-GiB buffers cost milliseconds and hipFree synchronises the device.
// Handing a buffer back while kernels that use it are still in flight is safe here because everything
// gl_prove launches is ordered on ONE stream: the next user's kernels queue behind them. That argument
// holds per CONTEXT, so a circuit keeps one pool per context that proves with it (two proofs of one
// circuit in flight on two contexts never hand each other a buffer whose kernels are still queued).
struct Pool {
    std::mutex m;
    std::multimap<uint64_t, uint64_t *> free_;  // bytes -> buffer
    // page-locked host staging of this context's proofs: what the host sends (circuit digest, public inputs) and everything it
    // fetches (challenges, caps, openings, query answers) goes through it, so that the copies are truly asynchronous
    uint64_t *pinned = nullptr;
    uint64_t pinned_words = 0;
    ~Pool() {
        for (auto &kv : free_) (void)gl_free(kv.second);
        if (pinned) (void)gl_free_host(pinned);
    }
    GlError staging(uint64_t words, uint64_t **out) {
        if (pinned_words < words) {
            if (pinned) (void)gl_free_host(pinned);
            pinned = nullptr, pinned_words = 0;
            void *q = nullptr;
            GlError e = gl_malloc_host(&q, words * 8);
            if (e.code != 0) return e;
            pinned = static_cast<uint64_t *>(q), pinned_words = words;
        }
        *out = pinned;
        return GlError{0, nullptr};
    }
    uint64_t *get(uint64_t bytes) {
        std::lock_guard<std::mutex> lock(m);
        auto it = free_.find(bytes);
        if (it == free_.end()) return nullptr;
        uint64_t *p = it->second;
        free_.erase(it);
        return p;
    }
    void put(uint64_t bytes, uint64_t *p) {
        std::lock_guard<std::mutex> lock(m);
        free_.emplace(bytes, p);
    }
};
thread_local Pool *g_pool = nullptr;  // installed by gl_prove for its duration; null = plain gl_malloc / gl_free
struct PoolScope {
    Pool *prev;
    explicit PoolScope(Pool *p) : prev(g_pool) { g_pool = p; }
    ~PoolScope() { g_pool = prev; }
};

struct DevBuf {  // RAII device buffer of u64
    uint64_t *p = nullptr;
    uint64_t n = 0, bytes = 0;
    Pool *pool = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n), bytes(o.bytes), pool(o.pool) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        reset();
        p = o.p, n = o.n, bytes = o.bytes, pool = o.pool, o.p = nullptr;
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) {
            if (pool)
                pool->put(bytes, p);
            else
                (void)gl_free(p);
        }
        p = nullptr;
    }
    GlError alloc(uint64_t elems) {
        reset();
        n = elems;
        bytes = (elems ? elems : 1) * 8;
        pool = g_pool;
        if (pool && (p = pool->get(bytes))) return ok();
        void *q = nullptr;
        TRY(gl_malloc(&q, bytes));
        p = static_cast<uint64_t *>(q);
        return ok();
    }
};

// A committed batch resident in HBM (PolynomialBatch, fri/oracle.rs:112-120), without a leaf-major copy.
struct Batch {
    DevBuf coeffs, lde, digests, cap_d;
    uint32_t n_polys = 0;
    uint32_t leaf_len = 0;  // n_polys + the salt of a blinded commitment (fri/oracle.rs:985-1002)
    std::vector<uint64_t> cap;  // host copy, 4 << cap_height
};

// ---- transcript: device-resident (gl_challenger_step), see prove_impl; gl_circuit_create hashes a few host words once ----
GlError hash_no_pad(const uint64_t *in, size_t n, uint64_t out[4], void *ctx) {  // hash/hashing.rs:81-108
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

// BytesHash<25>::to_vec (hash/hash_types.rs:179-189) of one digest slot: chunks of 7, 7, 7 and 4 bytes, little endian
void keccak_to_vec(const uint64_t slot[4], uint64_t out[4]) {
    uint8_t b[32];
    memcpy(b, slot, 32);
    for (int c = 0; c < 4; c++) {
        out[c] = 0;
        for (int i = 0; i < (c < 3 ? 7 : 4); i++) out[c] |= (uint64_t)b[7 * c + i] << (8 * i);
    }
}
// KeccakHash<25>::hash_no_pad of a few host words, on the device (gl_keccak_hash_no_pad_batch); out = one digest slot
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

// ---- what the commitments, the transcript and the FRI half of a proof need to know: shared by circuits and STARKs --------------
struct ProverShape {
    uint32_t degree_bits = 0, rate_bits = 0, cap_height = 0, pow_bits = 0, num_queries = 0;
    bool hiding = false;  // FriParams::hiding
    uint32_t hasher = GL_HASHER_POSEIDON;  // GenericConfig::Hasher: builds every Merkle tree; the Challenger stays Poseidon (plonk/config.rs:110-128)
    bool keccak() const { return hasher == GL_HASHER_KECCAK25; }
    // how the transcript reads a hash of this prover's trees: four field elements either way — a Poseidon HashOut as it lies, a
    // Keccak digest slot through BytesHash<25>::to_vec (merkle.hip keccak_digest_chunk)
    GlObserveSrc hashes(const uint64_t *d_slots, uint64_t words) const { return GlObserveSrc{d_slots, words, keccak() ? GL_OBSERVE_KECCAK_DIGESTS : 0}; }
    std::vector<uint32_t> arity_bits;
    mutable std::mutex pools_m;
    mutable std::map<void *, Pool> pools;  // context -> the working buffers of this handle's proofs there, recycled from proof to proof
    Pool *pool_of(void *ctx) const {
        std::lock_guard<std::mutex> lock(pools_m);
        return &pools[ctx];  // std::map: the address is stable
    }
    void set_fri(const GlFriParams &f) {
        rate_bits = f.rate_bits, cap_height = f.cap_height, pow_bits = f.proof_of_work_bits, num_queries = f.num_query_rounds;
        hiding = f.hiding != 0;
        arity_bits.assign(f.reduction_arity_bits, f.reduction_arity_bits + f.num_reductions);
    }
    GlError trim() {
        std::lock_guard<std::mutex> all(pools_m);
        for (auto &cp : pools) {
            Pool &pool = cp.second;
            std::lock_guard<std::mutex> lock(pool.m);
            for (auto &kv : pool.free_) TRY(gl_free(kv.second));
            pool.free_.clear();
        }
        return ok();
    }
};

// ---- the circuit object ---------------------------------------------------------------------------
struct Circuit : ProverShape {
    uint32_t num_wires, num_routed, num_constants, num_challenges, qdf, num_gate_constraints;
    uint64_t digest[4];  // HashOut, or one Keccak digest slot
    DevBuf k_is, sigmas;
    Batch cs;  // constants_sigmas_commitment
    // gates
    DevBuf d_instrs, d_gates, d_imms;
    uint32_t num_gates = 0, num_selectors = 0;
    void *gate_kernel = nullptr;
    ~Circuit() {
        if (gate_kernel) gl_gate_kernel_destroy(gate_kernel);
    }
};

uint32_t num_partial_products(uint32_t routed, uint32_t qdf) { return (routed + qdf - 1) / qdf - 1; }

constexpr uint32_t SALT_SIZE = 4;  // fri/oracle.rs:41

// d_salt: SALT_SIZE columns of n_ext caller-provided random elements in leaf order (a blinded commitment, prover.rs:84, 125, 174), or null
GlError commit(Batch *b, DevBuf &&polys, bool from_values, uint32_t n_polys, const ProverShape &c, void *ctx, const uint64_t *d_salt = nullptr,
              bool fetch_cap = true) {
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

struct Bytes {  // util/serialization.rs:466-560
    std::vector<uint8_t> v;
    void u8(uint8_t x) { v.push_back(x); }
    void field(uint64_t x) {
        x %= P;
        for (int i = 0; i < 8; i++) v.push_back((uint8_t)(x >> (8 * i)));
    }
    void fields(const uint64_t *p, size_t n) {
        for (size_t i = 0; i < n; i++) field(p[i]);
    }
    void fields(const std::vector<uint64_t> &a) { fields(a.data(), a.size()); }
    bool keccak = false;
    // write_hash (:537-543) of `count` hashes in their 4-word slots: GenericHashOut::to_bytes — the four elements of a HashOut, or the
    // first 25 bytes of a Keccak digest slot
    void hashes(const uint64_t *slots, uint64_t count) {
        if (!keccak) return fields(slots, 4 * count);
        for (uint64_t h = 0; h < count; h++)
            for (int i = 0; i < 25; i++) v.push_back((uint8_t)(slots[4 * h + (i >> 3)] >> (8 * (i & 7))));
    }
    void merkle_proof(const uint64_t *sib, uint32_t layers) {  // :573-589
        u8((uint8_t)layers);
        hashes(sib, layers);
    }
};

struct Stages {
    double *ms;
    void *ctx;
    std::chrono::steady_clock::time_point t;
    Stages(double *m, void *c) : ms(m), ctx(c), t(std::chrono::steady_clock::now()) {}
    GlError mark(int i) {
        if (!ms) return ok();
        TRY(gl_ctx_synchronize(ctx));
        auto now = std::chrono::steady_clock::now();
        ms[i] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return ok();
    }
};

// Asynchronous copies between device memory and the pool's page-locked staging, on the context's first stream.
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


// ---- the FRI half of a proof: PolynomialBatch::prove_openings (fri/oracle.rs:1047-1112) over fri_proof (fri/prover.rs:24-260) ----
// What a prover brings: its committed oracles, the two opening batches of its FriInstanceInfo as lists of coefficient columns,
// the openings where gl_eval_polys_ext2 left them (observed as to_fri_openings orders them), and the transcript T. Everything small
// lives in the prover's one device buffer D with its page-locked mirror H; the spans of this half are taken by fri_layout.
struct Span {
    uint64_t off = 0, words = 0;
};
struct SmallData {
    uint64_t top = 0;
    Span take(uint64_t words) {
        Span sp{top, words};
        top += (words + 1) & ~1ull;  // 16-byte granules
        return sp;
    }
};
struct FriShape {
    uint64_t n_leaves;
    uint32_t leaf_len, layers, shift;
};
struct FriLayout {
    std::vector<FriShape> fs;
    uint64_t final_len = 0;
    uint32_t n_fri = 0, init_layers = 0;
    Span alpha_fri_s, fri_betas, pow_w, resp_idx, fri_caps, final_s;
    std::vector<Span> q_leaves, q_sib, s_leaves, s_sib;
};
struct FriBatch {  // FriBatchInfo: the polynomials opened at one point
    E2 point;
    std::vector<const uint64_t *> polys;  // device coefficient columns of length n
};

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

// after fri_shapes; leaf_len: of every oracle, salt included
void fri_layout(const ProverShape &c, const std::vector<uint32_t> &leaf_len, SmallData *sd, FriLayout *L) {
    const uint64_t cap_words = 4ull << c.cap_height, nq = c.num_queries;
    L->alpha_fri_s = sd->take(2), L->fri_betas = sd->take(2ull * L->n_fri), L->pow_w = sd->take(1), L->resp_idx = sd->take(1 + nq);
    L->fri_caps = sd->take(cap_words * L->n_fri), L->final_s = sd->take(2 * L->final_len);
    for (uint32_t ll : leaf_len) L->q_leaves.push_back(sd->take(nq * ll)), L->q_sib.push_back(sd->take(nq * L->init_layers * 4));
    for (uint32_t li = 0; li < L->n_fri; li++)
        L->s_leaves.push_back(sd->take(nq * L->fs[li].leaf_len)), L->s_sib.push_back(sd->take(nq * L->fs[li].layers * 4));
}

// From the FRI alpha to the query openings; marks stages 6 (combine), 7 (commit phase), 8 (proof of work). The caller fetches
// everything, synchronises, marks stage 9 and calls fri_check_pow / fri_write.
GlError fri_prove(const ProverShape &c, const FriLayout &L, uint64_t *D, uint64_t *H, const Span &T, const std::vector<const Batch *> &oracles,
                  const std::vector<GlObserveSrc> &opening_srcs, const std::vector<FriBatch> &batches, Stages &st, uint64_t *pow_witness, void *ctx) {
    const uint64_t n = 1ull << c.degree_bits, n_ext = n << c.rate_bits, cap_words = 4ull << c.cap_height;
    const uint32_t n_fri = L.n_fri, nq = c.num_queries;
    const std::vector<FriShape> &fs = L.fs;
    auto step = [&](std::initializer_list<GlObserveSrc> srcs, uint32_t n_out, const Span &out) {
        return gl_challenger_step(D + T.off, srcs.begin(), (uint32_t)srcs.size(), n_out, n_out ? D + out.off : nullptr, 0, ctx);
    };
    TRY(gl_challenger_step(D + T.off, opening_srcs.data(), (uint32_t)opening_srcs.size(), 2, D + L.alpha_fri_s.off, 0, ctx));
    TRY(copy_async(H + L.alpha_fri_s.off, D + L.alpha_fri_s.off, L.alpha_fri_s.words * 8, true, ctx));
    TRY(stream_sync(ctx));
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
    TRY(st.mark(6));
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
            TRY(step({c.hashes(Ly.cap_d.p, cap_words)}, 2, Span{L.fri_betas.off + 2ull * li, 2}));
            DevBuf next;
            TRY(next.alloc(2 * (len >> ab)));
            TRY(gl_fri_fold_device(coeffs.p, len, ab, D + L.fri_betas.off + 2ull * li, next.p, ctx));
            coeffs = std::move(next);  // the old coefficients return to the pool (stream order keeps them valid)
            len >>= ab;
            shift = glh::pow(shift, 1ull << ab);
            if (li + 1 < n_fri) TRY(lde(&vals));
        }
        // observe_extension_elements(final_poly.coeffs) (fri/prover.rs:117): the two planes read interleaved
        TRY(step({GlObserveSrc{coeffs.p, 2 * len, len}}, 0, Span{}));
        final_coeffs_d = std::move(coeffs);
    }
    TRY(st.mark(7));
    // ---- fri_proof_of_work (fri/prover.rs:122-171) ----
    *pow_witness = 0;
    TRY(gl_fri_proof_of_work_device(D + T.off, c.pow_bits, D + L.pow_w.off, pow_witness, ctx));  // F::order() has 64 bits: leading zeros of the u64 response
    // observe the witness, draw the response, then the query indices (fri/prover.rs:163-170, 181-190)
    TRY(step({GlObserveSrc{D + L.pow_w.off, 1, 0}}, 1 + nq, L.resp_idx));
    TRY(st.mark(8));
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

// write_fri_proof (util/serialization.rs:591-639)
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

}  // namespace

extern "C" {

static GlError circuit_create(uint32_t hasher, const GlCircuitDesc *d, void **circuit, void *ctx) {
    if (!d || !circuit || !ctx || !d->h_k_is || !d->h_constants || !d->h_sigmas || (d->fri.num_reductions && !d->fri.reduction_arity_bits))
        return fail(GL_E_INVALID, "null pointer");
    if (d->struct_size != sizeof(GlCircuitDesc))
        return fail(GL_E_INVALID, "GlCircuitDesc.struct_size does not equal sizeof(GlCircuitDesc) of this library: the caller was compiled against another version of include/plonky2_hip.h");
    if (d->degree_bits > 24 || d->num_challenges == 0 || d->num_challenges > 4 || d->num_routed_wires > d->num_wires ||
        d->quotient_degree_factor < 2 || d->quotient_degree_factor >= d->num_routed_wires)
        return fail(GL_E_INVALID, "bad circuit shape (the prover needs quotient_degree_factor < num_routed_wires, prover.rs:99-102)");
    if (hasher == GL_HASHER_KECCAK25) {
        // KeccakHash<25>::hash_or_noop panics on a leaf of exactly four elements (a 32-byte slice of a 25-byte vector, plonk/config.rs:
        // 56-63): refuse such a circuit here, before anything is allocated, not in the middle of a proof
        const uint32_t salt = d->fri.hiding ? SALT_SIZE : 0, nch = d->num_challenges, qdf = d->quotient_degree_factor;
        const struct {
            const char *name;
            uint32_t leaf_len;
        } commitments[4] = {{"constants / sigmas", d->num_constants + d->num_routed_wires},
                            {"wires", d->num_wires + salt},
                            {"Zs / partial products", nch * (1 + num_partial_products(d->num_routed_wires, qdf)) + salt},
                            {"quotient", nch * qdf + salt}};
        for (const auto &cm : commitments)
            if (cm.leaf_len == 4)
                return fail(GL_E_INVALID, std::string("KeccakHash<25> cannot hash a Merkle leaf of 4 elements (plonk/config.rs:56-63) and the leaves of the ") + cm.name +
                            " commitment have 4");
        for (uint32_t li = 0; li < d->fri.num_reductions; li++)
            if (d->fri.reduction_arity_bits[li] == 1)
                return fail(GL_E_INVALID, "KeccakHash<25> cannot hash a Merkle leaf of 4 elements (plonk/config.rs:56-63) and FRI reduction " + std::to_string(li) +
                            " has arity_bits = 1: its leaves are 2 extension elements");
    }
    Circuit *c = new Circuit();
    c->hasher = hasher;
    c->degree_bits = d->degree_bits, c->num_wires = d->num_wires, c->num_routed = d->num_routed_wires;
    c->num_constants = d->num_constants, c->num_challenges = d->num_challenges, c->qdf = d->quotient_degree_factor;
    c->num_gate_constraints = d->num_gate_constraints;
    c->set_fri(d->fri);
    const uint64_t n = 1ull << c->degree_bits;
    auto bail = [&](GlError e) {
        delete c;
        return e;
    };
#define CTRY(expr)                         \
    do {                                   \
        GlError _e = (expr);               \
        if (_e.code != 0) return bail(_e); \
    } while (0)
    CTRY(c->k_is.alloc(c->num_routed));
    CTRY(gl_memcpy_h2d(c->k_is.p, d->h_k_is, 8ull * c->num_routed, ctx));
    CTRY(c->sigmas.alloc((uint64_t)c->num_routed * n));
    CTRY(gl_memcpy_h2d(c->sigmas.p, d->h_sigmas, 8ull * c->num_routed * n, ctx));
    // constants_sigmas_commitment (circuit_builder.rs:861-873): constants then sigmas, from values
    DevBuf csv;
    CTRY(csv.alloc((uint64_t)(c->num_constants + c->num_routed) * n));
    CTRY(gl_memcpy_h2d(csv.p, d->h_constants, 8ull * c->num_constants * n, ctx));
    CTRY(gl_memcpy_h2d(csv.p + (uint64_t)c->num_constants * n, d->h_sigmas, 8ull * c->num_routed * n, ctx));
    CTRY(commit(&c->cs, std::move(csv), true, c->num_constants + c->num_routed, *c, ctx));
    if (d->h_circuit_digest) {
        memcpy(c->digest, d->h_circuit_digest, 32);
    } else if (c->keccak()) {
        // the same with C::Hasher = KeccakHash<25>: cap.flatten() and the separator's hash enter as to_vec(), four elements per hash
        const std::vector<uint64_t> pad = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
        uint64_t dsd[4];
        CTRY(keccak_hash_no_pad(pad, dsd, ctx));
        std::vector<uint64_t> parts(c->cs.cap.size() + 5);
        for (size_t h = 0; h < c->cs.cap.size() / 4; h++) keccak_to_vec(c->cs.cap.data() + 4 * h, parts.data() + 4 * h);
        keccak_to_vec(dsd, parts.data() + c->cs.cap.size());
        parts.back() = c->degree_bits;
        CTRY(keccak_hash_no_pad(parts, c->digest, ctx));
    } else {
        // circuit_builder.rs:915-927: hash_no_pad(cap || hash_pad(domain separator = []) || degree_bits)
        uint64_t pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, dsd[4];
        CTRY(hash_no_pad(pad, 12, dsd, ctx));
        std::vector<uint64_t> parts(c->cs.cap);
        parts.insert(parts.end(), dsd, dsd + 4);
        parts.push_back(c->degree_bits);
        CTRY(hash_no_pad(parts.data(), parts.size(), c->digest, ctx));
    }
    if (d->num_gates) {
        if (!d->h_instrs || !d->h_gates) return bail(fail(GL_E_INVALID, "null gate program"));
        c->num_gates = d->num_gates, c->num_selectors = d->num_selectors;
        {
            std::string verr;
            uint32_t wires_needed = 0, constants_needed = 0;
            if (!plonky2_hip::gate_programs_validate(reinterpret_cast<const uint16_t *>(d->h_instrs), d->num_instrs, reinterpret_cast<const uint32_t *>(d->h_gates),
                                        d->num_gates, d->num_immediates, d->num_selectors, d->num_gate_constraints, &wires_needed,
                                        &constants_needed, &verr))
                return bail(fail(GL_E_INVALID, "gate programs: " + verr));
            if (wires_needed > c->num_wires || constants_needed > c->num_constants)
                return bail(fail(GL_E_INVALID, "gate programs load wire " + std::to_string(wires_needed ? wires_needed - 1 : 0) + " / constant column " +
                                 std::to_string(constants_needed ? constants_needed - 1 : 0) + " but the circuit has " + std::to_string(c->num_wires) +
                                 " wires and " + std::to_string(c->num_constants) + " constants"));
        }
        if (d->compile_gates) {
            CTRY(gl_gate_kernel_build(d->h_instrs, d->num_instrs, d->h_gates, d->num_gates, d->h_immediates, d->num_immediates,
                                      d->num_selectors, d->num_gate_constraints, d->num_challenges, &c->gate_kernel));
        } else {
            CTRY(c->d_instrs.alloc(d->num_instrs ? d->num_instrs : 1));  // 8 bytes per GlGateInstr
            CTRY(gl_memcpy_h2d(c->d_instrs.p, d->h_instrs, 8ull * d->num_instrs, ctx));
            CTRY(c->d_gates.alloc(3ull * d->num_gates));  // 24 bytes per GlGateDesc
            CTRY(gl_memcpy_h2d(c->d_gates.p, d->h_gates, 24ull * d->num_gates, ctx));
            if (d->num_immediates) {
                CTRY(c->d_imms.alloc(d->num_immediates));
                CTRY(gl_memcpy_h2d(c->d_imms.p, d->h_immediates, 8ull * d->num_immediates, ctx));
            }
        }
    }
    CTRY(gl_ctx_synchronize(ctx));
#undef CTRY
    *circuit = c;
    return ok();
}

GlError gl_circuit_create(const GlCircuitDesc *d, void **circuit, void *ctx) { return circuit_create(GL_HASHER_POSEIDON, d, circuit, ctx); }

GlError gl_circuit_create_h(uint32_t hasher, const GlCircuitDesc *d, void **circuit, void *ctx) {
    if (hasher == GL_HASHER_POSEIDON) return gl_circuit_create(d, circuit, ctx);
    if (hasher != GL_HASHER_KECCAK25) return fail(GL_E_INVALID, "unknown hasher");
    return circuit_create(hasher, d, circuit, ctx);
}

void gl_circuit_destroy(void *circuit) { delete static_cast<Circuit *>(circuit); }

GlError gl_circuit_trim(void *circuit) {
    if (!circuit) return fail(GL_E_INVALID, "null pointer");
    return static_cast<Circuit *>(circuit)->trim();
}

GlError gl_circuit_info(const void *circuit, uint64_t h_digest[4], uint64_t *h_constants_sigmas_cap) {
    if (!circuit) return fail(GL_E_INVALID, "null pointer");
    const Circuit *c = static_cast<const Circuit *>(circuit);
    if (h_digest) memcpy(h_digest, c->digest, 32);
    if (h_constants_sigmas_cap) memcpy(h_constants_sigmas_cap, c->cs.cap.data(), c->cs.cap.size() * 8);
    return ok();
}

void gl_bytes_free(uint8_t *p) { free(p); }

// The transcript of a proof lives on the device (gl_challenger_step): every observation reads its source where the producing kernel
// left it (caps, openings, the final polynomial, the proof-of-work witness), the FRI betas, the query indices and the proof-of-work
// state are consumed there, and the host fetches exactly the challenges it computes with — betas / gammas (with the public-inputs
// hash), alphas, zeta, the FRI alpha — one small copy and one stream synchronisation each, then the proof-of-work witness, then
// everything that goes into the proof bytes in one go. Round 5 paid a host round trip per Challenger call (sixteen per proof, each
// an upload, a launch, a download and a synchronisation) and one per cap, opening batch and query batch.
static GlError prove_impl(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                          const uint64_t *d_salts, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx) {
    if (!circuit || !d_wires || !proof || !proof_len || !ctx || (num_public_inputs && !h_public_inputs)) return fail(GL_E_INVALID, "null pointer");
    const Circuit &c = *static_cast<const Circuit *>(circuit);
    if (c.hiding && !d_salts) return fail(GL_E_INVALID, "the circuit's FRI parameters are hiding (zero_knowledge): prove it with gl_prove_zk and salt columns");
    if (!c.hiding && d_salts) return fail(GL_E_INVALID, "gl_prove_zk on a circuit whose FRI parameters are not hiding");
    Pool *pool = c.pool_of(ctx);
    PoolScope pool_scope(pool);  // every DevBuf below comes from / returns to the circuit's pool of this context
    const uint32_t db = c.degree_bits, nch = c.num_challenges, qdf = c.qdf, npi = num_public_inputs;
    const uint64_t n = 1ull << db, n_ext = n << c.rate_bits, cap_words = 4ull << c.cap_height;
    const uint32_t npp = num_partial_products(c.num_routed, qdf);
    if (h_stage_ms) memset(h_stage_ms, 0, sizeof(double) * GL_PROVE_STAGES);
    Stages st(h_stage_ms, ctx);

    // ---- the small-data side of the proof: one device buffer, one page-locked mirror -------------------------------------------
    const uint32_t n_polys[4] = {c.num_constants + c.num_routed, c.num_wires, nch * (1 + npp), nch * qdf};
    const uint32_t salt = d_salts ? SALT_SIZE : 0;
    const std::vector<uint32_t> leaf_len = {n_polys[0], n_polys[1] + salt, n_polys[2] + salt, n_polys[3] + salt};
    FriLayout L;
    TRY(fri_shapes(c, &L));
    SmallData sd;
    auto take = [&](uint64_t words) { return sd.take(words); };
    const Span T = take(32), HP = take(32), hostin = take(4 + (uint64_t)npi);
    const Span fetch0 = take(0);  // from here on: what the host fetches
    const Span pih_s = take(4), bg = take(2ull * nch), alphas_s = take(nch), zeta_s = take(2);
    Span opens[4], caps[3];
    for (int o = 0; o < 4; o++) opens[o] = take(2ull * (o == 2 ? 2 : 1) * n_polys[o]);
    for (int o = 0; o < 3; o++) caps[o] = take(cap_words);
    fri_layout(c, leaf_len, &sd, &L);
    const uint64_t top = sd.top;
    DevBuf small;
    TRY(small.alloc(top));
    uint64_t *const D = small.p;
    uint64_t *H = nullptr;
    TRY(pool->staging(top, &H));
    auto fetch = [&](const Span &sp) { return copy_async(H + sp.off, D + sp.off, sp.words * 8, true, ctx); };
    auto step = [&](std::initializer_list<GlObserveSrc> srcs, uint32_t n_out, const Span &out, uint32_t flags = 0, const Span *which = nullptr) {
        return gl_challenger_step(D + (which ? which->off : T.off), srcs.begin(), (uint32_t)srcs.size(), n_out, n_out || (flags & GL_CHALLENGER_HASH) ? D + out.off : nullptr,
                                  flags, ctx);
    };

    // circuit digest and public inputs go up once; hash_no_pad(public inputs) (prover.rs:52) on a scratch challenger
    memcpy(H + hostin.off, c.digest, 32);
    for (uint32_t i = 0; i < npi; i++) H[hostin.off + 4 + i] = h_public_inputs[i];
    TRY(copy_async(D + hostin.off, H + hostin.off, hostin.words * 8, false, ctx));
    TRY(step({GlObserveSrc{D + hostin.off + 4, npi, 0}}, 0, pih_s, GL_CHALLENGER_RESET | GL_CHALLENGER_HASH, &HP));
    // wires commitment (prover.rs:66-90); the caller's witness stays intact for the partial products
    Batch wires;
    {
        DevBuf w;
        TRY(w.alloc((uint64_t)c.num_wires * n));
        TRY(gl_memcpy_d2d(w.p, d_wires, 8ull * c.num_wires * n, ctx));
        TRY(commit(&wires, std::move(w), true, c.num_wires, c, ctx, d_salts, false));
    }
    TRY(st.mark(0));
    // challenger.observe_hash(circuit digest), observe_hash(public inputs hash), observe_cap(wires cap); betas, gammas (prover.rs:92-97)
    TRY(step({c.hashes(D + hostin.off, 4), GlObserveSrc{D + pih_s.off, 4, 0}, c.hashes(wires.cap_d.p, cap_words)}, 2 * nch, bg, GL_CHALLENGER_RESET));
    TRY(fetch(Span{pih_s.off, bg.off + bg.words - pih_s.off}));
    TRY(stream_sync(ctx));
    uint64_t pih[4];
    memcpy(pih, H + pih_s.off, 32);
    const std::vector<uint64_t> betas(H + bg.off, H + bg.off + nch), gammas(H + bg.off + nch, H + bg.off + 2 * nch);
    std::vector<uint64_t> alphas;
    // partial products and Z (prover.rs:99-117), committed in place
    Batch zs;
    {
        DevBuf z;
        TRY(z.alloc((uint64_t)nch * (1 + npp) * n));
        TRY(gl_permutation_partial_products(d_wires, n, c.sigmas.p, n, c.k_is.p, betas.data(), gammas.data(), nch, c.num_routed, qdf, db, z.p,
                                            ctx));
        TRY(st.mark(1));
        TRY(commit(&zs, std::move(z), true, nch * (1 + npp), c, ctx, d_salts ? d_salts + (uint64_t)SALT_SIZE * n_ext : nullptr, false));
    }
    TRY(st.mark(2));
    TRY(step({c.hashes(zs.cap_d.p, cap_words)}, nch, alphas_s));
    TRY(fetch(alphas_s));
    TRY(stream_sync(ctx));
    alphas.assign(H + alphas_s.off, H + alphas_s.off + nch);
    // quotient polynomials (prover.rs:137-151)
    const uint32_t qdb = glh::log2_ceil(qdf);
    DevBuf quotient, work;
    TRY(quotient.alloc((uint64_t)nch << (db + qdb)));
    {
        GlQuotientArgs a;
        memset(&a, 0, sizeof a);
        a.d_wires_leaves = wires.lde.p, a.d_constants_sigmas_leaves = c.cs.lde.p, a.d_zs_partial_products_leaves = zs.lde.p;
        a.wires_leaf_len = c.num_wires, a.constants_sigmas_leaf_len = c.num_constants + c.num_routed;
        a.zs_partial_products_leaf_len = nch * (1 + npp);
        a.d_k_is = c.k_is.p;
        a.h_betas = betas.data(), a.h_gammas = gammas.data(), a.h_alphas = alphas.data();
        a.num_constants = c.num_constants, a.num_routed_wires = c.num_routed, a.num_challenges = nch;
        a.num_gate_constraints = c.num_gates ? c.num_gate_constraints : 0;
        a.degree_bits = db, a.rate_bits = c.rate_bits, a.quotient_degree_factor = qdf, a.coset_shift = 7;
        a.column_stride = n_ext;
        GlGateProgram gp;
        memset(&gp, 0, sizeof gp);
        if (c.gate_kernel) {
            TRY(work.alloc((uint64_t)nch << (db + qdb)));
            a.gate_kernel = c.gate_kernel, a.h_public_inputs_hash = pih, a.d_gate_workspace = work.p;
        } else if (c.num_gates) {
            gp.d_instrs = reinterpret_cast<const GlGateInstr *>(c.d_instrs.p);
            gp.d_gates = reinterpret_cast<const GlGateDesc *>(c.d_gates.p);
            gp.d_immediates = c.d_imms.p;
            gp.num_gates = c.num_gates, gp.num_selectors = c.num_selectors;
            memcpy(gp.public_inputs_hash, pih, 32);
            a.gate_program = &gp;
        }
        TRY(gl_compute_quotient_polys(&a, quotient.p, ctx));
    }
    TRY(st.mark(3));
    // split into degree-n chunks (prover.rs:153-166) and commit from coefficients
    Batch quot;
    {
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
        TRY(commit(&quot, std::move(chunks), false, nch * qdf, c, ctx, d_salts ? d_salts + 2ull * SALT_SIZE * n_ext : nullptr, false));
    }
    TRY(st.mark(4));
    TRY(step({c.hashes(quot.cap_d.p, cap_words)}, 2, zeta_s));
    TRY(fetch(zeta_s));
    TRY(stream_sync(ctx));
    const E2 zeta{H[zeta_s.off], H[zeta_s.off + 1]};
    if (E2 zn = e2_pow(zeta, n); zn.a == 1 && zn.b == 0) return fail(GL_E_INVALID, "Opening point is in the subgroup.");
    const uint64_t g = glh::root_of_unity(db);
    const E2 g_zeta = e2_mul(E2{g, 0}, zeta);
    // OpeningSet::new (plonk/proof.rs:305-334): every oracle's polynomials at zeta, the Zs also at g * zeta, left in device memory
    const Batch *oracles[4] = {&c.cs, &wires, &zs, &quot};
    {
        const uint64_t pts[4] = {zeta.a, zeta.b, g_zeta.a, g_zeta.b};
        for (int o = 0; o < 4; o++)
            TRY(gl_eval_polys_ext2(oracles[o]->coeffs.p, oracles[o]->n_polys, db, n, pts, o == 2 ? 2 : 1, D + opens[o].off, ctx));
    }
    TRY(st.mark(5));
    // to_fri_openings (proof.rs:336-356): [constants, sigmas, wires, zs, partial products, quotient], then zs_next; then
    // PolynomialBatch::prove_openings: batch 0 is every polynomial of the four oracles at zeta, batch 1 the Zs at g*zeta
    // (circuit_data.rs:351-371)
    const std::vector<const Batch *> oracle_list(oracles, oracles + 4);
    uint64_t pow_witness = 0;
    {
        std::vector<FriBatch> batches(2);
        batches[0].point = zeta, batches[1].point = g_zeta;
        for (int o = 0; o < 4; o++)
            for (uint32_t k = 0; k < oracles[o]->n_polys; k++) batches[0].polys.push_back(oracles[o]->coeffs.p + (uint64_t)k * n);
        for (uint32_t k = 0; k < nch; k++) batches[1].polys.push_back(zs.coeffs.p + (uint64_t)k * n);
        const std::vector<GlObserveSrc> opening_srcs = {
            GlObserveSrc{D + opens[0].off, 2ull * n_polys[0], 0}, GlObserveSrc{D + opens[1].off, 2ull * n_polys[1], 0},
            GlObserveSrc{D + opens[2].off, 2ull * n_polys[2], 0}, GlObserveSrc{D + opens[3].off, 2ull * n_polys[3], 0},
            GlObserveSrc{D + opens[2].off + 2ull * n_polys[2], 2ull * nch, 0}};
        TRY(fri_prove(c, L, D, H, T, oracle_list, opening_srcs, batches, st, &pow_witness, ctx));
    }
    // everything the proof consists of, in one go
    TRY(gl_memcpy_d2d(D + caps[0].off, wires.cap_d.p, cap_words * 8, ctx));
    TRY(gl_memcpy_d2d(D + caps[1].off, zs.cap_d.p, cap_words * 8, ctx));
    TRY(gl_memcpy_d2d(D + caps[2].off, quot.cap_d.p, cap_words * 8, ctx));
    TRY(fetch(Span{fetch0.off, top - fetch0.off}));
    TRY(gl_ctx_synchronize(ctx));
    TRY(st.mark(9));
    TRY(fri_check_pow(c, L, H, pow_witness));
    // ---- write_proof_with_public_inputs (util/serialization.rs:641-689) ----
    Bytes out;
    out.keccak = c.keccak();
    for (int o = 0; o < 3; o++) out.hashes(H + caps[o].off, cap_words / 4);  // wires, zs / partial products, quotient
    // write_opening_set (:557-571): constants, sigmas, wires, zs, zs_next, partial products, quotient
    const uint64_t *ev[4] = {H + opens[0].off, H + opens[1].off, H + opens[2].off, H + opens[3].off};
    out.fields(ev[0], 2ull * n_polys[0]);                                   // constants then sigmas: contiguous
    out.fields(ev[1], 2ull * n_polys[1]);                                   // wires
    out.fields(ev[2], 2ull * nch);                                          // plonk_zs
    out.fields(ev[2] + 2ull * n_polys[2], 2ull * nch);                      // plonk_zs_next
    out.fields(ev[2] + 2ull * nch, 2ull * n_polys[2] - 2ull * nch);         // partial_products
    out.fields(ev[3], 2ull * n_polys[3]);                                   // quotient_polys
    fri_write(out, c, L, H, oracle_list, pow_witness);
    out.fields(h_public_inputs, num_public_inputs);
    TRY(bytes_out(out, proof, proof_len));
    return st.mark(10);
}

GlError gl_prove(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                 uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx) {
    return prove_impl(circuit, d_wires, h_public_inputs, num_public_inputs, nullptr, proof, proof_len, h_stage_ms, ctx);
}

// A batch of independent proofs of one circuit with several in flight (configs[4]'s unit of work per GPU): worker w — a host thread
// this call starts — proves witnesses w, w + in_flight, w + 2 in_flight, .. on ctxs[w]. The workers share the circuit handle (a buffer
// pool per context; the launches of its gate kernel take turns) and run at the same time: each fills the other's latency-bound phases.
GlError gl_prove_many(const void *circuit, const uint64_t *const *d_wires, const uint64_t *const *h_public_inputs, uint32_t num_public_inputs,
                      uint32_t count, uint8_t **proofs, uint64_t *proof_lens, void *const *ctxs, uint32_t in_flight) {
    if (!circuit || !proofs || !proof_lens || !ctxs || (count && (!d_wires || (num_public_inputs && !h_public_inputs)))) return fail(GL_E_INVALID, "null pointer");
    if (in_flight == 0 || in_flight > 16) return fail(GL_E_INVALID, "in_flight must be 1..16");
    for (uint32_t w = 0; w < in_flight; w++) {
        if (!ctxs[w]) return fail(GL_E_INVALID, "null context");
        for (uint32_t v = 0; v < w; v++)
            if (ctxs[v] == ctxs[w]) return fail(GL_E_INVALID, "every worker needs a context of its own");
    }
    for (uint32_t i = 0; i < count; i++) proofs[i] = nullptr, proof_lens[i] = 0;
    std::vector<GlError> errs(in_flight, GlError{0, nullptr});
    auto work = [&](uint32_t w) {
        for (uint32_t i = w; i < count; i += in_flight) {
            GlError e = prove_impl(circuit, d_wires[i], num_public_inputs ? h_public_inputs[i] : nullptr, num_public_inputs, nullptr, &proofs[i], &proof_lens[i],
                                   nullptr, ctxs[w]);
            if (e.code != 0) {
                errs[w] = e;
                return;
            }
        }
    };
    std::vector<std::thread> threads;
    for (uint32_t w = 1; w < in_flight && w < count; w++) threads.emplace_back(work, w);
    work(0);
    for (auto &t : threads) t.join();
    GlError first{0, nullptr};
    for (uint32_t w = 0; w < in_flight; w++)
        if (errs[w].code != 0) {
            if (first.code == 0) first = errs[w];
            else free(errs[w].message);
        }
    if (first.code != 0)
        for (uint32_t i = 0; i < count; i++) {  // all or nothing
            free(proofs[i]);
            proofs[i] = nullptr, proof_lens[i] = 0;
        }
    return first;
}

GlError gl_prove_zk(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                    const uint64_t *d_salts, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx) {
    if (!d_salts) return fail(GL_E_INVALID, "gl_prove_zk: null salt columns");
    return prove_impl(circuit, d_wires, h_public_inputs, num_public_inputs, d_salts, proof, proof_len, h_stage_ms, ctx);
}

}  // extern "C"

// ---- STARKs: gl_stark_create / gl_stark_prove = starky's prove() (starky/src/prover.rs:32-195); gl_stark_tables_create /
// gl_stark_tables_prove = prove_with_traces (evm/src/prover.rs:66-421) over the same per-table flow ------------------------------------
namespace {

struct Stark : ProverShape {
    uint32_t num_columns = 0, num_public_inputs = 0, num_challenges = 0, qdf = 0, qdb = 0, num_instrs = 0, num_pairs = 0, num_zs = 0;
    DevBuf d_instrs, d_imms, d_column_pairs, d_pair_bounds;
    // the description on the host, for gl_stark_compile's generator; jit: the compiled quotient kernel that replaces the interpreter
    // from gl_stark_compile on (null: interpreted)
    plonky2_hip::StarkJitDesc host;
    plonky2_hip::StarkJitKernel *jit = nullptr;
    ~Stark() { plonky2_hip::stark_jit_destroy(jit); }
    plonky2_hip::StarkPairsDev pairs() const {
        plonky2_hip::StarkPairsDev p;
        p.column_pairs = reinterpret_cast<const uint32_t *>(d_column_pairs.p), p.pair_bounds = reinterpret_cast<const uint32_t *>(d_pair_bounds.p);
        p.num_pairs = num_pairs;
        return p;
    }
};

GlError tables_of(void *ctx, const NttTables **tb) {
    if (hipError_t e = ctx_tables(ctx, tb); e != hipSuccess) return hip_fail(e, "context tables");
    return ok();
}

// the quotient values of one trace, then their coset_ifft (prover.rs:314-318); ctl / h_ctl_challenges: the table's CTL checks, or null
GlError stark_quotient(const Stark &s, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde, uint64_t column_stride, const uint64_t *h_alphas,
                       const uint64_t *h_challenges, const uint64_t *d_public_inputs, uint64_t *d_out, void *ctx,
                       const plonky2_hip::StarkCtlDev *ctl = nullptr, const uint64_t *h_ctl_challenges = nullptr) {
    const plonky2_hip::NttTables *tb;
    TRY(tables_of(ctx, &tb));
    plonky2_hip::StarkQuotientArgs a = {};
    a.instrs = reinterpret_cast<const uint16_t *>(s.d_instrs.p), a.num_instrs = s.num_instrs, a.imms = s.d_imms.p, a.public_inputs = d_public_inputs;
    a.trace_lde = d_trace_lde, a.zs_lde = d_zs_lde, a.column_stride = column_stride, a.pairs = s.pairs();
    a.alphas = h_alphas, a.challenges = h_challenges;
    a.num_challenges = s.num_challenges, a.qdf = s.qdf, a.degree_bits = s.degree_bits, a.rate_bits = s.rate_bits;
    if (ctl) a.ctl = *ctl, a.ctl_challenges = h_ctl_challenges;
    const hipError_t e = s.jit ? plonky2_hip::stark_jit_launch(s.jit, *tb, a, d_out, ctx_stream(ctx))
                               : plonky2_hip::stark_quotient_values(*tb, a, d_out, ctx_stream(ctx));
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "inconsistent arguments of the STARK quotient (column_stride / challenges / sizes)");
    if (e != hipSuccess) return hip_fail(e, "stark_quotient_values");
    const uint32_t log_size = s.degree_bits + s.qdb;
    return gl_coset_ntt_batch(d_out, s.num_challenges, log_size, 1ull << log_size, 7, 1, ctx);
}

// Everything gl_stark_create refuses, before anything is allocated. num_ctl_zs: the CTL Zs a table of
// gl_stark_tables_create adds to the Zs oracle (0 for a STARK on its own).
GlError stark_check(uint32_t hasher, const GlStarkDesc *d, uint32_t num_ctl_zs) {
    if (!d || !d->h_instrs || (d->num_immediates && !d->h_immediates) || (d->fri.num_reductions && !d->fri.reduction_arity_bits) ||
        (d->num_pairs && (!d->h_column_pairs || !d->h_pair_bounds)))
        return fail(GL_E_INVALID, "null pointer");
    if (d->struct_size != sizeof(GlStarkDesc))
        return fail(GL_E_INVALID, "GlStarkDesc.struct_size does not equal sizeof(GlStarkDesc) of this library: the caller was compiled against another version of include/plonky2_hip.h");
    if (hasher != GL_HASHER_POSEIDON && hasher != GL_HASHER_KECCAK25) return fail(GL_E_INVALID, "unknown hasher");
    if (d->fri.hiding) return fail(GL_E_INVALID, "a STARK's FRI parameters are not hiding (starky: fri_params(degree_bits, false))");
    if (d->degree_bits == 0 || d->degree_bits + d->fri.rate_bits > 24 || d->num_columns == 0 || d->num_columns > 65535 || d->num_public_inputs > 65535 ||
        d->num_challenges == 0 || d->num_challenges > plonky2_hip::STARK_MAX_CHALLENGES || d->constraint_degree == 0)
        return fail(GL_E_INVALID, "bad STARK shape (1 <= degree_bits, degree_bits + rate_bits <= 24, 1 <= num_columns, 1 <= num_challenges <= 4, 1 <= constraint_degree)");
    const uint32_t qdf = d->constraint_degree > 2 ? d->constraint_degree - 1 : 1;  // stark.rs:79-81
    const uint32_t qdb = glh::log2_ceil(qdf);
    if (qdf > plonky2_hip::STARK_MAX_QDF) return fail(GL_E_INVALID, "quotient_degree_factor > 16");
    if (qdb > d->fri.rate_bits) return fail(GL_E_INVALID, "Having constraints of degree higher than the rate is not supported yet. (log2_ceil(quotient_degree_factor) > rate_bits, prover.rs:223-226)");
    uint32_t total_arity = 0;
    for (uint32_t li = 0; li < d->fri.num_reductions; li++) total_arity += d->fri.reduction_arity_bits[li];
    if (d->fri.cap_height > d->degree_bits + d->fri.rate_bits || total_arity > d->degree_bits + d->fri.rate_bits - d->fri.cap_height || total_arity > d->degree_bits)
        return fail(GL_E_INVALID, "FRI total reduction arity is too large.");
    if (d->num_pairs) {
        if (d->h_pair_bounds[0] != 0) return fail(GL_E_INVALID, "h_pair_bounds must start at 0");
        for (uint32_t p = 0; p < d->num_pairs; p++)
            if (d->h_pair_bounds[p + 1] < d->h_pair_bounds[p]) return fail(GL_E_INVALID, "h_pair_bounds must not decrease");
        for (uint32_t k = 0; k < 2 * d->h_pair_bounds[d->num_pairs]; k++)
            if (d->h_column_pairs[k] >= d->num_columns) return fail(GL_E_INVALID, "permutation pair: column out of range");
    }
    const uint32_t num_zs = d->num_pairs ? plonky2_hip::stark_num_zs(d->num_pairs, d->num_challenges, qdf) : 0;
    {
        std::string verr;
        if (!plonky2_hip::stark_program_validate(reinterpret_cast<const uint16_t *>(d->h_instrs), d->num_instrs, d->h_immediates, d->num_immediates,
                                                 d->num_columns, d->num_public_inputs, &verr))
            return fail(GL_E_INVALID, verr);
    }
    if (hasher == GL_HASHER_KECCAK25) {  // as gl_circuit_create_h: KeccakHash<25>::hash_or_noop panics on a leaf of exactly four elements
        const struct {
            const char *name;
            uint32_t leaf_len;
        } commitments[3] = {{"trace", d->num_columns}, {num_ctl_zs ? "permutation / CTL Zs" : "permutation Zs", num_zs + num_ctl_zs}, {"quotient", d->num_challenges * qdf}};
        for (const auto &cm : commitments)
            if (cm.leaf_len == 4)
                return fail(GL_E_INVALID, std::string("KeccakHash<25> cannot hash a Merkle leaf of 4 elements (plonk/config.rs:56-63) and the leaves of the ") + cm.name +
                            " commitment have 4");
        for (uint32_t li = 0; li < d->fri.num_reductions; li++)
            if (d->fri.reduction_arity_bits[li] == 1)
                return fail(GL_E_INVALID, "KeccakHash<25> cannot hash a Merkle leaf of 4 elements (plonk/config.rs:56-63) and FRI reduction " + std::to_string(li) +
                            " has arity_bits = 1: its leaves are 2 extension elements");
    }
    return ok();
}

// after stark_check: what the generator of the compiled quotient kernel reads (stark_jit.h), without the CTL part
plonky2_hip::StarkJitDesc stark_host_desc(const GlStarkDesc *d) {
    plonky2_hip::StarkJitDesc h;
    const uint16_t *instrs = reinterpret_cast<const uint16_t *>(d->h_instrs);
    h.instrs.assign(instrs, instrs + 4ull * d->num_instrs);
    for (uint32_t i = 0; i < d->num_immediates; i++) h.imms.push_back(d->h_immediates[i] % P);
    h.num_challenges = d->num_challenges, h.qdf = d->constraint_degree > 2 ? d->constraint_degree - 1 : 1;
    if (d->num_pairs) {
        h.pair_bounds.assign(d->h_pair_bounds, d->h_pair_bounds + d->num_pairs + 1);
        h.column_pairs.assign(d->h_column_pairs, d->h_column_pairs + 2ull * d->h_pair_bounds[d->num_pairs]);
    }
    return h;
}

// the CTL part of table k's description: the arrays of all tables and the table's own CTL Zs
void stark_host_ctl(plonky2_hip::StarkJitDesc *h, const GlStarkTablesDesc *d, const std::vector<uint32_t> &zs) {
    const uint32_t ncol = d->num_ctl_columns, ntw = d->num_twcs, nterms = d->h_column_bounds[ncol];
    h->term_columns.assign(d->h_term_columns, d->h_term_columns + nterms);
    for (uint32_t j = 0; j < nterms; j++) h->term_coeffs.push_back(d->h_term_coeffs[j] % P);
    h->column_bounds.assign(d->h_column_bounds, d->h_column_bounds + ncol + 1);
    for (uint32_t k = 0; k < ncol; k++) h->column_constants.push_back(d->h_column_constants[k] % P);
    h->twc_column_bounds.assign(d->h_twc_column_bounds, d->h_twc_column_bounds + ntw + 1);
    h->twc_filter.assign(d->h_twc_filter, d->h_twc_filter + ntw);
    h->ctl_zs = zs;
}

// after stark_check
GlError stark_build(uint32_t hasher, const GlStarkDesc *d, Stark **stark, void *ctx) {
    const uint32_t qdf = d->constraint_degree > 2 ? d->constraint_degree - 1 : 1;
    const uint32_t qdb = glh::log2_ceil(qdf);
    const uint32_t num_column_pairs = d->num_pairs ? d->h_pair_bounds[d->num_pairs] : 0;
    const plonky2_hip::NttTables *tb;  // makes the context's device current before the first allocation
    TRY(tables_of(ctx, &tb));
    Stark *s = new Stark();
    s->hasher = hasher;
    s->degree_bits = d->degree_bits, s->num_columns = d->num_columns, s->num_public_inputs = d->num_public_inputs;
    s->num_challenges = d->num_challenges, s->qdf = qdf, s->qdb = qdb, s->num_instrs = d->num_instrs, s->num_pairs = d->num_pairs;
    s->num_zs = d->num_pairs ? plonky2_hip::stark_num_zs(d->num_pairs, d->num_challenges, qdf) : 0;
    s->set_fri(d->fri);
    s->host = stark_host_desc(d);
    auto bail = [&](GlError e) {
        delete s;
        return e;
    };
#define STRY(expr)                         \
    do {                                   \
        GlError _e = (expr);               \
        if (_e.code != 0) return bail(_e); \
    } while (0)
    STRY(s->d_instrs.alloc(d->num_instrs));  // 8 bytes per GlGateInstr
    STRY(gl_memcpy_h2d(s->d_instrs.p, d->h_instrs, 8ull * d->num_instrs, ctx));
    if (d->num_immediates) {
        std::vector<uint64_t> imms(d->h_immediates, d->h_immediates + d->num_immediates);
        for (uint64_t &v : imms) v %= P;
        STRY(s->d_imms.alloc(imms.size()));
        STRY(gl_memcpy_h2d(s->d_imms.p, imms.data(), 8ull * imms.size(), ctx));
    }
    if (d->num_pairs) {
        STRY(s->d_column_pairs.alloc(num_column_pairs ? num_column_pairs : 1));  // two u32 per column pair
        STRY(gl_memcpy_h2d(s->d_column_pairs.p, d->h_column_pairs, 8ull * num_column_pairs, ctx));
        STRY(s->d_pair_bounds.alloc((d->num_pairs + 2) / 2));
        STRY(gl_memcpy_h2d(s->d_pair_bounds.p, d->h_pair_bounds, 4ull * (d->num_pairs + 1), ctx));
    }
    STRY(gl_ctx_synchronize(ctx));
#undef STRY
    *stark = s;
    return ok();
}

// ---- the tables of gl_stark_tables_create: one Stark per table, the CTL descriptors in device memory ----
struct StarkTables : ProverShape {  // a ProverShape for its pools: the trace commitments, the CTL Zs and the shared transcript of a proof
    std::vector<Stark *> tables;
    uint32_t num_challenges = 0;
    DevBuf d_term_columns, d_term_coeffs, d_column_bounds, d_column_constants, d_twc_column_bounds, d_twc_filter;
    std::vector<DevBuf> d_zs;          // per table: (twc, challenge) of its CTL Zs, in the order of cross_table_lookup_data
    std::vector<uint32_t> num_ctl_zs;  // per table
    ~StarkTables() {
        for (Stark *s : tables) delete s;
    }
    plonky2_hip::StarkCtlDev ctl(uint32_t k) const {
        auto u32 = [](const DevBuf &b) { return reinterpret_cast<const uint32_t *>(b.p); };
        plonky2_hip::StarkCtlDev c;
        c.term_columns = u32(d_term_columns), c.column_bounds = u32(d_column_bounds), c.twc_column_bounds = u32(d_twc_column_bounds);
        c.twc_filter = u32(d_twc_filter), c.zs = u32(d_zs[k]), c.term_coeffs = d_term_coeffs.p, c.column_constants = d_column_constants.p;
        c.num_zs = num_ctl_zs[k];
        return c;
    }
};

// What a table of gl_stark_tables_prove brings to the flow of gl_stark_prove
struct CtlPart {
    Batch *trace;                     // committed before the transcript began
    plonky2_hip::StarkCtlDev ctl;     // ctl.num_zs CTL Zs behind the permutation Zs
    const uint64_t *d_ctl_zs;         // their values [ctl.num_zs][n]
    const uint64_t *h_ctl_challenges;
    uint64_t *d_transcript;           // the Challenger all tables share: compacted, never reset
    const uint64_t *h_filter_flag;    // page-locked; its copy is queued: valid after the next host synchronisation
};

// One STARK proof from the trace (commitment) to its bytes, appended to `out`: prove() of starky/src/prover.rs:32-195 with a fresh
// transcript and public inputs (ctl = null), or prove_single_table of evm/src/prover.rs:245-421 on the compacted shared transcript
// with the table's CTL Zs in the Zs oracle, their checks in the quotient and the third opening batch.
GlError stark_prove_one(const Stark &c, const uint64_t *d_trace, const uint64_t *h_public_inputs, const CtlPart *ctl, Bytes &out, double *h_stage_ms,
                        void *ctx) {
    Pool *pool = c.pool_of(ctx);
    PoolScope pool_scope(pool);  // every DevBuf below comes from / returns to the handle's pool of this context
    const uint32_t db = c.degree_bits, nch = c.num_challenges, qdf = c.qdf, qdb = c.qdb, npi = c.num_public_inputs;
    const uint32_t nperm = c.num_zs, nctl = ctl ? ctl->ctl.num_zs : 0, nz = nperm + nctl;
    const uint64_t n = 1ull << db, n_ext = n << c.rate_bits, cap_words = 4ull << c.cap_height;
    const bool perm = c.num_pairs != 0, has_zs = nz != 0;
    Stages st(h_stage_ms, ctx);

    // ---- the small-data side of the proof: one device buffer, one page-locked mirror ----
    // oracles: trace, [Zs], quotient (stark.rs:94-119)
    const uint32_t n_quot = nch * qdf;
    std::vector<uint32_t> leaf_len = {c.num_columns};
    if (has_zs) leaf_len.push_back(nz);
    leaf_len.push_back(n_quot);
    FriLayout L;
    TRY(fri_shapes(c, &L));
    SmallData sd;
    const Span T = sd.take(32), hostin = sd.take(npi);
    const Span fetch0 = sd.take(0);  // from here on: what the host fetches
    const Span perm_s = sd.take(perm ? 2ull * qdf * nch : 0), alphas_s = sd.take(nch), zeta_s = sd.take(2);
    // openings at zeta and g * zeta: [2][n_polys] extension elements for the trace and the Zs, [1][n_polys] for the quotient; the CTL
    // Zs at 1 / g as extension elements (x, 0)
    const Span open_trace = sd.take(4ull * c.num_columns), open_zs = sd.take(4ull * nz), open_quot = sd.take(2ull * n_quot), open_last = sd.take(2ull * nctl);
    const Span cap_trace = sd.take(cap_words), cap_zs = sd.take(has_zs ? cap_words : 0), cap_quot = sd.take(cap_words);
    fri_layout(c, leaf_len, &sd, &L);
    const uint64_t top = sd.top;
    DevBuf small;
    TRY(small.alloc(top));
    uint64_t *const D = small.p;
    uint64_t *H = nullptr;
    TRY(pool->staging(top, &H));
    auto fetch = [&](const Span &sp) { return copy_async(H + sp.off, D + sp.off, sp.words * 8, true, ctx); };
    auto step = [&](std::initializer_list<GlObserveSrc> srcs, uint32_t n_out, const Span &out_s, uint32_t flags = 0) {
        return gl_challenger_step(D + T.off, srcs.begin(), (uint32_t)srcs.size(), n_out, n_out ? D + out_s.off : nullptr, flags, ctx);
    };
    for (uint32_t i = 0; i < npi; i++) H[hostin.off + i] = h_public_inputs[i] % P;
    TRY(copy_async(D + hostin.off, H + hostin.off, hostin.words * 8, false, ctx));

    // trace commitment (prover.rs:57-70); the caller's trace stays intact
    Batch own_trace;
    if (!ctl) {
        DevBuf w;
        TRY(w.alloc((uint64_t)c.num_columns * n));
        TRY(gl_memcpy_d2d(w.p, d_trace, 8ull * c.num_columns * n, ctx));
        TRY(commit(&own_trace, std::move(w), true, c.num_columns, c, ctx, nullptr, false));
    } else {
        TRY(gl_memcpy_d2d(D + T.off, ctl->d_transcript, 32 * 8, ctx));  // the shared transcript runs on in this proof's buffer
    }
    Batch &trace = ctl ? *ctl->trace : own_trace;
    TRY(st.mark(0));
    // On its own: a fresh Challenger observes the trace cap (prover.rs:72-74), nothing else. As a table: the shared Challenger has
    // observed every trace cap already and is compacted (evm/src/prover.rs:271).
    const uint32_t begin = ctl ? GL_CHALLENGER_COMPACT : GL_CHALLENGER_RESET;
    auto filter_check = [&]() { return ctl && *ctl->h_filter_flag ? fail(GL_E_INVALID, "Non-binary filter?") : ok(); };
    Batch zs;
    std::vector<uint64_t> perm_challenges;
    if (has_zs) {
        DevBuf z;
        TRY(z.alloc((uint64_t)nz * n));
        if (perm) {
            // get_n_permutation_challenge_sets (permutation.rs:153-179): qdf sets of num_challenges (beta, gamma) draws
            if (ctl)
                TRY(step({}, 2 * qdf * nch, perm_s, begin));
            else
                TRY(step({c.hashes(trace.cap_d.p, cap_words)}, 2 * qdf * nch, perm_s, begin));
            TRY(fetch(perm_s));
            TRY(stream_sync(ctx));
            TRY(filter_check());
            perm_challenges.assign(H + perm_s.off, H + perm_s.off + 2ull * qdf * nch);
            TRY(gl_stark_permutation_zs(&c, d_trace, n, perm_challenges.data(), z.p, ctx));
        }
        // the Zs oracle: permutation Zs, then CTL Zs (evm/src/prover.rs:290-311)
        if (nctl) TRY(gl_memcpy_d2d(z.p + (uint64_t)nperm * n, ctl->d_ctl_zs, 8ull * nctl * n, ctx));
        TRY(st.mark(1));
        TRY(commit(&zs, std::move(z), true, nz, c, ctx, nullptr, false));
        TRY(st.mark(2));
        TRY(step({c.hashes(zs.cap_d.p, cap_words)}, nch, alphas_s, perm ? 0 : begin));
    } else {
        TRY(step({c.hashes(trace.cap_d.p, cap_words)}, nch, alphas_s, begin));
    }
    TRY(fetch(alphas_s));
    TRY(stream_sync(ctx));
    TRY(filter_check());
    const std::vector<uint64_t> alphas(H + alphas_s.off, H + alphas_s.off + nch);
    // quotient polynomials (prover.rs:115-123)
    DevBuf quotient;
    TRY(quotient.alloc((uint64_t)nch << (db + qdb)));
    TRY(stark_quotient(c, trace.lde.p, has_zs ? zs.lde.p : nullptr, n_ext, alphas.data(), perm ? perm_challenges.data() : nullptr, D + hostin.off,
                       quotient.p, ctx, ctl ? &ctl->ctl : nullptr, ctl ? ctl->h_ctl_challenges : nullptr));
    TRY(st.mark(3));
    // trim_to_len(degree * qdf) and the split into degree-n chunks (prover.rs:124-133), committed from coefficients. Of the
    // n << qdb coefficients those from qdf * n on must vanish: there are some only when qdf is no power of two.
    Batch quot;
    {
        DevBuf chunks;
        if (qdf == (1u << qdb)) {
            chunks = std::move(quotient);  // [nch][n << qdb] read flat is [nch * qdf][n]
        } else {
            TRY(chunks.alloc((uint64_t)n_quot * n));
            std::vector<uint64_t> tail((n << qdb) - (uint64_t)qdf * n);
            for (uint32_t k = 0; k < nch; k++) {
                TRY(gl_memcpy_d2h(tail.data(), quotient.p + ((uint64_t)k << (db + qdb)) + (uint64_t)qdf * n, tail.size() * 8, ctx));
                for (uint64_t t : tail)
                    if (t) return fail(GL_E_INVALID, "Quotient has failed, the vanishing polynomial is not divisible by Z_H");
                TRY(gl_memcpy_d2d(chunks.p + (uint64_t)k * qdf * n, quotient.p + ((uint64_t)k << (db + qdb)), 8ull * qdf * n, ctx));
            }
        }
        TRY(commit(&quot, std::move(chunks), false, n_quot, c, ctx, nullptr, false));
    }
    TRY(st.mark(4));
    TRY(step({c.hashes(quot.cap_d.p, cap_words)}, 2, zeta_s));
    TRY(fetch(zeta_s));
    TRY(stream_sync(ctx));
    const E2 zeta{H[zeta_s.off], H[zeta_s.off + 1]};
    if (E2 zn = e2_pow(zeta, n); zn.a == 1 && zn.b == 0) return fail(GL_E_INVALID, "Opening point is in the subgroup.");
    const uint64_t g = glh::root_of_unity(db);
    const E2 g_zeta = e2_mul(E2{g, 0}, zeta), g_inv{glh::inv(g), 0};
    // StarkOpeningSet::new (proof.rs:138-159; evm/src/proof.rs:190-224): trace and Zs at zeta and g * zeta, the quotient at zeta, the
    // CTL Zs at the last element of the subgroup
    {
        const uint64_t pts[4] = {zeta.a, zeta.b, g_zeta.a, g_zeta.b}, last[2] = {g_inv.a, g_inv.b};
        TRY(gl_eval_polys_ext2(trace.coeffs.p, c.num_columns, db, n, pts, 2, D + open_trace.off, ctx));
        if (has_zs) TRY(gl_eval_polys_ext2(zs.coeffs.p, nz, db, n, pts, 2, D + open_zs.off, ctx));
        TRY(gl_eval_polys_ext2(quot.coeffs.p, n_quot, db, n, pts, 1, D + open_quot.off, ctx));
        if (nctl) TRY(gl_eval_polys_ext2(zs.coeffs.p + (uint64_t)nperm * n, nctl, db, n, last, 1, D + open_last.off, ctx));
    }
    TRY(st.mark(5));
    // to_fri_openings (proof.rs:161-182): [local_values, permutation_zs, quotient_polys], then [next_values, permutation_zs_next], then
    // with CTLs [ctl_zs_last]; the instance of stark.rs:88-137 (evm/src/stark.rs:83-142): batch 0 everything at zeta, batch 1 trace then
    // Zs at g * zeta, batch 2 the CTL Zs at 1 / g
    std::vector<const Batch *> oracles = {&trace};
    if (has_zs) oracles.push_back(&zs);
    oracles.push_back(&quot);
    uint64_t pow_witness = 0;
    {
        std::vector<FriBatch> batches(nctl ? 3 : 2);
        batches[0].point = zeta, batches[1].point = g_zeta;
        for (const Batch *o : oracles)
            for (uint32_t k = 0; k < o->n_polys; k++) batches[0].polys.push_back(o->coeffs.p + (uint64_t)k * n);
        for (size_t o = 0; o + 1 < oracles.size(); o++)
            for (uint32_t k = 0; k < oracles[o]->n_polys; k++) batches[1].polys.push_back(oracles[o]->coeffs.p + (uint64_t)k * n);
        if (nctl) {
            batches[2].point = g_inv;
            for (uint32_t k = nperm; k < nz; k++) batches[2].polys.push_back(zs.coeffs.p + (uint64_t)k * n);
        }
        std::vector<GlObserveSrc> srcs = {GlObserveSrc{D + open_trace.off, 2ull * c.num_columns, 0}};
        if (has_zs) srcs.push_back(GlObserveSrc{D + open_zs.off, 2ull * nz, 0});
        srcs.push_back(GlObserveSrc{D + open_quot.off, 2ull * n_quot, 0});
        srcs.push_back(GlObserveSrc{D + open_trace.off + 2ull * c.num_columns, 2ull * c.num_columns, 0});
        if (has_zs) srcs.push_back(GlObserveSrc{D + open_zs.off + 2ull * nz, 2ull * nz, 0});
        if (nctl) srcs.push_back(GlObserveSrc{D + open_last.off, 2ull * nctl, 0});
        TRY(fri_prove(c, L, D, H, T, oracles, srcs, batches, st, &pow_witness, ctx));
    }
    if (ctl) TRY(gl_memcpy_d2d(ctl->d_transcript, D + T.off, 32 * 8, ctx));  // the next table goes on from here
    // everything the proof consists of, in one go
    TRY(gl_memcpy_d2d(D + cap_trace.off, trace.cap_d.p, cap_words * 8, ctx));
    if (has_zs) TRY(gl_memcpy_d2d(D + cap_zs.off, zs.cap_d.p, cap_words * 8, ctx));
    TRY(gl_memcpy_d2d(D + cap_quot.off, quot.cap_d.p, cap_words * 8, ctx));
    TRY(fetch(Span{fetch0.off, top - fetch0.off}));
    TRY(gl_ctx_synchronize(ctx));
    TRY(st.mark(9));
    TRY(fri_check_pow(c, L, H, pow_witness));
    // ---- the wire format of StarkProofWithPublicInputs / of one StarkProof of the tables (include/plonky2_hip.h) ----
    out.keccak = c.keccak();
    out.hashes(H + cap_trace.off, cap_words / 4);
    if (has_zs) out.hashes(H + cap_zs.off, cap_words / 4);
    out.hashes(H + cap_quot.off, cap_words / 4);
    out.fields(H + open_trace.off, 4ull * c.num_columns);  // local_values, next_values
    if (has_zs) out.fields(H + open_zs.off, 4ull * nz);    // permutation_zs, permutation_zs_next
    for (uint32_t k = 0; k < nctl; k++) out.field(H[open_last.off + 2ull * k]);  // ctl_zs_last: base field elements
    out.fields(H + open_quot.off, 2ull * n_quot);          // quotient_polys
    fri_write(out, c, L, H, oracles, pow_witness);
    out.fields(H + hostin.off, npi);
    return st.mark(10);
}

}  // namespace

extern "C" {

GlError gl_stark_create(uint32_t hasher, const GlStarkDesc *d, void **stark, void *ctx) {
    if (!d || !stark || !ctx) return fail(GL_E_INVALID, "null pointer");
    TRY(stark_check(hasher, d, 0));
    Stark *s = nullptr;
    TRY(stark_build(hasher, d, &s, ctx));
    *stark = s;
    return ok();
}

void gl_stark_destroy(void *stark) { delete static_cast<Stark *>(stark); }

GlError gl_stark_trim(void *stark) {
    if (!stark) return fail(GL_E_INVALID, "null pointer");
    return static_cast<Stark *>(stark)->trim();
}

GlError gl_stark_permutation_zs(const void *stark, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_challenges, uint64_t *d_zs,
                                void *ctx) {
    if (!stark || !d_trace || !h_challenges || !d_zs || !ctx) return fail(GL_E_INVALID, "null pointer");
    const Stark &s = *static_cast<const Stark *>(stark);
    if (!s.num_pairs) return fail(GL_E_INVALID, "the STARK has no permutation pairs");
    if (trace_stride < (1ull << s.degree_bits)) return fail(GL_E_INVALID, "trace_stride smaller than the column length");
    const plonky2_hip::NttTables *tb;
    TRY(tables_of(ctx, &tb));
    const hipError_t e = plonky2_hip::stark_permutation_zs(*tb, d_trace, trace_stride, s.pairs(), h_challenges, s.num_challenges, s.qdf, s.degree_bits, d_zs,
                                                           ctx_stream(ctx));
    if (e != hipSuccess) return hip_fail(e, "stark_permutation_zs");
    return ok();
}

// gl_stark_quotient_polys, and with `ctl` gl_stark_tables_quotient_polys
static GlError quotient_polys_call(const Stark &s, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde, uint64_t column_stride, const uint64_t *h_alphas,
                                   const uint64_t *h_challenges, const uint64_t *h_public_inputs, uint64_t *d_quotient_polys, void *ctx,
                                   const plonky2_hip::StarkCtlDev *ctl, const uint64_t *h_ctl_challenges) {
    if (s.num_pairs && (!d_zs_lde || !h_challenges)) return fail(GL_E_INVALID, "the STARK has permutation pairs: d_zs_lde and h_challenges are needed");
    if (s.num_public_inputs && !h_public_inputs) return fail(GL_E_INVALID, "null public inputs");
    if (column_stride < (1ull << (s.degree_bits + s.rate_bits))) return fail(GL_E_INVALID, "column_stride smaller than the LDE's column length n << rate_bits");
    const plonky2_hip::NttTables *tb;  // the context's device becomes current
    TRY(tables_of(ctx, &tb));
    DevBuf pis;
    TRY(pis.alloc(s.num_public_inputs));
    std::vector<uint64_t> h_pis(s.num_public_inputs);
    for (uint32_t i = 0; i < s.num_public_inputs; i++) h_pis[i] = h_public_inputs[i] % P;
    TRY(gl_memcpy_h2d(pis.p, h_pis.data(), 8ull * h_pis.size(), ctx));
    TRY(stark_quotient(s, d_trace_lde, d_zs_lde, column_stride, h_alphas, h_challenges, pis.p, d_quotient_polys, ctx, ctl, h_ctl_challenges));
    return gl_ctx_synchronize(ctx);  // pis is freed on return
}

GlError gl_stark_quotient_polys(const void *stark, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde, uint64_t column_stride,
                                const uint64_t *h_alphas, const uint64_t *h_challenges, const uint64_t *h_public_inputs,
                                uint64_t *d_quotient_polys, void *ctx) {
    if (!stark || !d_trace_lde || !h_alphas || !d_quotient_polys || !ctx) return fail(GL_E_INVALID, "null pointer");
    return quotient_polys_call(*static_cast<const Stark *>(stark), d_trace_lde, d_zs_lde, column_stride, h_alphas, h_challenges, h_public_inputs,
                               d_quotient_polys, ctx, nullptr, nullptr);
}

GlError gl_stark_prove(const void *stark, const uint64_t *d_trace, const uint64_t *h_public_inputs, uint8_t **proof, uint64_t *proof_len,
                       double *h_stage_ms, void *ctx) {
    if (!stark || !d_trace || !proof || !proof_len || !ctx) return fail(GL_E_INVALID, "null pointer");
    const Stark &c = *static_cast<const Stark *>(stark);
    if (c.num_public_inputs && !h_public_inputs) return fail(GL_E_INVALID, "null public inputs");
    {  // the context's device is current from here on, whatever the calling thread had: every allocation below follows it
        const plonky2_hip::NttTables *tb;
        TRY(tables_of(ctx, &tb));
    }
    if (h_stage_ms) memset(h_stage_ms, 0, sizeof(double) * GL_STARK_STAGES);
    Bytes out;
    TRY(stark_prove_one(c, d_trace, h_public_inputs, nullptr, out, h_stage_ms, ctx));
    return bytes_out(out, proof, proof_len);
}

// Everything gl_stark_tables_create refuses, before anything is allocated. zs: per table (twc, challenge) of its CTL Zs, in
// cross_table_lookup_data's order.
static GlError stark_tables_check(uint32_t hasher, const GlStarkTablesDesc *d, std::vector<std::vector<uint32_t>> *zs_out) {
    if (d->struct_size != sizeof(GlStarkTablesDesc))
        return fail(GL_E_INVALID, "GlStarkTablesDesc.struct_size does not equal sizeof(GlStarkTablesDesc) of this library: the caller was compiled against another version of include/plonky2_hip.h");
    if (!d->num_tables || !d->tables) return fail(GL_E_INVALID, "no tables");
    if (!d->num_lookups || !d->num_twcs || !d->h_lookup_bounds || !d->h_twc_table || !d->h_twc_column_bounds || !d->h_twc_filter || !d->h_column_bounds ||
        (d->num_ctl_columns && !d->h_column_constants))
        return fail(GL_E_INVALID, "No CTL? (null or empty cross-table lookup arrays)");
    const uint32_t nt = d->num_tables, ncol = d->num_ctl_columns, ntw = d->num_twcs, nl = d->num_lookups;
    auto bounds_ok = [](const uint32_t *b, uint32_t count, uint32_t limit) {
        if (b[0] != 0) return false;
        for (uint32_t i = 0; i < count; i++)
            if (b[i + 1] < b[i]) return false;
        return b[count] <= limit;
    };
    if (!bounds_ok(d->h_column_bounds, ncol, 0xFFFFFFFFu)) return fail(GL_E_INVALID, "h_column_bounds must start at 0 and not decrease");
    const uint32_t nterms = d->h_column_bounds[ncol];
    if (nterms && (!d->h_term_columns || !d->h_term_coeffs)) return fail(GL_E_INVALID, "null pointer");
    if (!bounds_ok(d->h_twc_column_bounds, ntw, ncol)) return fail(GL_E_INVALID, "h_twc_column_bounds must start at 0, not decrease and stay within the CTL columns");
    if (!bounds_ok(d->h_lookup_bounds, nl, ntw)) return fail(GL_E_INVALID, "h_lookup_bounds must start at 0, not decrease and stay within the TWCs");
    const uint32_t nch = d->tables[0].num_challenges;
    for (uint32_t k = 0; k < nt; k++) {
        const GlStarkDesc &t = d->tables[k], &t0 = d->tables[0];
        if (t.struct_size != sizeof(GlStarkDesc)) return fail(GL_E_INVALID, "GlStarkDesc.struct_size does not equal sizeof(GlStarkDesc) of this library: the caller was compiled against another version of include/plonky2_hip.h");
        if (t.num_challenges != t0.num_challenges || t.fri.rate_bits != t0.fri.rate_bits || t.fri.cap_height != t0.fri.cap_height ||
            t.fri.proof_of_work_bits != t0.fri.proof_of_work_bits || t.fri.num_query_rounds != t0.fri.num_query_rounds || (t.fri.hiding != 0) != (t0.fri.hiding != 0))
            return fail(GL_E_INVALID, "table " + std::to_string(k) + ": the tables share one StarkConfig (num_challenges, rate_bits, cap_height, proof_of_work_bits, num_query_rounds, hiding); only reduction_arity_bits may differ");
        if (t.num_public_inputs) return fail(GL_E_INVALID, "table " + std::to_string(k) + ": a table of a multi-table STARK has no public inputs");
    }
    // a CTL column as used by a TWC of table `table`: its terms name columns of that table
    auto column_ok = [&](uint32_t col, uint32_t table) {
        for (uint32_t j = d->h_column_bounds[col]; j < d->h_column_bounds[col + 1]; j++)
            if (d->h_term_columns[j] >= d->tables[table].num_columns) return false;
        return true;
    };
    for (uint32_t t = 0; t < ntw; t++) {
        if (d->h_twc_table[t] >= nt) return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": table out of range");
        if (d->h_twc_filter[t] != GL_CTL_NO_FILTER && d->h_twc_filter[t] >= ncol) return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": filter column out of range");
        for (uint32_t k = d->h_twc_column_bounds[t]; k < d->h_twc_column_bounds[t + 1]; k++)
            if (!column_ok(k, d->h_twc_table[t])) return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": a term's column is out of range for its table");
        if (d->h_twc_filter[t] != GL_CTL_NO_FILTER && !column_ok(d->h_twc_filter[t], d->h_twc_table[t]))
            return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": a term's column of the filter is out of range for its table");
    }
    std::vector<std::vector<uint32_t>> &zs = *zs_out;
    zs.assign(nt, {});
    std::vector<bool> filtered(nt, false), unfiltered(nt, false);
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t lo = d->h_lookup_bounds[l], hi = d->h_lookup_bounds[l + 1];
        if (hi - lo < 2) return fail(GL_E_INVALID, "lookup " + std::to_string(l) + ": a lookup has at least one looking table and the looked table");
        const uint32_t width = d->h_twc_column_bounds[lo + 1] - d->h_twc_column_bounds[lo];
        const bool has_filter = d->h_twc_filter[lo] != GL_CTL_NO_FILTER;
        for (uint32_t t = lo; t < hi; t++) {
            if (d->h_twc_column_bounds[t + 1] - d->h_twc_column_bounds[t] != width) return fail(GL_E_INVALID, "lookup " + std::to_string(l) + ": its tables have unequal numbers of columns");
            if ((d->h_twc_filter[t] != GL_CTL_NO_FILTER) != has_filter)
                return fail(GL_E_INVALID, "lookup " + std::to_string(l) + ": either every table of a lookup has a filter column or none has (CrossTableLookup::new)");
            (has_filter ? filtered : unfiltered)[d->h_twc_table[t]] = true;
        }
        for (uint32_t c = 0; c < nch; c++)
            for (uint32_t t = lo; t < hi; t++) zs[d->h_twc_table[t]].push_back(t), zs[d->h_twc_table[t]].push_back(c);
    }
    for (uint32_t k = 0; k < nt; k++) {
        if (zs[k].empty()) return fail(GL_E_INVALID, "No CTL? (no lookup names table " + std::to_string(k) + ")");
        if (filtered[k] && d->tables[k].constraint_degree < 3) return fail(GL_E_INVALID, "table " + std::to_string(k) + ": the checks of a filtered CTL Z have degree 3: constraint_degree must be at least 3");
        if (d->tables[k].constraint_degree < 2) return fail(GL_E_INVALID, "table " + std::to_string(k) + ": the checks of a CTL Z have degree 2: constraint_degree must be at least 2");
        TRY(stark_check(hasher, &d->tables[k], (uint32_t)zs[k].size() / 2));
    }
    return ok();
}

GlError gl_stark_tables_create(uint32_t hasher, const GlStarkTablesDesc *d, void **tables, void *ctx) {
    if (!d || !tables || !ctx) return fail(GL_E_INVALID, "null pointer");
    std::vector<std::vector<uint32_t>> zs;  // per table (twc, challenge), cross_table_lookup_data's order
    TRY(stark_tables_check(hasher, d, &zs));
    const uint32_t nt = d->num_tables, ncol = d->num_ctl_columns, ntw = d->num_twcs, nterms = d->h_column_bounds[ncol];
    const uint32_t nch = d->tables[0].num_challenges;
    const plonky2_hip::NttTables *tb;
    TRY(tables_of(ctx, &tb));
    StarkTables *T = new StarkTables();
    auto bail = [&](GlError e) {
        delete T;
        return e;
    };
#define STRY(expr)                         \
    do {                                   \
        GlError _e = (expr);               \
        if (_e.code != 0) return bail(_e); \
    } while (0)
    T->hasher = hasher, T->num_challenges = nch;
    T->set_fri(d->tables[0].fri);
    for (uint32_t k = 0; k < nt; k++) {
        Stark *s = nullptr;
        STRY(stark_build(hasher, &d->tables[k], &s, ctx));
        stark_host_ctl(&s->host, d, zs[k]);
        T->tables.push_back(s);
    }
    auto upload32 = [&](DevBuf &b, const uint32_t *src, uint64_t count) -> GlError {
        TRY(b.alloc((count + 1) / 2));
        return count ? gl_memcpy_h2d(b.p, src, 4 * count, ctx) : ok();
    };
    auto upload64 = [&](DevBuf &b, const uint64_t *src, uint64_t count) -> GlError {
        std::vector<uint64_t> v(src, src + count);
        for (uint64_t &x : v) x %= P;
        TRY(b.alloc(count));
        return count ? gl_memcpy_h2d(b.p, v.data(), 8 * count, ctx) : ok();
    };
    STRY(upload32(T->d_term_columns, d->h_term_columns, nterms));
    STRY(upload64(T->d_term_coeffs, d->h_term_coeffs, nterms));
    STRY(upload32(T->d_column_bounds, d->h_column_bounds, ncol + 1ull));
    STRY(upload64(T->d_column_constants, d->h_column_constants, ncol));
    STRY(upload32(T->d_twc_column_bounds, d->h_twc_column_bounds, ntw + 1ull));
    STRY(upload32(T->d_twc_filter, d->h_twc_filter, ntw));
    T->d_zs.resize(nt);
    for (uint32_t k = 0; k < nt; k++) {
        STRY(upload32(T->d_zs[k], zs[k].data(), zs[k].size()));
        T->num_ctl_zs.push_back((uint32_t)zs[k].size() / 2);
    }
    STRY(gl_ctx_synchronize(ctx));
#undef STRY
    *tables = T;
    return ok();
}

void gl_stark_tables_destroy(void *tables) { delete static_cast<StarkTables *>(tables); }

GlError gl_stark_tables_trim(void *tables) {
    if (!tables) return fail(GL_E_INVALID, "null pointer");
    StarkTables *T = static_cast<StarkTables *>(tables);
    for (Stark *s : T->tables) TRY(s->trim());
    return T->trim();
}

// the CTL Zs of table k; *d_flag is raised by a non-binary filter
static GlError tables_ctl_zs(const StarkTables &T, uint32_t k, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_ctl_challenges,
                             uint64_t *d_zs, uint64_t *d_flag, void *ctx) {
    const plonky2_hip::NttTables *tb;
    TRY(tables_of(ctx, &tb));
    const hipError_t e = plonky2_hip::stark_ctl_zs(*tb, d_trace, trace_stride, T.ctl(k), h_ctl_challenges, T.num_challenges, T.tables[k]->degree_bits, d_zs,
                                                   d_flag, ctx_stream(ctx));
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "inconsistent arguments of the CTL Zs (trace_stride / sizes / more Zs than the context's scratch holds block totals for)");
    if (e != hipSuccess) return hip_fail(e, "stark_ctl_zs");
    return ok();
}

GlError gl_stark_tables_ctl_zs(const void *tables, uint32_t table, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_ctl_challenges,
                               uint64_t *d_zs, void *ctx) {
    if (!tables || !d_trace || !h_ctl_challenges || !d_zs || !ctx) return fail(GL_E_INVALID, "null pointer");
    const StarkTables &T = *static_cast<const StarkTables *>(tables);
    if (table >= T.tables.size()) return fail(GL_E_INVALID, "table out of range");
    if (trace_stride < (1ull << T.tables[table]->degree_bits)) return fail(GL_E_INVALID, "trace_stride smaller than the column length");
    {
        const plonky2_hip::NttTables *tb;
        TRY(tables_of(ctx, &tb));
    }
    DevBuf flag;
    TRY(flag.alloc(1));
    TRY(gl_memset_zero(flag.p, 8, ctx));
    TRY(tables_ctl_zs(T, table, d_trace, trace_stride, h_ctl_challenges, d_zs, flag.p, ctx));
    uint64_t h_flag = 0;
    TRY(gl_memcpy_d2h(&h_flag, flag.p, 8, ctx));  // synchronous
    if (h_flag) return fail(GL_E_INVALID, "Non-binary filter?");
    return ok();
}

GlError gl_stark_tables_quotient_polys(const void *tables, uint32_t table, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde,
                                       uint64_t column_stride, const uint64_t *h_alphas, const uint64_t *h_perm_challenges,
                                       const uint64_t *h_ctl_challenges, uint64_t *d_quotient_polys, void *ctx) {
    if (!tables || !d_trace_lde || !d_zs_lde || !h_alphas || !h_ctl_challenges || !d_quotient_polys || !ctx) return fail(GL_E_INVALID, "null pointer");
    const StarkTables &T = *static_cast<const StarkTables *>(tables);
    if (table >= T.tables.size()) return fail(GL_E_INVALID, "table out of range");
    const plonky2_hip::StarkCtlDev ctl = T.ctl(table);
    return quotient_polys_call(*T.tables[table], d_trace_lde, d_zs_lde, column_stride, h_alphas, h_perm_challenges, nullptr, d_quotient_polys, ctx, &ctl,
                               h_ctl_challenges);
}

GlError gl_stark_tables_prove(const void *tables, const uint64_t *const *d_traces, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms,
                              void *ctx) {
    if (!tables || !d_traces || !proof || !proof_len || !ctx) return fail(GL_E_INVALID, "null pointer");
    const StarkTables &T = *static_cast<const StarkTables *>(tables);
    const uint32_t nt = (uint32_t)T.tables.size(), nch = T.num_challenges;
    for (uint32_t k = 0; k < nt; k++)
        if (!d_traces[k]) return fail(GL_E_INVALID, "null trace");
    {
        const plonky2_hip::NttTables *tb;
        TRY(tables_of(ctx, &tb));
    }
    Pool *pool = T.pool_of(ctx);
    PoolScope pool_scope(pool);  // the trace commitments, the CTL Zs and the shared small data; every table's own buffers: its Stark's pool
    if (h_stage_ms) memset(h_stage_ms, 0, sizeof(double) * GL_STARK_STAGES * nt);
    auto ms = [&](uint32_t k) { return h_stage_ms ? h_stage_ms + (size_t)GL_STARK_STAGES * k : nullptr; };
    const uint64_t cap_words = 4ull << T.cap_height;
    SmallData sd;
    const Span TR = sd.take(32), chal_s = sd.take(2ull * nch), flag_s = sd.take(1);
    DevBuf small;
    TRY(small.alloc(sd.top));
    uint64_t *const D = small.p;
    uint64_t *H = nullptr;
    TRY(pool->staging(sd.top, &H));
    TRY(gl_memset_zero(D + flag_s.off, 8, ctx));
    // every trace is committed before the transcript begins (evm/src/prover.rs:86-118) and stays until its table is proved
    std::vector<Batch> traces(nt);
    for (uint32_t k = 0; k < nt; k++) {
        const Stark &c = *T.tables[k];
        Stages st(ms(k), ctx);
        DevBuf w;
        TRY(w.alloc((uint64_t)c.num_columns << c.degree_bits));
        TRY(gl_memcpy_d2d(w.p, d_traces[k], (8ull * c.num_columns) << c.degree_bits, ctx));
        TRY(commit(&traces[k], std::move(w), true, c.num_columns, c, ctx, nullptr, false));
        TRY(st.mark(0));
    }
    // a fresh Challenger observes all trace caps, then get_grand_product_challenge_set (cross_table_lookup.rs:243)
    for (uint32_t k = 0; k < nt; k += 8) {
        std::vector<GlObserveSrc> srcs;
        for (uint32_t j = k; j < nt && j < k + 8; j++) srcs.push_back(T.hashes(traces[j].cap_d.p, cap_words));
        const bool last = k + 8 >= nt;
        TRY(gl_challenger_step(D + TR.off, srcs.data(), (uint32_t)srcs.size(), last ? 2 * nch : 0, last ? D + chal_s.off : nullptr,
                               k == 0 ? GL_CHALLENGER_RESET : 0, ctx));
    }
    TRY(copy_async(H + chal_s.off, D + chal_s.off, chal_s.words * 8, true, ctx));
    TRY(stream_sync(ctx));
    const std::vector<uint64_t> ctl_challenges(H + chal_s.off, H + chal_s.off + 2ull * nch);
    std::vector<DevBuf> ctl_zs(nt);
    for (uint32_t k = 0; k < nt; k++) {
        const Stark &c = *T.tables[k];
        Stages st(ms(k), ctx);
        TRY(ctl_zs[k].alloc((uint64_t)T.num_ctl_zs[k] << c.degree_bits));
        TRY(tables_ctl_zs(T, k, d_traces[k], 1ull << c.degree_bits, ctl_challenges.data(), ctl_zs[k].p, D + flag_s.off, ctx));
        TRY(st.mark(1));
    }
    H[flag_s.off] = 0;
    TRY(copy_async(H + flag_s.off, D + flag_s.off, 8, true, ctx));  // read at the first table's first synchronisation
    Bytes out;
    for (uint32_t k = 0; k < nt; k++) {
        CtlPart part{&traces[k], T.ctl(k), ctl_zs[k].p, ctl_challenges.data(), D + TR.off, H + flag_s.off};
        TRY(stark_prove_one(*T.tables[k], d_traces[k], nullptr, &part, out, ms(k), ctx));
        traces[k] = Batch();  // this table's trace LDE and CTL Zs return to the pool
        ctl_zs[k].reset();
    }
    return bytes_out(out, proof, proof_len);
}

// ---- the compiled quotient kernels (stark_jit.hip) ----
// the sources of every description's units under the cap, flat, with bounds[i] .. bounds[i + 1] those of description i
static std::vector<std::string> stark_unit_sources(const std::vector<const plonky2_hip::StarkJitDesc *> &descs, uint32_t max_unit_instrs, std::vector<size_t> *bounds) {
    std::vector<std::string> sources;
    bounds->assign(1, 0);
    for (const plonky2_hip::StarkJitDesc *h : descs) {
        const std::vector<plonky2_hip::StarkJitUnit> units = plonky2_hip::stark_jit_units(*h, max_unit_instrs);
        for (size_t u = 0; u < units.size(); u++) sources.push_back(plonky2_hip::stark_jit_unit_source(*h, units[u], u == 0, u + 1 == units.size()));
        bounds->push_back(sources.size());
    }
    return sources;
}

// gl_*_units' max_unit_instrs: 0 is the library's default cap
static uint32_t unit_cap(uint32_t max_unit_instrs) { return max_unit_instrs ? max_unit_instrs : plonky2_hip::STARK_JIT_DEFAULT_UNIT_INSTRS; }

static GlError stark_compile_all(const std::vector<Stark *> &tables, uint32_t max_unit_instrs, void *ctx) {
    {  // the context's device becomes current: the modules are loaded there
        const plonky2_hip::NttTables *tb;
        TRY(tables_of(ctx, &tb));
    }
    std::vector<Stark *> todo;
    for (Stark *s : tables)
        if (!s->jit) todo.push_back(s);
    if (todo.empty()) return ok();  // a second call is a no-op
    std::vector<const plonky2_hip::StarkJitDesc *> descs;
    for (Stark *s : todo) descs.push_back(&s->host);
    std::vector<size_t> bounds;
    const std::vector<std::string> sources = stark_unit_sources(descs, max_unit_instrs, &bounds);
    std::vector<std::vector<char>> codes;
    std::string err;
    if (!plonky2_hip::stark_jit_compile_sources(sources, &codes, nullptr, &err)) return fail(GL_E_INVALID, err);
    // all or nothing: a handle whose compile failed stays interpreted
    std::vector<plonky2_hip::StarkJitKernel *> kernels;
    for (size_t i = 0; i < todo.size(); i++) {
        plonky2_hip::StarkJitKernel *k = plonky2_hip::stark_jit_load(
            todo[i]->host, std::vector<std::string>(sources.begin() + bounds[i], sources.begin() + bounds[i + 1]),
            std::vector<std::vector<char>>(std::make_move_iterator(codes.begin() + bounds[i]), std::make_move_iterator(codes.begin() + bounds[i + 1])), &err);
        if (!k) {
            for (plonky2_hip::StarkJitKernel *done : kernels) plonky2_hip::stark_jit_destroy(done);
            return fail(GL_E_INVALID, err);
        }
        kernels.push_back(k);
    }
    for (size_t i = 0; i < todo.size(); i++) todo[i]->jit = kernels[i];
    return ok();
}

static GlError stark_precompile_all(const std::vector<plonky2_hip::StarkJitDesc> &descs, uint32_t max_unit_instrs) {
    if (plonky2_hip::jit_cache_dir().empty())
        return fail(GL_E_INVALID, "no kernel cache to compile into: set PLONKY2_HIP_KERNEL_CACHE or create the directory kernel_cache next to the library");
    std::vector<const plonky2_hip::StarkJitDesc *> ptrs;
    for (const plonky2_hip::StarkJitDesc &h : descs) ptrs.push_back(&h);
    std::vector<size_t> bounds;
    const std::vector<std::string> sources = stark_unit_sources(ptrs, max_unit_instrs, &bounds);
    std::vector<std::vector<char>> codes;
    std::string err;
    if (!plonky2_hip::stark_jit_compile_sources(sources, &codes, nullptr, &err)) return fail(GL_E_INVALID, err);
    return ok();
}

GlError gl_stark_compile(void *stark, void *ctx) {
    if (!stark || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all({static_cast<Stark *>(stark)}, plonky2_hip::STARK_JIT_ONE_UNIT, ctx);
}

GlError gl_stark_tables_compile(void *tables, void *ctx) {
    if (!tables || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all(static_cast<StarkTables *>(tables)->tables, plonky2_hip::STARK_JIT_ONE_UNIT, ctx);
}

GlError gl_stark_compile_units(void *stark, uint32_t max_unit_instrs, void *ctx) {
    if (!stark || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all({static_cast<Stark *>(stark)}, unit_cap(max_unit_instrs), ctx);
}

GlError gl_stark_tables_compile_units(void *tables, uint32_t max_unit_instrs, void *ctx) {
    if (!tables || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all(static_cast<StarkTables *>(tables)->tables, unit_cap(max_unit_instrs), ctx);
}

int gl_stark_is_compiled(const void *stark) { return stark && static_cast<const Stark *>(stark)->jit ? 1 : 0; }

int gl_stark_tables_is_compiled(const void *tables) {
    if (!tables) return 0;
    for (const Stark *s : static_cast<const StarkTables *>(tables)->tables)
        if (!s->jit) return 0;
    return 1;
}

int gl_stark_kernel_units(const void *stark) {
    const Stark *s = static_cast<const Stark *>(stark);
    return s && s->jit ? (int)plonky2_hip::stark_jit_kernel_units(s->jit) : 0;
}

int gl_stark_tables_kernel_units(const void *tables, uint32_t table) {
    const StarkTables *T = static_cast<const StarkTables *>(tables);
    if (!T || table >= T->tables.size()) return 0;
    return gl_stark_kernel_units(T->tables[table]);
}

const char *gl_stark_kernel_unit_source(const void *stark, uint32_t unit) {
    const Stark *s = static_cast<const Stark *>(stark);
    return s && s->jit ? plonky2_hip::stark_jit_kernel_source(s->jit, unit) : nullptr;
}

const char *gl_stark_tables_kernel_unit_source(const void *tables, uint32_t table, uint32_t unit) {
    const StarkTables *T = static_cast<const StarkTables *>(tables);
    if (!T || table >= T->tables.size()) return nullptr;
    return gl_stark_kernel_unit_source(T->tables[table], unit);
}

const char *gl_stark_kernel_source(const void *stark) { return gl_stark_kernel_unit_source(stark, 0); }

const char *gl_stark_tables_kernel_source(const void *tables, uint32_t table) { return gl_stark_tables_kernel_unit_source(tables, table, 0); }

static GlError stark_precompile_one(uint32_t hasher, const GlStarkDesc *d, uint32_t max_unit_instrs) {
    if (!d) return fail(GL_E_INVALID, "null pointer");
    TRY(stark_check(hasher, d, 0));
    return stark_precompile_all({stark_host_desc(d)}, max_unit_instrs);
}

static GlError stark_precompile_tables(uint32_t hasher, const GlStarkTablesDesc *d, uint32_t max_unit_instrs) {
    if (!d) return fail(GL_E_INVALID, "null pointer");
    std::vector<std::vector<uint32_t>> zs;
    TRY(stark_tables_check(hasher, d, &zs));
    std::vector<plonky2_hip::StarkJitDesc> descs;
    for (uint32_t k = 0; k < d->num_tables; k++) {
        descs.push_back(stark_host_desc(&d->tables[k]));
        stark_host_ctl(&descs.back(), d, zs[k]);
    }
    return stark_precompile_all(descs, max_unit_instrs);
}

GlError gl_stark_precompile(uint32_t hasher, const GlStarkDesc *d) { return stark_precompile_one(hasher, d, plonky2_hip::STARK_JIT_ONE_UNIT); }

GlError gl_stark_tables_precompile(uint32_t hasher, const GlStarkTablesDesc *d) { return stark_precompile_tables(hasher, d, plonky2_hip::STARK_JIT_ONE_UNIT); }

GlError gl_stark_precompile_units(uint32_t hasher, const GlStarkDesc *d, uint32_t max_unit_instrs) {
    return stark_precompile_one(hasher, d, unit_cap(max_unit_instrs));
}

GlError gl_stark_tables_precompile_units(uint32_t hasher, const GlStarkTablesDesc *d, uint32_t max_unit_instrs) {
    return stark_precompile_tables(hasher, d, unit_cap(max_unit_instrs));
}

// the device-free splitter (stark_split.hip) behind the checks gl_stark_create makes of the program
GlError gl_stark_split_program(const GlStarkDesc *d, uint32_t max_unit_instrs, GlGatePrograms *out) {
    if (!d || !out || !d->h_instrs || (d->num_immediates && !d->h_immediates)) return fail(GL_E_INVALID, "null pointer");
    memset(out, 0, sizeof *out);
    if (d->struct_size != sizeof(GlStarkDesc))
        return fail(GL_E_INVALID, "GlStarkDesc.struct_size does not equal sizeof(GlStarkDesc) of this library: the caller was compiled against another version of include/plonky2_hip.h");
    const uint16_t *instrs = reinterpret_cast<const uint16_t *>(d->h_instrs);
    std::string verr;
    if (!plonky2_hip::stark_program_validate(instrs, d->num_instrs, d->h_immediates, d->num_immediates, d->num_columns, d->num_public_inputs, &verr))
        return fail(GL_E_INVALID, verr);
    const std::vector<plonky2_hip::StarkProgramUnit> units = plonky2_hip::stark_program_split(instrs, d->num_instrs, unit_cap(max_unit_instrs));
    size_t words = 0;
    for (const plonky2_hip::StarkProgramUnit &u : units) words += u.instrs.size();
    out->instrs = (GlGateInstr *)malloc(std::max<size_t>(1, words) * sizeof(uint16_t));
    out->gates = (GlGateDesc *)malloc(units.size() * sizeof(GlGateDesc));
    out->immediates = (uint64_t *)malloc(std::max<size_t>(1, d->num_immediates) * sizeof(uint64_t));
    if (!out->instrs || !out->gates || !out->immediates) {
        gl_gate_programs_free(out);
        return fail(GL_E_INVALID, "gl_stark_split_program: out of memory");
    }
    uint32_t at = 0;
    for (size_t k = 0; k < units.size(); k++) {
        const uint32_t len = (uint32_t)(units[k].instrs.size() / 4);
        memcpy(out->instrs + at, units[k].instrs.data(), units[k].instrs.size() * sizeof(uint16_t));
        out->gates[k] = GlGateDesc{(uint32_t)k, 0, units[k].emit_start, units[k].emit_end, at, len};
        at += len;
    }
    if (d->num_immediates) memcpy(out->immediates, d->h_immediates, d->num_immediates * sizeof(uint64_t));
    out->num_instrs = at, out->num_gates = (uint32_t)units.size(), out->num_immediates = d->num_immediates;
    out->num_gate_constraints = units.back().emit_end;
    return ok();
}

}  // extern "C"
