// prove_common.h — what the provers' host logic shares (prove.hip, stark_prove.hip, stark_compile.hip): pooled device buffers, committed
// batches, a prover's shape, one proof's session, the wire format and the FRI half of a proof (prove_common.hip). Internal (exports.map).
#pragma once
#include <chrono>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "commit.h"
#include "gl_field.h"

namespace plonky2_hip {

using glh::P;

struct E2 {  // a + bX, X^2 = 7 (field/src/goldilocks_extensions.rs:13-26)
    uint64_t a, b;
};
inline E2 e2_mul(E2 x, E2 y) {
    return E2{glh::add(glh::mul(x.a, y.a), glh::mul(7, glh::mul(x.b, y.b))), glh::add(glh::mul(x.a, y.b), glh::mul(x.b, y.a))};
}
inline E2 e2_pow(E2 x, uint64_t e) {
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
            TRY(gl_malloc_host(&q, words * 8));
            pinned = static_cast<uint64_t *>(q), pinned_words = words;
        }
        *out = pinned;
        return ok();
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
inline thread_local Pool *g_pool = nullptr;  // installed by gl_prove for its duration; null = plain gl_malloc / gl_free
struct PoolScope {
    Pool *prev;
    explicit PoolScope(Pool *p) : prev(g_pool) { g_pool = p; }
    ~PoolScope() { g_pool = prev; }
};

struct DevBuf {  // RAII device buffer of u64
    uint64_t *p = nullptr;
    uint64_t bytes = 0;
    Pool *pool = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), pool(o.pool) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        reset();
        p = o.p, bytes = o.bytes, pool = o.pool, o.p = nullptr;
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

constexpr uint32_t SALT_SIZE = 4;  // fri/oracle.rs:41

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
GlError copy_async(void *dst, const void *src, uint64_t bytes, bool to_host, void *ctx);
GlError stream_sync(void *ctx);

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

// What one proof of a handle on a context sets up before its flow begins, in this order: the context's device becomes current
// (every allocation of the proof follows it, whatever device the calling thread had), the handle's pool of this context serves
// every DevBuf, the spans of the small data are taken, and begin() allocates the one device buffer D and its page-locked mirror H.
struct ProofSession {
    DeviceCall device;
    void *ctx;
    Pool *pool;
    PoolScope pool_scope;
    SmallData sd;
    Stages st;
    DevBuf small;
    uint64_t *D = nullptr, *H = nullptr;
    ProofSession(const ProverShape &shape, double *h_stage_ms, void *c) : device(c), ctx(c), pool(shape.pool_of(c)), pool_scope(pool), st(h_stage_ms, c) {}
    Span take(uint64_t words) { return sd.take(words); }
    GlError begin() {  // after the last take()
        TRY(small.alloc(sd.top));
        D = small.p;
        return pool->staging(sd.top, &H);
    }
    GlError fetch(const Span &sp) { return copy_async(H + sp.off, D + sp.off, sp.words * 8, true, ctx); }
    GlError upload(const Span &sp) { return copy_async(D + sp.off, H + sp.off, sp.words * 8, false, ctx); }
    GlError sync() { return stream_sync(ctx); }
    // one gl_challenger_step of the Challenger at `transcript`: observe srcs, then draw n_out challenges (with GL_CHALLENGER_HASH: the hash) at `out`
    GlError step(const Span &transcript, const std::vector<GlObserveSrc> &srcs, uint32_t n_out, const Span &out, uint32_t flags = 0) {
        return gl_challenger_step(D + transcript.off, srcs.data(), (uint32_t)srcs.size(), n_out, n_out || (flags & GL_CHALLENGER_HASH) ? D + out.off : nullptr,
                                  flags, ctx);
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

GlError fri_shapes(const ProverShape &c, FriLayout *L);
// after fri_shapes; leaf_len: of every oracle, salt included
void fri_layout(const ProverShape &c, const std::vector<uint32_t> &leaf_len, SmallData *sd, FriLayout *L);
// From the FRI alpha to the query openings; marks stages 6 (combine), 7 (commit phase), 8 (proof of work). The caller fetches
// everything, synchronises, marks stage 9 and calls fri_check_pow / fri_write.
GlError fri_prove(const ProverShape &c, const FriLayout &L, ProofSession &s, const Span &T, const std::vector<const Batch *> &oracles,
                  const std::vector<GlObserveSrc> &opening_srcs, const std::vector<FriBatch> &batches, uint64_t *pow_witness);
GlError fri_check_pow(const ProverShape &c, const FriLayout &L, const uint64_t *H, uint64_t pow_witness);
// write_fri_proof (util/serialization.rs:591-639)
void fri_write(Bytes &out, const ProverShape &c, const FriLayout &L, const uint64_t *H, const std::vector<const Batch *> &oracles, uint64_t pow_witness);
GlError bytes_out(const Bytes &out, uint8_t **proof, uint64_t *proof_len);

// ---- transcript: device-resident (gl_challenger_step), see prove_impl; gl_circuit_create hashes a few host words once ----
GlError hash_no_pad(const uint64_t *in, size_t n, uint64_t out[4], void *ctx);  // hash/hashing.rs:81-108
// BytesHash<25>::to_vec (hash/hash_types.rs:179-189) of one digest slot: chunks of 7, 7, 7 and 4 bytes, little endian
void keccak_to_vec(const uint64_t slot[4], uint64_t out[4]);
// KeccakHash<25>::hash_no_pad of a few host words, on the device (gl_keccak_hash_no_pad_batch); out = one digest slot
GlError keccak_hash_no_pad(const std::vector<uint64_t> &in, uint64_t out[4], void *ctx);

// d_salt: SALT_SIZE columns of n_ext caller-provided random elements in leaf order (a blinded commitment, prover.rs:84, 125, 174), or null
GlError commit(Batch *b, DevBuf &&polys, bool from_values, uint32_t n_polys, const ProverShape &c, void *ctx, const uint64_t *d_salt = nullptr,
               bool fetch_cap = true);
// a caller's matrix of n_polys value columns, copied into a pool buffer (the caller's stays intact) and committed from values
GlError commit_copy(Batch *b, const uint64_t *d_src, uint32_t n_polys, const ProverShape &c, void *ctx, const uint64_t *d_salt);
// trim_to_len(degree * qdf) of nch quotients of n << qdb coefficients, the split into degree-n chunks (plonk/prover.rs:153-166, starky
// prover.rs:124-133) and their commit from coefficients. Those from qdf * n on must vanish: there are some only when qdf is no power of two.
GlError commit_quotient_chunks(Batch *b, DevBuf &&quotient, uint32_t nch, uint32_t qdf, uint32_t qdb, const ProverShape &c, void *ctx, const uint64_t *d_salt);

// KeccakHash<25>::hash_or_noop panics on a leaf of exactly four elements (a 32-byte slice of a 25-byte vector, plonk/config.rs:
// 56-63): the refusal of a Keccak handle one of whose commitments or FRI layers has such leaves, or ok()
GlError keccak_leaf_error(uint32_t hasher, std::initializer_list<std::pair<const char *, uint32_t>> names_and_leaf_lens, const GlFriParams &fri);
GlError struct_size_error(const char *name);

}  // namespace plonky2_hip
