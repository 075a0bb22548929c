// plonky2_hip.hpp — header-only C++ mirror of the reference's operator interface for the hot path,
// over the C ABI of plonky2_hip.h. Same names and argument meaning as the Rust side:
//   PolynomialBatch::from_values / from_coeffs / get_lde_values   (plonky2/src/fri/oracle.rs:709-731, 911-1018)
//   MerkleTree::new_ / prove, MerkleCap                            (plonky2/src/hash/merkle_tree.rs:283-319, 392-440)
//   fft_with_options / ifft_with_options                           (field/src/fft.rs:58-103)
//   Circuit (gl_circuit_create_h) / Circuit::prove                 (plonk/circuit_builder.rs:849-960, plonk/prover.rs:40-233)
// Host containers are std::vector<uint64_t>; everything else stays in HBM. Errors (the reference
// panics or drops them) become plonky2_hip::Error exceptions. No CPU fallback exists.
#pragma once
#include <array>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "plonky2_hip.h"

namespace plonky2_hip {

constexpr uint64_t ORDER = 0xFFFFFFFF00000001ULL;  // goldilocks_field.rs:133
constexpr uint64_t COSET_SHIFT = 7;                // Field::coset_shift, types.rs:431-433
constexpr uint32_t SALT_SIZE = 4;                  // fri/oracle.rs:41

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error("plonky2_hip error " + std::to_string(c) + ": " + m), code(c) {}
};

inline void check(GlError e) {
    if (e.code == 0) return;
    std::string msg = e.message ? e.message : cudaGetErrorString(e.code);
    if (e.message) std::free(e.message);
    throw Error(e.code, msg);
}

// Two HIP streams on one device (CudaInnerContext, fri/oracle.rs:43-47).
class Context {
  public:
    explicit Context(int device = 0) : ptr_(gl_ctx_create(device)) {
        if (!ptr_) throw Error(GL_E_INVALID, "gl_ctx_create failed (no HIP device?)");
    }
    ~Context() { gl_ctx_destroy(ptr_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    void *get() const { return ptr_; }
    void synchronize() const { check(gl_ctx_synchronize(ptr_)); }

  private:
    void *ptr_;
};

// n u64 field elements in HBM.
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    DeviceBuffer(const Context &ctx, uint64_t n) : ctx_(&ctx), n_(n) {
        void *p = nullptr;
        check(gl_ctx_malloc(&p, n * 8, ctx.get()));
        ptr_ = static_cast<uint64_t *>(p);
    }
    DeviceBuffer(const Context &ctx, const std::vector<uint64_t> &host) : DeviceBuffer(ctx, host.size()) { upload(host); }
    DeviceBuffer(DeviceBuffer &&o) noexcept { *this = std::move(o); }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
        release();
        ctx_ = o.ctx_; ptr_ = o.ptr_; n_ = o.n_;
        o.ptr_ = nullptr; o.n_ = 0;
        return *this;
    }
    ~DeviceBuffer() { release(); }
    uint64_t *data() const { return ptr_; }
    uint64_t size() const { return n_; }
    void upload(const std::vector<uint64_t> &host, uint64_t offset = 0) {
        if (offset + host.size() > n_) throw Error(GL_E_INVALID, "upload out of range");
        if (!host.empty()) check(gl_memcpy_h2d(ptr_ + offset, host.data(), host.size() * 8, ctx_->get()));
    }
    std::vector<uint64_t> download(uint64_t offset, uint64_t count) const {
        if (offset + count > n_) throw Error(GL_E_INVALID, "download out of range");
        std::vector<uint64_t> out(count);
        if (count) check(gl_memcpy_d2h(out.data(), ptr_ + offset, count * 8, ctx_->get()));
        return out;
    }
    std::vector<uint64_t> download() const { return download(0, n_); }

  private:
    void release() {
        if (ptr_) gl_free(ptr_);
        ptr_ = nullptr;
    }
    const Context *ctx_ = nullptr;
    uint64_t *ptr_ = nullptr;
    uint64_t n_ = 0;
};

inline uint32_t log2_strict(uint64_t n) {
    uint32_t l = 0;
    while ((1ull << l) < n) l++;
    if ((1ull << l) != n) throw Error(GL_E_INVALID, "not a power of two");  // util/src/lib.rs log2_strict panics
    return l;
}

// fft_with_options(poly, zero_factor, root_table): the last two are performance hints in the
// reference (fft.rs:203-217) and are not needed here. polys: n_polys rows of length n.
inline std::vector<uint64_t> fft_with_options(const Context &ctx, const std::vector<uint64_t> &polys, uint64_t n_polys) {
    uint64_t n = polys.size() / n_polys;
    DeviceBuffer d(ctx, polys);
    check(gl_ntt_batch(d.data(), n_polys, log2_strict(n), n, 0, 0, ctx.get()));
    return d.download();
}

inline std::vector<uint64_t> ifft_with_options(const Context &ctx, const std::vector<uint64_t> &polys, uint64_t n_polys) {
    uint64_t n = polys.size() / n_polys;
    DeviceBuffer d(ctx, polys);
    check(gl_ntt_batch(d.data(), n_polys, log2_strict(n), n, 1, 0, ctx.get()));
    return d.download();
}

using HashOut = std::vector<uint64_t>;  // 4 elements (hash_types.rs:17-22); a Keccak hash: the first 25 bytes of the 4 words

// The hasher of a Merkle tree: PoseidonGoldilocksConfig or KeccakGoldilocksConfig (plonk/config.rs:110-128).
enum class Hasher : uint32_t { Poseidon = GL_HASHER_POSEIDON, Keccak = GL_HASHER_KECCAK25 };

// BytesHash<25> of a digest slot (hash_types.rs:133-137): bytes 0..24 of its four little-endian words.
inline std::vector<uint8_t> keccak_hash_bytes(const uint64_t *slot) {
    std::vector<uint8_t> out(25);
    for (int i = 0; i < 25; i++) out[i] = (uint8_t)(slot[i / 8] >> (8 * (i % 8)));
    return out;
}

struct MerkleProof {
    std::vector<HashOut> siblings;  // merkle_proofs.rs:18-22
};

class MerkleTree {
  public:
    // MerkleTree::new(leaves, cap_height) (merkle_tree.rs:283-319); leaves leaf-major [n_leaves][leaf_len].
    // hasher: Poseidon (the default) or Keccak; the buffers, indices and prove() are the same for both.
    static MerkleTree new_(const Context &ctx, const std::vector<uint64_t> &leaves, uint64_t n_leaves, uint32_t cap_height,
                           Hasher hasher = Hasher::Poseidon) {
        uint32_t lg = log2_strict(n_leaves);
        if (cap_height > lg)
            throw Error(GL_E_INVALID, "cap_height=" + std::to_string(cap_height) + " should be at most log2(leaves.len())=" + std::to_string(lg));
        MerkleTree t;
        t.ctx_ = &ctx;
        t.n_leaves_ = n_leaves;
        t.leaf_len_ = (uint32_t)(leaves.size() / n_leaves);
        t.cap_height_ = cap_height;
        t.d_leaves_ = DeviceBuffer(ctx, leaves);
        t.d_digests_ = DeviceBuffer(ctx, 8 * (n_leaves - (1ull << cap_height)) + 4);
        t.d_cap_ = DeviceBuffer(ctx, 4ull << cap_height);
        t.hasher_ = hasher;
        if (hasher == Hasher::Poseidon)
            check(gl_merkle_tree_from_leaves(t.d_leaves_.data(), t.leaf_len_, n_leaves, cap_height, t.d_digests_.data(),
                                             t.d_cap_.data(), ctx.get()));
        else
            check(gl_merkle_tree_from_leaves_h((uint32_t)hasher, t.d_leaves_.data(), t.leaf_len_, n_leaves, cap_height, t.d_digests_.data(),
                                               t.d_cap_.data(), ctx.get()));
        return t;
    }
    // adopt buffers produced by a commit
    static MerkleTree adopt(const Context &ctx, uint64_t n_leaves, uint32_t leaf_len, uint32_t cap_height, DeviceBuffer digests,
                            DeviceBuffer cap, DeviceBuffer leaves, Hasher hasher = Hasher::Poseidon) {
        MerkleTree t;
        t.hasher_ = hasher;
        t.ctx_ = &ctx; t.n_leaves_ = n_leaves; t.leaf_len_ = leaf_len; t.cap_height_ = cap_height;
        t.d_digests_ = std::move(digests); t.d_cap_ = std::move(cap); t.d_leaves_ = std::move(leaves);
        return t;
    }
    uint64_t num_digests() const { return 2 * (n_leaves_ - (1ull << cap_height_)); }
    std::vector<uint64_t> cap() const { return d_cap_.download(0, 4ull << cap_height_); }
    std::vector<uint64_t> digests() const { return d_digests_.download(0, 4 * num_digests()); }
    std::vector<uint64_t> get(uint64_t i) const { return d_leaves_.download(i * leaf_len_, leaf_len_); }  // merkle_tree.rs:385-391
    // MerkleTree::prove (merkle_tree.rs:392-440)
    MerkleProof prove(uint64_t leaf_index) const {
        uint32_t num_layers = log2_strict(n_leaves_) - cap_height_;
        uint64_t tree_len = num_digests() >> cap_height_;
        uint64_t tree_index = leaf_index >> num_layers;
        uint64_t pair_index = leaf_index & ((1ull << num_layers) - 1);
        MerkleProof p;
        for (uint32_t i = 0; i < num_layers; i++) {
            uint64_t parity = pair_index & 1;
            pair_index >>= 1;
            uint64_t siblings_index = (pair_index << (i + 1)) + (1ull << i) - 1;
            uint64_t sibling_index = 2 * siblings_index + (1 - parity);
            p.siblings.push_back(d_digests_.download(4 * (tree_len * tree_index + sibling_index), 4));
        }
        return p;
    }
    uint64_t n_leaves() const { return n_leaves_; }
    uint32_t leaf_len() const { return leaf_len_; }
    Hasher hasher() const { return hasher_; }

  private:
    Hasher hasher_ = Hasher::Poseidon;
    const Context *ctx_ = nullptr;
    uint64_t n_leaves_ = 0;
    uint32_t leaf_len_ = 0, cap_height_ = 0;
    DeviceBuffer d_leaves_, d_digests_, d_cap_;
};

// PolynomialBatch (fri/oracle.rs:112-120): coefficients, LDE and tree stay resident in HBM.
class PolynomialBatch {
  public:
    // from_values(values, rate_bits, blinding, cap_height, timing, fft_root_table) (oracle.rs:709-731).
    // values: n_polys columns of length n, column-major. `salt` = SALT_SIZE columns of n<<rate_bits
    // elements when blinding (the reference draws them from OsRng, oracle.rs:998-1002).
    static PolynomialBatch from_values(const Context &ctx, const std::vector<uint64_t> &values, uint64_t n_polys, uint32_t rate_bits,
                                       bool blinding, uint32_t cap_height, const std::vector<uint64_t> &salt = {},
                                       Hasher hasher = Hasher::Poseidon) {
        return commit(ctx, values, n_polys, rate_bits, blinding, cap_height, salt, true, hasher);
    }
    // from_coeffs (oracle.rs:911-977)
    static PolynomialBatch from_coeffs(const Context &ctx, const std::vector<uint64_t> &coeffs, uint64_t n_polys, uint32_t rate_bits,
                                       bool blinding, uint32_t cap_height, const std::vector<uint64_t> &salt = {},
                                       Hasher hasher = Hasher::Poseidon) {
        return commit(ctx, coeffs, n_polys, rate_bits, blinding, cap_height, salt, false, hasher);
    }
    std::vector<uint64_t> polynomials() const { return d_polys_.download(); }
    // get_lde_values(index, step) (oracle.rs:1007-1018)
    std::vector<uint64_t> get_lde_values(uint64_t index, uint64_t step = 1) const {
        uint64_t idx = index * step, bits = degree_log + rate_bits, rev = 0;
        for (uint64_t b = 0; b < bits; b++) rev |= ((idx >> b) & 1) << (bits - 1 - b);
        std::vector<uint64_t> row = merkle_tree.get(rev);
        row.resize(row.size() - (blinding ? SALT_SIZE : 0));
        return row;
    }
    MerkleTree merkle_tree;
    uint32_t degree_log = 0, rate_bits = 0;
    bool blinding = false;

  private:
    static PolynomialBatch commit(const Context &ctx, const std::vector<uint64_t> &polys, uint64_t n_polys, uint32_t rate_bits,
                                  bool blinding, uint32_t cap_height, const std::vector<uint64_t> &salt, bool is_values, Hasher hasher) {
        uint64_t n = polys.size() / n_polys;
        uint32_t lg = log2_strict(n);
        uint64_t n_ext = n << rate_bits;
        uint32_t salt_size = blinding ? SALT_SIZE : 0;
        if (cap_height > lg + rate_bits) throw Error(GL_E_INVALID, "cap_height should be at most log2(leaves.len())");
        if (salt.size() != (uint64_t)salt_size * n_ext) throw Error(GL_E_INVALID, "blinding needs SALT_SIZE columns of salt");
        uint64_t cols = n_polys + salt_size;
        PolynomialBatch b;
        b.degree_log = lg; b.rate_bits = rate_bits; b.blinding = blinding;
        b.d_polys_ = DeviceBuffer(ctx, polys);
        b.d_lde_ = DeviceBuffer(ctx, cols * n_ext);
        if (salt_size) b.d_lde_.upload(salt, n_polys * n_ext);
        DeviceBuffer leaves(ctx, cols * n_ext), dig(ctx, 8 * (n_ext - (1ull << cap_height)) + 4), cap(ctx, 4ull << cap_height);
        if (hasher == Hasher::Poseidon)
            check((is_values ? gl_commit_from_values : gl_commit_from_coeffs_nc)(b.d_polys_.data(), n_polys, lg, rate_bits, cap_height, salt_size,
                                                                                  COSET_SHIFT, b.d_lde_.data(), leaves.data(), dig.data(),
                                                                                  cap.data(), ctx.get()));
        else
            check((is_values ? gl_commit_from_values_h : gl_commit_from_coeffs_h_nc)((uint32_t)hasher, b.d_polys_.data(), n_polys, lg, rate_bits,
                                                                                      cap_height, salt_size, COSET_SHIFT, b.d_lde_.data(),
                                                                                      leaves.data(), dig.data(), cap.data(), ctx.get()));
        ctx.synchronize();
        b.merkle_tree = MerkleTree::adopt(ctx, n_ext, (uint32_t)cols, cap_height, std::move(dig), std::move(cap), std::move(leaves), hasher);
        return b;
    }
    static GlError gl_commit_from_coeffs_nc(uint64_t *c, uint64_t p, uint32_t l, uint32_t r, uint32_t h, uint32_t s, uint64_t sh, uint64_t *lde,
                                            uint64_t *lv, uint64_t *dg, uint64_t *cp, void *ctx) {
        return gl_commit_from_coeffs(c, p, l, r, h, s, sh, lde, lv, dg, cp, ctx);
    }
    static GlError gl_commit_from_coeffs_h_nc(uint32_t hs, uint64_t *c, uint64_t p, uint32_t l, uint32_t r, uint32_t h, uint32_t s, uint64_t sh,
                                              uint64_t *lde, uint64_t *lv, uint64_t *dg, uint64_t *cp, void *ctx) {
        return gl_commit_from_coeffs_h(hs, c, p, l, r, h, s, sh, lde, lv, dg, cp, ctx);
    }
    DeviceBuffer d_polys_, d_lde_;
};

// The circuit handle of the native prover (plonky2_hip.h "the whole prover in two calls"): gl_circuit_create_h on construction —
// `hasher` is the GenericConfig's Hasher, which builds every Merkle tree of the circuit and its proofs — gl_circuit_destroy on
// destruction. prove() = gl_prove: the proof in the reference's wire format (write_proof_with_public_inputs) for that config.
class Circuit {
  public:
    Circuit(const Context &ctx, const GlCircuitDesc &desc, Hasher hasher = Hasher::Poseidon) : hasher_(hasher), cap_height_(desc.fri.cap_height) {
        check(gl_circuit_create_h((uint32_t)hasher, &desc, &ptr_, ctx.get()));
    }
    ~Circuit() {
        if (ptr_) gl_circuit_destroy(ptr_);
    }
    Circuit(const Circuit &) = delete;
    Circuit &operator=(const Circuit &) = delete;
    void *get() const { return ptr_; }
    Hasher hasher() const { return hasher_; }
    // VerifierOnlyCircuitData: one 4-word slot per hash (Keccak: keccak_hash_bytes(slot))
    HashOut circuit_digest() const {
        HashOut d(4);
        check(gl_circuit_info(ptr_, d.data(), nullptr));
        return d;
    }
    std::vector<uint64_t> constants_sigmas_cap() const {
        std::vector<uint64_t> cap(4ull << cap_height_);
        check(gl_circuit_info(ptr_, nullptr, cap.data()));
        return cap;
    }
    // d_wires: [num_wires][2^degree_bits] in HBM; d_salts: the blinding of a hiding circuit (gl_prove_zk), else null
    std::vector<uint8_t> prove(const Context &ctx, const uint64_t *d_wires, const std::vector<uint64_t> &public_inputs,
                               const uint64_t *d_salts = nullptr) const {
        uint8_t *bytes = nullptr;
        uint64_t len = 0;
        const uint64_t *pis = public_inputs.empty() ? nullptr : public_inputs.data();
        if (d_salts)
            check(gl_prove_zk(ptr_, d_wires, pis, (uint32_t)public_inputs.size(), d_salts, &bytes, &len, nullptr, ctx.get()));
        else
            check(gl_prove(ptr_, d_wires, pis, (uint32_t)public_inputs.size(), &bytes, &len, nullptr, ctx.get()));
        std::vector<uint8_t> out(bytes, bytes + len);
        gl_bytes_free(bytes);
        return out;
    }

  private:
    void *ptr_ = nullptr;
    Hasher hasher_;
    uint32_t cap_height_;
};

// The STARK handle (plonky2_hip.h "STARKs: starky's prove() in two calls"): gl_stark_create on construction, gl_stark_destroy on
// destruction. prove() = gl_stark_prove: StarkProofWithPublicInputs in the wire format the header defines.
class Stark {
  public:
    Stark(const Context &ctx, const GlStarkDesc &desc, Hasher hasher = Hasher::Poseidon) : num_public_inputs_(desc.num_public_inputs) {
        check(gl_stark_create((uint32_t)hasher, &desc, &ptr_, ctx.get()));
    }
    ~Stark() {
        if (ptr_) gl_stark_destroy(ptr_);
    }
    Stark(const Stark &) = delete;
    Stark &operator=(const Stark &) = delete;
    void *get() const { return ptr_; }
    // d_trace: [num_columns][2^degree_bits] value columns in HBM
    std::vector<uint8_t> prove(const Context &ctx, const uint64_t *d_trace, const std::vector<uint64_t> &public_inputs) const {
        if (public_inputs.size() != num_public_inputs_) throw std::invalid_argument("Stark::prove: wrong number of public inputs");
        uint8_t *bytes = nullptr;
        uint64_t len = 0;
        check(gl_stark_prove(ptr_, d_trace, public_inputs.empty() ? nullptr : public_inputs.data(), &bytes, &len, nullptr, ctx.get()));
        std::vector<uint8_t> out(bytes, bytes + len);
        gl_bytes_free(bytes);
        return out;
    }
    void trim() const { check(gl_stark_trim(ptr_)); }
    // gl_stark_compile: from now on the quotient runs a kernel generated from this STARK's description (the same values); only
    // between proofs. Throws with the compiler's log on failure; the handle then stays interpreted and usable.
    void compile(const Context &ctx) { check(gl_stark_compile(ptr_, ctx.get())); }
    bool is_compiled() const { return gl_stark_is_compiled(ptr_) != 0; }
    std::string kernel_source() const {
        const char *src = gl_stark_kernel_source(ptr_);
        return src ? src : "";
    }
    // gl_stark_precompile: validate, generate and compile into the kernel cache without a device (a build machine's step)
    static void precompile(const GlStarkDesc &desc, Hasher hasher = Hasher::Poseidon) { check(gl_stark_precompile((uint32_t)hasher, &desc)); }
    // gl_stark_compile_units / gl_stark_precompile_units: the same as several kernels of at most max_unit_instrs instructions
    // that run in order (0: the library's default cap) — what a long program needs to compile in reasonable time
    void compile_units(const Context &ctx, uint32_t max_unit_instrs = 0) { check(gl_stark_compile_units(ptr_, max_unit_instrs, ctx.get())); }
    uint32_t num_units() const { return (uint32_t)gl_stark_kernel_units(ptr_); }  // 0 while interpreted
    std::string unit_source(uint32_t unit) const {
        const char *src = gl_stark_kernel_unit_source(ptr_, unit);
        return src ? src : "";
    }
    static void precompile_units(const GlStarkDesc &desc, uint32_t max_unit_instrs = 0, Hasher hasher = Hasher::Poseidon) {
        check(gl_stark_precompile_units((uint32_t)hasher, &desc, max_unit_instrs));
    }

  private:
    void *ptr_ = nullptr;
    uint32_t num_public_inputs_;
};

// Several STARKs tied by cross-table lookups (plonky2_hip.h "Multi-table STARKs with cross-table lookups"): gl_stark_tables_create
// on construction, gl_stark_tables_destroy on destruction. prove() = gl_stark_tables_prove: the tables' StarkProofs in table order.
class StarkTables {
  public:
    StarkTables(const Context &ctx, const GlStarkTablesDesc &desc, Hasher hasher = Hasher::Poseidon) : num_tables_(desc.num_tables) {
        check(gl_stark_tables_create((uint32_t)hasher, &desc, &ptr_, ctx.get()));
    }
    ~StarkTables() {
        if (ptr_) gl_stark_tables_destroy(ptr_);
    }
    StarkTables(const StarkTables &) = delete;
    StarkTables &operator=(const StarkTables &) = delete;
    void *get() const { return ptr_; }
    // d_traces[k]: [num_columns][2^degree_bits] value columns of table k in HBM
    std::vector<uint8_t> prove(const Context &ctx, const std::vector<const uint64_t *> &d_traces) const {
        if (d_traces.size() != num_tables_) throw std::invalid_argument("StarkTables::prove: one trace per table");
        uint8_t *bytes = nullptr;
        uint64_t len = 0;
        check(gl_stark_tables_prove(ptr_, d_traces.data(), &bytes, &len, nullptr, ctx.get()));
        std::vector<uint8_t> out(bytes, bytes + len);
        gl_bytes_free(bytes);
        return out;
    }
    void trim() const { check(gl_stark_tables_trim(ptr_)); }
    // gl_stark_tables_compile: one generated quotient kernel per table, as Stark::compile; all tables or none
    void compile(const Context &ctx) { check(gl_stark_tables_compile(ptr_, ctx.get())); }
    bool is_compiled() const { return gl_stark_tables_is_compiled(ptr_) != 0; }
    std::string kernel_source(uint32_t table) const {
        const char *src = gl_stark_tables_kernel_source(ptr_, table);
        return src ? src : "";
    }
    static void precompile(const GlStarkTablesDesc &desc, Hasher hasher = Hasher::Poseidon) {
        check(gl_stark_tables_precompile((uint32_t)hasher, &desc));
    }
    // gl_stark_tables_compile_units / gl_stark_tables_precompile_units: every table in units, as Stark::compile_units
    void compile_units(const Context &ctx, uint32_t max_unit_instrs = 0) { check(gl_stark_tables_compile_units(ptr_, max_unit_instrs, ctx.get())); }
    uint32_t num_units(uint32_t table) const { return (uint32_t)gl_stark_tables_kernel_units(ptr_, table); }
    std::string unit_source(uint32_t table, uint32_t unit) const {
        const char *src = gl_stark_tables_kernel_unit_source(ptr_, table, unit);
        return src ? src : "";
    }
    static void precompile_units(const GlStarkTablesDesc &desc, uint32_t max_unit_instrs = 0, Hasher hasher = Hasher::Poseidon) {
        check(gl_stark_tables_precompile_units((uint32_t)hasher, &desc, max_unit_instrs));
    }

  private:
    void *ptr_ = nullptr;
    uint32_t num_tables_;
};

// The lookup columns of a trace (plonky2_hip.h "The lookup columns of a trace"). d_scratch: gl_lookup_scratch_bytes(n) bytes in HBM.
// lookups: (input, table, permuted input, permuted table) columns of d_trace; the two permuted columns are written on the
// context's stream, before a prove() of the same context reads them.
inline void fill_lookups(const Context &ctx, uint64_t *d_trace, uint64_t trace_stride, uint64_t n, uint32_t num_columns,
                         const std::vector<std::array<uint32_t, 4>> &lookups, void *d_scratch) {
    check(gl_stark_fill_lookups(d_trace, trace_stride, n, num_columns, lookups.empty() ? nullptr : lookups[0].data(), (uint32_t)lookups.size(),
                                d_scratch, ctx.get()));
}

// The Keccak-f table (plonky2_hip.h "The Keccak-f table"). keccak_table_trace: d_inputs [num_inputs][25] states -> d_trace
// [2430][trace_stride] with 2^degree_bits rows, on the context's stream. keccak_table_program: its constraints; the instructions
// and immediates are what GlStarkDesc.h_instrs / h_immediates take (constraint_degree 3, no public inputs, no pairs).
inline void keccak_table_trace(const Context &ctx, const uint64_t *d_inputs, uint64_t num_inputs, uint32_t degree_bits, uint64_t *d_trace,
                               uint64_t trace_stride) {
    check(gl_keccak_table_trace(d_inputs, num_inputs, degree_bits, d_trace, trace_stride, ctx.get()));
}
struct KeccakTableProgram {
    std::vector<GlGateInstr> instrs;
    std::vector<uint64_t> immediates;
    uint32_t num_constraints = 0;
};
inline KeccakTableProgram keccak_table_program() {
    GlGatePrograms p;
    check(gl_keccak_table_program(&p));
    KeccakTableProgram out;
    out.instrs.assign(p.instrs, p.instrs + p.num_instrs);
    out.immediates.assign(p.immediates, p.immediates + p.num_immediates);
    out.num_constraints = p.num_gate_constraints;
    gl_gate_programs_free(&p);
    return out;
}

// The memory table (plonky2_hip.h "The memory table"). memory_table_trace: d_ops [num_ops][14] unsorted operations -> d_trace
// [26][trace_stride] with 2^degree_bits rows; returns operations + dummies, which is all a call with d_trace == nullptr computes.
// d_scratch: gl_memory_table_scratch_bytes(num_ops, degree_bits) bytes in HBM. The call waits once, for the count; the trace is
// complete on the context's stream before a prove() of the same context reads it. memory_table_program: its constraints
// (constraint_degree 3, no public inputs, pairs (22, 24) and (23, 25)).
inline uint64_t memory_table_trace(const Context &ctx, const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                   uint64_t trace_stride, void *d_scratch) {
    uint64_t rows = 0;
    check(gl_memory_table_trace(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, &rows, ctx.get()));
    return rows;
}
using MemoryTableProgram = KeccakTableProgram;  // instructions, immediates and the number of constraints
inline MemoryTableProgram memory_table_program() {
    GlGatePrograms p;
    check(gl_memory_table_program(&p));
    MemoryTableProgram out;
    out.instrs.assign(p.instrs, p.instrs + p.num_instrs);
    out.immediates.assign(p.immediates, p.immediates + p.num_immediates);
    out.num_constraints = p.num_gate_constraints;
    gl_gate_programs_free(&p);
    return out;
}

// The logic table (plonky2_hip.h "The logic table"). logic_table_trace: d_ops [num_ops][17] records (operator, the limbs of the
// two inputs) -> d_trace [523][trace_stride] with 2^degree_bits rows, list order = row order, zero rows behind. d_scratch:
// GL_LOGIC_TABLE_SCRATCH_BYTES bytes in HBM, 16-byte aligned. The call waits once, for the validation (not at all with
// num_ops == 0); the trace is complete on the context's stream before a prove() of the same context reads it.
// logic_table_program: its constraints (constraint_degree 3, no public inputs, no pairs).
inline void logic_table_trace(const Context &ctx, const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                              uint64_t trace_stride, void *d_scratch) {
    check(gl_logic_table_trace(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, ctx.get()));
}
using LogicTableProgram = KeccakTableProgram;  // instructions, immediates and the number of constraints
inline LogicTableProgram logic_table_program() {
    GlGatePrograms p;
    check(gl_logic_table_program(&p));
    LogicTableProgram out;
    out.instrs.assign(p.instrs, p.instrs + p.num_instrs);
    out.immediates.assign(p.immediates, p.immediates + p.num_immediates);
    out.num_constraints = p.num_gate_constraints;
    gl_gate_programs_free(&p);
    return out;
}

// The Keccak sponge table (plonky2_hip.h "The Keccak sponge table"). keccak_sponge_table_trace: d_ops [num_ops][5] records
// (context, segment, virt, timestamp, len) and the concatenated input bytes -> d_trace [414][trace_stride] with 2^degree_bits
// rows; returns the rows the operations take, which is all a call with d_trace == nullptr computes. d_scratch:
// gl_keccak_sponge_table_scratch_bytes(num_ops, degree_bits) bytes in HBM. The call waits once, for the count.
// keccak_sponge_table_ops: from the finished trace, the records gl_keccak_table_trace, gl_logic_table_trace and
// gl_memory_table_trace take; any output may be nullptr. keccak_sponge_table_program: the reference's to-do list of constraints
// written out (constraint_degree 3, no public inputs, no pairs).
inline uint64_t keccak_sponge_table_trace(const Context &ctx, const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint32_t degree_bits,
                                          uint64_t *d_trace, uint64_t trace_stride, void *d_scratch) {
    uint64_t rows = 0;
    check(gl_keccak_sponge_table_trace(d_ops, num_ops, d_bytes, degree_bits, d_trace, trace_stride, d_scratch, &rows, ctx.get()));
    return rows;
}
inline void keccak_sponge_table_ops(const Context &ctx, const uint64_t *d_trace, uint64_t trace_stride, uint32_t degree_bits, uint64_t rows,
                                    uint64_t *d_keccak_inputs, uint64_t *d_logic_ops, uint64_t *d_memory_ops, void *d_scratch) {
    check(gl_keccak_sponge_table_ops(d_trace, trace_stride, degree_bits, rows, d_keccak_inputs, d_logic_ops, d_memory_ops, d_scratch, ctx.get()));
}
using KeccakSpongeTableProgram = KeccakTableProgram;  // instructions, immediates and the number of constraints
inline KeccakSpongeTableProgram keccak_sponge_table_program() {
    GlGatePrograms p;
    check(gl_keccak_sponge_table_program(&p));
    KeccakSpongeTableProgram out;
    out.instrs.assign(p.instrs, p.instrs + p.num_instrs);
    out.immediates.assign(p.immediates, p.immediates + p.num_immediates);
    out.num_constraints = p.num_gate_constraints;
    gl_gate_programs_free(&p);
    return out;
}

// The arithmetic table (plonky2_hip.h "The arithmetic table"). arithmetic_table_trace: d_ops [num_ops][25] records (operator, the
// limbs of in0, in1, in2) -> d_trace [92][trace_stride] with 2^degree_bits rows; returns the rows the operations take, which is
// all a call with d_trace == nullptr computes. d_scratch: gl_arithmetic_table_scratch_bytes(num_ops, degree_bits) bytes in HBM.
// The call waits once, for the count. arithmetic_table_program: its constraints (declare constraint_degree 5 where a DIV row may
// exist; no public inputs, no pairs).
inline uint64_t arithmetic_table_trace(const Context &ctx, const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                       uint64_t trace_stride, void *d_scratch) {
    uint64_t rows = 0;
    check(gl_arithmetic_table_trace(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, &rows, ctx.get()));
    return rows;
}
using ArithmeticTableProgram = KeccakTableProgram;  // instructions, immediates and the number of constraints
inline ArithmeticTableProgram arithmetic_table_program() {
    GlGatePrograms p;
    check(gl_arithmetic_table_program(&p));
    ArithmeticTableProgram out;
    out.instrs.assign(p.instrs, p.instrs + p.num_instrs);
    out.immediates.assign(p.immediates, p.immediates + p.num_immediates);
    out.num_constraints = p.num_gate_constraints;
    gl_gate_programs_free(&p);
    return out;
}

// The Poseidon table (plonky2_hip.h "The Poseidon table"). poseidon_table_trace: d_ops [num_ops][13] records (the kind — 0 START,
// k = 1 .. 8 ABSORB of k elements into the row before — and twelve element words, any u64) -> d_trace [249][trace_stride] with
// 2^degree_bits rows, list order = row order, behind them the permutation of the all-zero state with IS_REAL = 0. d_scratch:
// GL_POSEIDON_TABLE_SCRATCH_BYTES bytes in HBM, 16-byte aligned. The call waits once, for the validation (not at all with
// num_ops == 0). poseidon_table_program: its constraints (constraint_degree 3, no public inputs, no pairs).
inline void poseidon_table_trace(const Context &ctx, const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                 uint64_t trace_stride, void *d_scratch) {
    check(gl_poseidon_table_trace(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, ctx.get()));
}
using PoseidonTableProgram = KeccakTableProgram;  // instructions, immediates and the number of constraints
inline PoseidonTableProgram poseidon_table_program() {
    GlGatePrograms p;
    check(gl_poseidon_table_program(&p));
    PoseidonTableProgram out;
    out.instrs.assign(p.instrs, p.instrs + p.num_instrs);
    out.immediates.assign(p.immediates, p.immediates + p.num_immediates);
    out.num_constraints = p.num_gate_constraints;
    gl_gate_programs_free(&p);
    return out;
}

// gl_stark_split_program: the unit programs gl_stark_compile_units cuts desc's program into (device-free). Every unit is a
// program of its own over desc's immediates; its EMITs are numbers emit_start .. emit_end - 1 of the program's.
struct StarkProgramUnit {
    std::vector<GlGateInstr> instrs;
    uint32_t emit_start = 0, emit_end = 0;
};
inline std::vector<StarkProgramUnit> stark_split_program(const GlStarkDesc &desc, uint32_t max_unit_instrs = 0) {
    GlGatePrograms p;
    check(gl_stark_split_program(&desc, max_unit_instrs, &p));
    std::vector<StarkProgramUnit> out(p.num_gates);
    for (uint32_t k = 0; k < p.num_gates; k++) {
        out[k].instrs.assign(p.instrs + p.gates[k].prog_start, p.instrs + p.gates[k].prog_start + p.gates[k].prog_len);
        out[k].emit_start = p.gates[k].group_start, out[k].emit_end = p.gates[k].group_end;
    }
    gl_gate_programs_free(&p);
    return out;
}

}  // namespace plonky2_hip
