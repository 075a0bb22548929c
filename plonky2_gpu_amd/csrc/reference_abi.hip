// reference_abi.hip — the seven symbols of the reference's boundary (cuda/src/lib.rs:58-145) over this library's entry points, and
// what only they need: the ed25519 circuit's gate kernel and the staging buffer of compute_quotient_polys (gl_reference_*).
#include <mutex>
#include <string>

#include <stdlib.h>

#include "commit.h"
#include "gl_field.h"
#include "knobs.h"
#include "merkle.h"
#include "plonk.h"
#include "ed25519_gate_program.inc"

using namespace plonky2_hip;

namespace {

// The gate kernel of the one circuit the reference's compute_quotient_polys is compiled for (ed25519_gate_program.inc).
// A cold hiprtc build of it takes about a minute (gate_jit.hip keeps compiled code objects under
// $PLONKY2_HIP_KERNEL_CACHE; comgr's own cache cuts a repeat to ~2 s), so this has its own lock: table lookups of
// other threads do not wait for it.
std::mutex g_ref_mu;
uint64_t g_ref_pih[4] = {ED25519_REFERENCE_PUBLIC_INPUTS_HASH[0], ED25519_REFERENCE_PUBLIC_INPUTS_HASH[1],
                         ED25519_REFERENCE_PUBLIC_INPUTS_HASH[2], ED25519_REFERENCE_PUBLIC_INPUTS_HASH[3]};

GlError get_ed25519_kernel(const GateKernel **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ref_mu);
    DeviceState &st = device_state(dev);
    if (!st.ed25519_kernel) {
        std::string err;
        st.ed25519_kernel = gate_kernel_build(ED25519_INSTRS, ED25519_NUM_INSTRS, ED25519_GATES, ED25519_NUM_GATES, ED25519_IMMEDIATES,
                                              ED25519_NUM_IMMEDIATES, ED25519_NUM_SELECTORS, ED25519_NUM_GATE_CONSTRAINTS,
                                              ED25519_NUM_CHALLENGES, &err);
        if (!st.ed25519_kernel) return fail(GL_E_INVALID, "compute_quotient_polys: building the ed25519 gate kernel failed: " + err);
    }
    *out = st.ed25519_kernel;
    return ok();
}

__global__ void bit_reverse_columns_kernel(uint64_t *v, uint32_t log_n, uint64_t total) {
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    uint64_t n = 1ull << log_n, i = g & (n - 1), base = g - i;
    uint64_t j = log_n ? (__brevll(i) >> (64 - log_n)) : 0;
    if (i < j) {
        uint64_t a = v[base + i], b = v[base + j];
        v[base + i] = b;
        v[base + j] = a;
    }
}

}  // namespace

extern "C" {

void init(void) {
    if (hipSetDevice(0) != hipSuccess) return;
    const NttTables *tb;
    (void)device_tables(0, &tb);
}

GlError ifft(uint64_t *d_values_flatten, int poly_num, int values_num_per_poly, int log_len,
             const uint64_t *d_root_table, const uint64_t *n_inv, void *ctx) {
    DeviceCall device_call(ctx);
    (void)d_root_table;
    if (poly_num < 0 || log_len < 0 || values_num_per_poly != (1 << log_len)) return fail(GL_E_INVALID, "bad sizes");
    if (n_inv) {
        uint64_t expect = glh::P - ((glh::P - 1) >> log_len);
        if (*n_inv % glh::P != expect) return fail(GL_E_INVALID, "n_inv does not equal 2^-log_len");
    }
    GlError e = gl_ntt_batch(d_values_flatten, (uint64_t)poly_num, (uint32_t)log_len, (uint64_t)values_num_per_poly, 1, 0, ctx);
    if (e.code) return e;
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    return ok();
}

GlError merkle_tree_from_coeffs(uint64_t *d_values_flatten, uint64_t *d_ext_values_flatten, int poly_num,
                                int values_num_per_poly, int log_len, const uint64_t *d_root_table,
                                const uint64_t *d_root_table2, const uint64_t *d_shift_powers, int rate_bits,
                                int salt_size, int cap_height, int pad_extvalues_len, void *ctx) {
    DeviceCall device_call(ctx);
    (void)d_root_table;
    (void)d_root_table2;
    (void)d_shift_powers;
    if (poly_num <= 0 || log_len < 0 || rate_bits < 0 || salt_size < 0 || cap_height < 0 || pad_extvalues_len < 0 ||
        values_num_per_poly != (1 << log_len))
        return fail(GL_E_INVALID, "bad sizes");
    if (log_len > 24) return fail(GL_E_INVALID, "log_len > 24 is not supported by this build");
    const uint64_t n_ext = (uint64_t)values_num_per_poly << rate_bits;
    const uint64_t ext_polys = (uint64_t)poly_num + salt_size;
    if ((uint64_t)pad_extvalues_len < ext_polys * n_ext)
        return fail(GL_E_INVALID, "pad_extvalues_len smaller than (poly_num+salt_size)*n_ext: regions would overlap");
    uint64_t *region_b = d_ext_values_flatten + pad_extvalues_len;
    uint64_t *digests = region_b + ext_polys * n_ext;
    uint64_t num_digests = 2 * (n_ext - (1ull << cap_height));
    GlError e = commit_from_coeffs(GL_HASHER_POSEIDON, d_values_flatten, (uint64_t)poly_num, (uint32_t)log_len, (uint32_t)rate_bits,
                                   (uint32_t)cap_height, (uint32_t)salt_size, 7, region_b, d_ext_values_flatten, digests,
                                   digests + 4 * num_digests, S(ctx));
    if (e.code) return e;
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    // the reference's body ends its hashing with cudaStreamSynchronize(ctx->stream2) (plonky2_gpu.cu:586) and its caller reads the
    // destination of the copy it queued there as soon as this returns (fri/oracle.rs:403-407, 462): stream order already put
    // that copy before the first write of region A; this makes its completion visible to the host as well
    if (!PLONKY2_KNOB("PLONKY2_DROP_STREAM2_WAIT")) HIP_TRY(hipStreamSynchronize(S(ctx)->stream2));
    return ok();
}

GlError merkle_tree_from_values(uint64_t *d_values_flatten, uint64_t *d_ext_values_flatten, int poly_num,
                                int values_num_per_poly, int log_len, const uint64_t *d_root_table,
                                const uint64_t *d_root_table2, const uint64_t *d_shift_powers, const uint64_t *n_inv,
                                int rate_bits, int salt_size, int cap_height, int pad_extvalues_len, void *ctx) {
    DeviceCall device_call(ctx);
    GlError e = ifft(d_values_flatten, poly_num, values_num_per_poly, log_len, d_root_table, n_inv, ctx);
    if (e.code) return e;
    return merkle_tree_from_coeffs(d_values_flatten, d_ext_values_flatten, poly_num, values_num_per_poly, log_len,
                                   d_root_table, d_root_table2, d_shift_powers, rate_bits, salt_size, cap_height,
                                   pad_extvalues_len, ctx);
}

GlError build_merkle_tree(uint64_t *d_ext_values_flatten, int poly_num, int values_num_per_poly, int log_len,
                          int rate_bits, int salt_size, int cap_height, int pad_extvalues_len, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_ext_values_flatten) return fail(GL_E_INVALID, "null pointer");
    if (poly_num <= 0 || log_len < 0 || rate_bits < 0 || salt_size < 0 || cap_height < 0 || pad_extvalues_len < 0 ||
        values_num_per_poly != (1 << log_len) || cap_height > log_len + rate_bits)
        return fail(GL_E_INVALID, "bad sizes");
    const uint32_t log_ext = (uint32_t)(log_len + rate_bits);
    const uint64_t n_ext = 1ull << log_ext, ext_polys = (uint64_t)poly_num + salt_size;
    uint64_t *region_b = d_ext_values_flatten + pad_extvalues_len;
    uint64_t *digests = region_b + ext_polys * n_ext;
    uint64_t num_digests = 2 * (n_ext - (1ull << cap_height));
    uint64_t total = (uint64_t)poly_num * n_ext;  // plonky2_gpu.cu:159-161: salt columns are not permuted
    hipLaunchKernelGGL(bit_reverse_columns_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(ctx)->stream,
                       region_b, log_ext, total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(merkle_tree_from_columns(region_b, (uint32_t)ext_polys, n_ext, n_ext, (uint32_t)cap_height, digests,
                                     digests + 4 * num_digests, S(ctx)->stream));
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    return ok();
}

// Column-major staging for compute_quotient_polys: the reference's contract hands over LEAF-MAJOR rows, which the
// quotient kernels read with the row length (1872 B for the wires) as the stride between the lanes of a wave;
// transposing first (streaming, through LDS tiles) and reading column-major is 2x faster end to end. One buffer per
// device — the library's own, grown on demand and given back by gl_reference_quotient_release(), or the CALLER'S
// (gl_reference_quotient_set_staging: a host that sizes all device memory up front, fri/oracle.rs:94-106, keeps doing so and
// the library allocates nothing here). nullptr = could not allocate / the caller's buffer is too small, or
// PLONKY2_HIP_REFERENCE_IN_PLACE=1: read the rows in place. Called with the device's ref_mu held.
static uint64_t *get_ref_staging(DeviceState &st, uint64_t elems) {
    if (const char *v = getenv("PLONKY2_HIP_REFERENCE_IN_PLACE"))
        if (v[0] && v[0] != '0') return nullptr;  // the caller would rather not have the staging buffer
    if (st.ref_staging && !st.ref_staging_owned) return st.ref_staging_elems >= elems ? st.ref_staging : nullptr;
    if (st.ref_staging_elems < elems) {
        if (st.ref_staging) (void)hipFree(st.ref_staging);  // synchronises the device: nothing in flight reads it
        st.ref_staging = nullptr;
        st.ref_staging_elems = 0;
        if (hipMalloc(&st.ref_staging, elems * sizeof(uint64_t)) != hipSuccess) {
            (void)hipGetLastError();  // not an error of the call: fall back to reading the rows in place
            st.ref_staging = nullptr;
            return nullptr;
        }
        st.ref_staging_elems = elems;
        st.ref_staging_owned = true;
    }
    return st.ref_staging;
}

uint64_t gl_reference_quotient_staging_bytes(int log_len) {
    if (log_len < 0 || log_len + (int)ED25519_RATE_BITS > 24) return 0;
    const uint64_t n_ext = (1ull << log_len) << ED25519_RATE_BITS;
    return 8ull * (ED25519_NUM_WIRES + ED25519_CONSTANTS_SIGMAS_LEAF_LEN + ED25519_ZS_PARTIAL_PRODUCTS_LEAF_LEN) * n_ext;
}

GlError gl_reference_quotient_set_staging(void *d_staging, uint64_t bytes) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (d_staging && ((uintptr_t)d_staging & 15)) return fail(GL_E_INVALID, "the staging buffer must be 16-byte aligned");
    DeviceState &st = device_state(dev);
    std::lock_guard<std::mutex> lk(st.ref_mu);  // no compute_quotient_polys is running on this device
    if (st.ref_staging && st.ref_staging_owned) HIP_TRY(hipFree(st.ref_staging));
    st.ref_staging = static_cast<uint64_t *>(d_staging);
    st.ref_staging_elems = d_staging ? bytes / 8 : 0;
    st.ref_staging_owned = false;
    return ok();
}

GlError gl_reference_quotient_release(void) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    DeviceState &st = device_state(dev);
    std::lock_guard<std::mutex> lk(st.ref_mu);
    if (st.ref_staging && st.ref_staging_owned) HIP_TRY(hipFree(st.ref_staging));
    st.ref_staging = nullptr;
    st.ref_staging_elems = 0;
    st.ref_staging_owned = false;
    return ok();
}

GlError gl_reference_quotient_prepare(void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null pointer");
    const GateKernel *k;
    return get_ed25519_kernel(&k);
}

GlError gl_reference_set_public_inputs_hash(const uint64_t *h_hash) {
    std::lock_guard<std::mutex> lk(g_ref_mu);
    for (int k = 0; k < 4; k++) g_ref_pih[k] = h_hash ? h_hash[k] : ED25519_REFERENCE_PUBLIC_INPUTS_HASH[k];
    return ok();
}

GlError gl_reference_set_public_inputs_hash_ctx(const uint64_t *h_hash, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    CtxState *c;
    HIP_TRY(ctx_state(ctx, &c));
    c->have_pih = h_hash != nullptr;
    for (int k = 0; k < 4; k++) c->pih[k] = h_hash ? h_hash[k] : 0;
    return ok();
}

// cuda/plonky2_gpu.cu:609-783. The circuit (shape, gate table, selector groups) is compiled in, as in the
// reference; what the reference precomputes on the host and hands over as tables (root_table2, shift_inv_powers,
// points, Z_H on the coset and its inverses) the kernels here derive themselves, so those arguments are not read.
GlError compute_quotient_polys(const uint64_t *d_ext_values_flatten, int poly_num, int values_num_per_poly, int log_len,
                               const uint64_t *d_root_table2, const uint64_t *d_shift_inv_powers, int rate_bits, int salt_size,
                               const GlDataSlice *zs_partial_products_commitment_leaves,
                               const GlDataSlice *constants_sigmas_commitment_leaves, void *d_outs, void *d_quotient_polys,
                               const GlDataSlice *points, const GlDataSlice *z_h_on_coset_evals,
                               const GlDataSlice *z_h_on_coset_inverses, const GlDataSlice *k_is, const GlDataSlice *alphas,
                               const GlDataSlice *betas, const GlDataSlice *gammas, void *ctx) {
    DeviceCall device_call(ctx);
    (void)d_root_table2, (void)d_shift_inv_powers, (void)points, (void)z_h_on_coset_evals, (void)z_h_on_coset_inverses;
    const GlDataSlice *zs = zs_partial_products_commitment_leaves, *cs = constants_sigmas_commitment_leaves;
    if (!ctx || !d_ext_values_flatten || !zs || !cs || !d_outs || !d_quotient_polys || !k_is || !alphas || !betas || !gammas)
        return fail(GL_E_INVALID, "null pointer");
    if (!zs->ptr || !cs->ptr || !k_is->ptr || !alphas->ptr || !betas->ptr || !gammas->ptr) return fail(GL_E_INVALID, "null pointer in DataSlice");
    if (log_len < 0 || log_len + (int)ED25519_RATE_BITS > 24 || values_num_per_poly != (1 << log_len)) return fail(GL_E_INVALID, "bad sizes");
    if (salt_size < 0 || poly_num != (int)ED25519_NUM_WIRES || rate_bits != (int)ED25519_RATE_BITS)
        return fail(GL_E_INVALID, "compute_quotient_polys is compiled for the ed25519 circuit: 234 wire polynomials, rate_bits 3 "
                                  "(plonky2_gpu.cu:666-675); use gl_compute_quotient_polys for any other circuit");
    const uint64_t n_ext = (uint64_t)values_num_per_poly << rate_bits;
    // the reference's own asserts (plonky2_gpu.cu:677-683)
    if ((uint64_t)cs->len != n_ext * ED25519_CONSTANTS_SIGMAS_LEAF_LEN || (uint64_t)zs->len != n_ext * ED25519_ZS_PARTIAL_PRODUCTS_LEAF_LEN)
        return fail(GL_E_INVALID, "leaf buffers must hold n_ext x 88 (constants_sigmas) and n_ext x 20 (zs_partial_products) elements");
    if (alphas->len != (int)ED25519_NUM_CHALLENGES || betas->len != (int)ED25519_NUM_CHALLENGES || gammas->len != (int)ED25519_NUM_CHALLENGES)
        return fail(GL_E_INVALID, "alphas, betas and gammas must hold num_challenges = 2 elements each");
    if (k_is->len < (int)ED25519_NUM_ROUTED_WIRES) return fail(GL_E_INVALID, "k_is must hold num_routed_wires = 80 elements");
    const GateKernel *kernel;
    GlError ge = get_ed25519_kernel(&kernel);
    if (ge.code) return ge;
    // the challenges live in device memory on the reference's side of the boundary (prover.rs:489-516)
    uint64_t ch[3][2];
    const GlDataSlice *src[3] = {alphas, betas, gammas};
    for (int i = 0; i < 3; i++) HIP_TRY(hipMemcpyAsync(ch[i], src[i]->ptr, sizeof(ch[i]), hipMemcpyDeviceToHost, S(ctx)->stream));
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    // The circuit's public-inputs hash has no slot in the reference's signature (its kernel has the proof's value compiled in,
    // plonky2_gpu_impl.cuh:600-685): the context's own (gl_reference_set_public_inputs_hash_ctx) if it has one, else the process's.
    uint64_t pih[4];
    CtxState *cst;
    HIP_TRY(ctx_state(ctx, &cst));
    if (cst->have_pih) {
        for (int k = 0; k < 4; k++) pih[k] = cst->pih[k];
    } else {
        std::lock_guard<std::mutex> lk(g_ref_mu);
        for (int k = 0; k < 4; k++) pih[k] = g_ref_pih[k];
    }
    // one gate-kernel object (its constant tables) and one staging buffer per device: calls of this symbol on one device take
    // turns, held to the stream synchronisation that ends the call
    DeviceState &dst = device_state(cst->dev);
    std::lock_guard<std::mutex> ref_turn(dst.ref_mu);
    GlQuotientArgs a = {};
    a.d_wires_leaves = d_ext_values_flatten;  // leaf-major, leaf t = point bitrev(t) (plonky2_gpu_impl.cuh:537-541)
    a.d_constants_sigmas_leaves = static_cast<const uint64_t *>(cs->ptr);
    a.d_zs_partial_products_leaves = static_cast<const uint64_t *>(zs->ptr);
    a.wires_leaf_len = (uint32_t)(poly_num + salt_size);
    a.constants_sigmas_leaf_len = ED25519_CONSTANTS_SIGMAS_LEAF_LEN;
    a.zs_partial_products_leaf_len = ED25519_ZS_PARTIAL_PRODUCTS_LEAF_LEN;
    a.d_k_is = static_cast<const uint64_t *>(k_is->ptr);
    a.h_alphas = ch[0], a.h_betas = ch[1], a.h_gammas = ch[2];
    a.num_constants = ED25519_NUM_CONSTANTS;
    a.num_routed_wires = ED25519_NUM_ROUTED_WIRES;
    a.num_challenges = ED25519_NUM_CHALLENGES;
    a.num_gate_constraints = ED25519_NUM_GATE_CONSTRAINTS;
    a.degree_bits = (uint32_t)log_len;
    a.rate_bits = (uint32_t)rate_bits;
    a.quotient_degree_factor = ED25519_QUOTIENT_DEGREE_FACTOR;
    a.coset_shift = 7;
    a.column_stride = 0;
    if (uint64_t *stage = get_ref_staging(dst, (uint64_t)(a.wires_leaf_len + a.constants_sigmas_leaf_len + a.zs_partial_products_leaf_len) * n_ext)) {
        uint64_t *w = stage, *c = w + (uint64_t)a.wires_leaf_len * n_ext, *z = c + (uint64_t)a.constants_sigmas_leaf_len * n_ext;
        HIP_TRY(transpose_to_column_major(a.d_wires_leaves, w, a.wires_leaf_len, n_ext, n_ext, S(ctx)->stream));
        HIP_TRY(transpose_to_column_major(a.d_constants_sigmas_leaves, c, a.constants_sigmas_leaf_len, n_ext, n_ext, S(ctx)->stream));
        HIP_TRY(transpose_to_column_major(a.d_zs_partial_products_leaves, z, a.zs_partial_products_leaf_len, n_ext, n_ext, S(ctx)->stream));
        a.d_wires_leaves = w, a.d_constants_sigmas_leaves = c, a.d_zs_partial_products_leaves = z;
        a.column_stride = n_ext;
    }
    a.gate_kernel = kernel;
    a.h_public_inputs_hash = pih;
    a.d_gate_workspace = static_cast<uint64_t *>(d_outs);  // [2][n_ext]: the reference's scratch for the same stage
    GlError e = gl_compute_quotient_polys(&a, static_cast<uint64_t *>(d_quotient_polys), ctx);
    if (e.code) return e;
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    return ok();
}

const char *cudaGetErrorString(int code) {
    if (code < 0) return code == GL_E_INVALID ? "plonky2_hip: invalid argument" : "plonky2_hip: unsupported";
    return hipGetErrorString((hipError_t)code);
}

}  // extern "C"
