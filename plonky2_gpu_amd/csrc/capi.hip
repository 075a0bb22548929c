// capi.hip — the extern "C" boundary of libplonky2_hip.so (declared in include/plonky2_hip.h): the thin gl_* wrappers. The state behind a
// ctx is in ctx.hip, the commit in commit.hip, the reference's own symbols in reference_abi.hip, the tests' probes in probes.hip.
#include <string>

#include <stdlib.h>

#include "commit.h"
#include "gl_field.h"
#include "keccak.h"
#include "merkle.h"
#include "plonk.h"
#include "lookup.h"
#include "fri.h"

using namespace plonky2_hip;

namespace {

// out[(q * n_cols + c) * L + i] = lde[c * col_stride + q * L + i]: every column's leaf range of every rank, grouped by
// rank — what a column-sharded commit sends (dist.py); 16 B per lane, L is a multiple of 2.
__global__ __launch_bounds__(256) void pack_leaf_ranges_kernel(const uint64_t *__restrict__ lde, uint64_t col_stride, uint32_t n_cols,
                                                               uint64_t L, uint32_t world, uint64_t *__restrict__ out) {
    const uint64_t pairs = L / 2, total = (uint64_t)world * n_cols * pairs;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = (g % pairs) * 2, rest = g / pairs;
        const uint32_t c = (uint32_t)(rest % n_cols), q = (uint32_t)(rest / n_cols);
        const uint4 v = *reinterpret_cast<const uint4 *>(lde + (uint64_t)c * col_stride + (uint64_t)q * L + i);
        *reinterpret_cast<uint4 *>(out + ((uint64_t)q * n_cols + c) * L + i) = v;
    }
}

}  // namespace

extern "C" {

const char *gl_version(void) { return "plonky2_hip 0.6.0 gfx950"; }

int gl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void *gl_ctx_create(int device) {
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    Streams *s = (Streams *)calloc(1, sizeof(Streams));
    if (!s) return nullptr;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking) != hipSuccess) {
        free(s);
        return nullptr;
    }
    CtxState *c;
    if (ctx_state(s, &c) != hipSuccess) {  // the device's tables and this context's workspace, now rather than inside the first call
        (void)hipGetLastError();
        (void)hipStreamDestroy(s->stream);
        (void)hipStreamDestroy(s->stream2);
        free(s);
        return nullptr;
    }
    return s;
}

void gl_ctx_release(void *ctx) {
    if (!ctx) return;
    int dev = 0;
    if (!ctx_device(ctx, &dev)) (void)hipGetLastError();
    (void)hipStreamSynchronize(S(ctx)->stream);
    (void)hipStreamSynchronize(S(ctx)->stream2);
    ctx_state_release(ctx);
}

void gl_ctx_destroy(void *ctx) {
    if (!ctx) return;
    gl_ctx_release(ctx);
    (void)hipStreamDestroy(S(ctx)->stream);
    (void)hipStreamDestroy(S(ctx)->stream2);
    free(ctx);
}

uint64_t gl_workspace_bytes(void) { return NTT_SCRATCH_ELEMS * sizeof(uint64_t); }

GlError gl_ctx_set_workspace(void *ctx, void *d_workspace, uint64_t bytes) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    if (d_workspace && (bytes < gl_workspace_bytes() || ((uintptr_t)d_workspace & 15)))
        return fail(GL_E_INVALID, "a caller-provided workspace holds at least gl_workspace_bytes() bytes, 16-byte aligned");
    CtxState *c;
    HIP_TRY(ctx_state(ctx, &c));
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));  // nothing of this context may still use the old one
    if (c->hash_stream) HIP_TRY(hipStreamSynchronize(c->hash_stream));
    if (c->scratch_owned && c->tb.scratch) HIP_TRY(hipFree(c->tb.scratch));
    c->tb.scratch = nullptr;
    c->scratch_owned = false;
    if (d_workspace) {
        c->tb.scratch = static_cast<uint64_t *>(d_workspace);
        c->tb.scratch_elems = bytes / 8;
    } else {
        HIP_TRY(hipMalloc(&c->tb.scratch, NTT_SCRATCH_ELEMS * sizeof(uint64_t)));
        c->tb.scratch_elems = NTT_SCRATCH_ELEMS;
        c->scratch_owned = true;
    }
    return ok();
}

GlError gl_ctx_synchronize(void *ctx) {
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream2));
    return ok();
}

GlError gl_malloc(void **d_ptr, uint64_t bytes) {
    if (!d_ptr) return fail(GL_E_INVALID, "null pointer");
    HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 8));
    return ok();
}

GlError gl_ctx_malloc(void **d_ptr, uint64_t bytes, void *ctx) {
    if (!d_ptr || !ctx) return fail(GL_E_INVALID, "null pointer");
    int dev = 0;
    if (!ctx_device(ctx, &dev)) return fail(GL_E_INVALID, "the context's stream has no device");
    HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 8));
    return ok();
}

GlError gl_free(void *d_ptr) {
    HIP_TRY(hipFree(d_ptr));
    return ok();
}

GlError gl_malloc_host(void **h_ptr, uint64_t bytes) {
    if (!h_ptr) return fail(GL_E_INVALID, "null pointer");
    HIP_TRY(hipHostMalloc(h_ptr, bytes ? bytes : 8, hipHostMallocDefault));
    return ok();
}

GlError gl_free_host(void *h_ptr) {
    HIP_TRY(hipHostFree(h_ptr));
    return ok();
}

GlError gl_memcpy_h2d(void *d_dst, const void *h_src, uint64_t bytes, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, S(ctx)->stream));
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    return ok();
}

GlError gl_memcpy_h2d_async(void *d_dst, const void *h_src, uint64_t bytes, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, S(ctx)->stream2));
    return ok();
}

GlError gl_memcpy_d2h(void *h_dst, const void *d_src, uint64_t bytes, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, S(ctx)->stream));
    HIP_TRY(hipStreamSynchronize(S(ctx)->stream));
    return ok();
}

GlError gl_memcpy_d2d(void *d_dst, const void *d_src, uint64_t bytes, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    HIP_TRY(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, S(ctx)->stream));
    return ok();
}

GlError gl_memset_zero(void *d_dst, uint64_t bytes, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx) return fail(GL_E_INVALID, "null ctx");
    HIP_TRY(hipMemsetAsync(d_dst, 0, bytes, S(ctx)->stream));
    return ok();
}

GlError gl_event_create(void **event) {
    if (!event) return fail(GL_E_INVALID, "null pointer");
    hipEvent_t ev;
    HIP_TRY(hipEventCreate(&ev));
    *event = ev;
    return ok();
}

GlError gl_event_record(void *event, void *ctx) {
    if (!event || !ctx) return fail(GL_E_INVALID, "null pointer");
    HIP_TRY(hipEventRecord((hipEvent_t)event, S(ctx)->stream));
    return ok();
}

GlError gl_event_elapsed_ms(float *ms, void *start_event, void *stop_event) {
    if (!ms || !start_event || !stop_event) return fail(GL_E_INVALID, "null pointer");
    HIP_TRY(hipEventSynchronize((hipEvent_t)stop_event));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start_event, (hipEvent_t)stop_event));
    return ok();
}

void gl_event_destroy(void *event) {
    if (event) (void)hipEventDestroy((hipEvent_t)event);
}

// the argument rules of gl_ntt_batch (include/plonky2_hip.h), also checked by gl_coset_ntt_batch BEFORE it scales the values: a refused
// call leaves the caller's buffer as it was
static const char *ntt_batch_argument_error(const uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint64_t stride, int inverse,
                                            int bit_reversed) {
    if (log_n > 24) return "log_n > 24 is not supported by this build";
    if (stride < (1ull << log_n)) return "stride smaller than the polynomial";
    if (inverse && bit_reversed) return "bit-reversed inverse is not on the hot path";
    if (inverse && (stride & ((1ull << log_n) - 1))) return "inverse needs stride % n == 0";
    if ((stride & 1) && log_n > 0 && poly_num > 1) return "stride must be even (16-byte accesses)";
    if ((uintptr_t)d_values & 15) return "d_values must be 16-byte aligned";
    return nullptr;
}

GlError gl_ntt_batch(uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint64_t stride, int inverse,
                     int bit_reversed, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || (!d_values && poly_num)) return fail(GL_E_INVALID, "null pointer");
    if (const char *why = ntt_batch_argument_error(d_values, poly_num, log_n, stride, inverse, bit_reversed)) return fail(GL_E_INVALID, why);
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    hipError_t e = ntt_batch(*tb, d_values, d_values, poly_num, log_n, stride, stride,
                             bit_reversed ? NttOrder::BitReversed : NttOrder::Natural, inverse != 0, S(ctx)->stream);
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "gl_ntt_batch: size, order, stride or batch outside what the pass plans take");
    HIP_TRY(e);
    return ok();
}

GlError gl_coset_lde_batch(const uint64_t *d_coeffs, uint64_t *d_out, uint64_t poly_num, uint32_t log_n,
                           uint32_t rate_bits, uint64_t shift, uint64_t src_stride, uint64_t dst_stride, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || ((!d_coeffs || !d_out) && poly_num)) return fail(GL_E_INVALID, "null pointer");
    if (log_n > 24 || rate_bits > 8) return fail(GL_E_INVALID, "log_n > 24 or rate_bits > 8 not supported");
    const uint64_t n = 1ull << log_n;
    if (src_stride < n || dst_stride < (n << rate_bits)) return fail(GL_E_INVALID, "stride too small");
    if (((uintptr_t)d_coeffs | (uintptr_t)d_out) & 15) return fail(GL_E_INVALID, "buffers must be 16-byte aligned");
    if (log_n > 0 && ((src_stride | dst_stride) & 1)) return fail(GL_E_INVALID, "strides must be even");
    const NttTables *tb;
    CosetLease ct;
    HIP_TRY(get_tables(ctx, &tb));
    HIP_TRY(get_coset_tables(log_n, rate_bits, shift, S(ctx)->stream, &ct));
    hipError_t e = coset_lde_batch(*tb, *ct, d_coeffs, d_out, poly_num, src_stride, dst_stride, S(ctx)->stream);
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "gl_coset_lde_batch: size, strides or batch outside what the pass plans take");
    HIP_TRY(e);
    return ok();
}

GlError gl_coset_ntt_batch(uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint64_t stride, uint64_t shift, int inverse,
                           void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || (!d_values && poly_num)) return fail(GL_E_INVALID, "null pointer");
    if (shift % glh::P == 0) return fail(GL_E_INVALID, "shift must be non-zero");
    if (const char *why = ntt_batch_argument_error(d_values, poly_num, log_n, stride, inverse, 0)) return fail(GL_E_INVALID, why);
    CosetLease ct;
    if (!inverse) {
        // coset_fft: c_i *= shift^i, then fft (polynomial/mod.rs:286-299)
        HIP_TRY(get_coset_tables(log_n, 0, shift % glh::P, S(ctx)->stream, &ct));
        HIP_TRY(scale_by_powers(*ct, d_values, poly_num, stride, S(ctx)->stream));
        return gl_ntt_batch(d_values, poly_num, log_n, stride, 0, 0, ctx);
    }
    // coset_ifft: ifft, then c_i *= shift^-i (polynomial/mod.rs:64-77)
    GlError e = gl_ntt_batch(d_values, poly_num, log_n, stride, 1, 0, ctx);
    if (e.code) return e;
    HIP_TRY(get_coset_tables(log_n, 0, glh::inv(shift), S(ctx)->stream, &ct));
    HIP_TRY(scale_by_powers(*ct, d_values, poly_num, stride, S(ctx)->stream));
    return ok();
}

GlError gl_permutation_partial_products(const uint64_t *d_wires, uint64_t wires_stride, const uint64_t *d_sigmas,
                                        uint64_t sigmas_stride, const uint64_t *d_k_is, const uint64_t *h_betas,
                                        const uint64_t *h_gammas, uint32_t num_challenges, uint32_t num_routed,
                                        uint32_t quotient_degree_factor, uint32_t log_n, uint64_t *d_out, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_wires || !d_sigmas || !d_k_is || !h_betas || !h_gammas || !d_out) return fail(GL_E_INVALID, "null pointer");
    if (num_challenges == 0 || num_challenges > 4) return fail(GL_E_INVALID, "num_challenges must be 1..4");
    if (quotient_degree_factor < 2 || num_routed == 0) return fail(GL_E_INVALID, "bad num_routed / quotient_degree_factor");
    if (quotient_degree_factor >= num_routed)
        return fail(GL_E_INVALID, "quotient_degree_factor must be smaller than num_routed_wires (prover.rs:102-105)");
    if (log_n > 24) return fail(GL_E_INVALID, "log_n > 24");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    HIP_TRY(permutation_partial_products(*tb, d_wires, wires_stride, d_sigmas, sigmas_stride, d_k_is, h_betas, h_gammas,
                                         num_challenges, num_routed, quotient_degree_factor, log_n, d_out, S(ctx)->stream));
    return ok();
}

GlError gl_gate_kernel_build(const GlGateInstr *h_instrs, uint32_t num_instrs, const GlGateDesc *h_gates, uint32_t num_gates,
                             const uint64_t *h_immediates, uint32_t num_immediates, uint32_t num_selectors,
                             uint32_t num_gate_constraints, uint32_t num_challenges, void **kernel) {
    if (!h_instrs || !h_gates || !kernel || (num_immediates && !h_immediates)) return fail(GL_E_INVALID, "null pointer");
    if (num_gate_constraints > 256) return fail(GL_E_INVALID, "num_gate_constraints > 256");
    std::string err;
    GateKernel *k = gate_kernel_build(reinterpret_cast<const uint16_t *>(h_instrs), num_instrs, reinterpret_cast<const uint32_t *>(h_gates),
                                      num_gates, h_immediates, num_immediates, num_selectors, num_gate_constraints, num_challenges, &err);
    if (!k) return fail(GL_E_INVALID, err.c_str());
    *kernel = k;
    return ok();
}

void gl_gate_kernel_destroy(void *kernel) { gate_kernel_destroy(static_cast<GateKernel *>(kernel)); }

const char *gl_gate_kernel_source(const void *kernel) { return kernel ? gate_kernel_source(static_cast<const GateKernel *>(kernel)) : ""; }

GlError gl_compute_quotient_polys(const GlQuotientArgs *args, uint64_t *d_quotient_polys, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !args || !d_quotient_polys) return fail(GL_E_INVALID, "null pointer");
    if (!args->d_wires_leaves || !args->d_constants_sigmas_leaves || !args->d_zs_partial_products_leaves || !args->d_k_is ||
        !args->h_betas || !args->h_gammas || !args->h_alphas)
        return fail(GL_E_INVALID, "null pointer in GlQuotientArgs");
    QuotientArgs a = {};
    a.wires_leaves = args->d_wires_leaves;
    a.cs_leaves = args->d_constants_sigmas_leaves;
    a.zpp_leaves = args->d_zs_partial_products_leaves;
    a.wires_len = args->wires_leaf_len;
    a.cs_len = args->constants_sigmas_leaf_len;
    a.zpp_len = args->zs_partial_products_leaf_len;
    a.k_is = args->d_k_is;
    a.gate_terms = args->d_gate_constraint_terms;
    a.betas = args->h_betas;
    a.gammas = args->h_gammas;
    a.alphas = args->h_alphas;
    a.num_constants = args->num_constants;
    a.num_routed = args->num_routed_wires;
    a.num_challenges = args->num_challenges;
    a.num_gate_constraints = args->num_gate_constraints;
    a.degree_bits = args->degree_bits;
    a.rate_bits = args->rate_bits;
    a.quotient_degree_factor = args->quotient_degree_factor;
    a.shift = args->coset_shift;
    a.column_stride = args->column_stride;
    if (args->gate_kernel) {
        if (args->gate_program || args->d_gate_constraint_terms)
            return fail(GL_E_INVALID, "give one source of gate constraints: terms, a gate program or a gate kernel");
        if (!args->h_public_inputs_hash || !args->d_gate_workspace) return fail(GL_E_INVALID, "gate_kernel needs h_public_inputs_hash and d_gate_workspace");
        a.gate_kernel = static_cast<const GateKernel *>(args->gate_kernel);
        if (gate_kernel_num_constraints(a.gate_kernel) != args->num_gate_constraints || gate_kernel_num_challenges(a.gate_kernel) != args->num_challenges)
            return fail(GL_E_INVALID, "gate kernel was built for other num_gate_constraints / num_challenges");
        a.public_inputs_hash = args->h_public_inputs_hash;
        a.gate_partial_workspace = args->d_gate_workspace;
    }
    GateProgramArgs gpa = {};
    if (args->gate_program) {
        const GlGateProgram *g = args->gate_program;
        if (!g->d_instrs || !g->d_gates) return fail(GL_E_INVALID, "null pointer in GlGateProgram");
        if (args->d_gate_constraint_terms) return fail(GL_E_INVALID, "give either gate terms or a gate program, not both");
        if (args->num_gate_constraints > 256) return fail(GL_E_INVALID, "num_gate_constraints > 256");
        gpa.instrs = reinterpret_cast<const uint16_t *>(g->d_instrs);
        gpa.gates = reinterpret_cast<const uint32_t *>(g->d_gates);
        gpa.imms = g->d_immediates;
        gpa.num_gates = g->num_gates;
        gpa.num_selectors = g->num_selectors;
        for (int k = 0; k < 4; k++) gpa.public_inputs_hash[k] = g->public_inputs_hash[k];
        a.gate_program = &gpa;
    }
    const uint32_t qdb = glh::log2_ceil(a.quotient_degree_factor);
    if (a.quotient_degree_factor < 2 || qdb > a.rate_bits)
        return fail(GL_E_INVALID, "constraints of degree higher than the rate are not supported (prover.rs:807-811)");
    if (a.column_stride && a.degree_bits + qdb <= 24 && a.column_stride < (1ull << (a.degree_bits + qdb)))
        return fail(GL_E_INVALID, "column_stride smaller than the column length n << log2_ceil(quotient_degree_factor)");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    hipError_t e = quotient_values(*tb, a, d_quotient_polys, S(ctx)->stream);
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "inconsistent GlQuotientArgs (leaf lengths / counts / sizes)");
    HIP_TRY(e);
    // values on the coset -> coefficients: coset_ifft per challenge (prover.rs:1009-1021)
    const uint32_t log_lde = a.degree_bits + qdb;
    return gl_coset_ntt_batch(d_quotient_polys, a.num_challenges, log_lde, 1ull << log_lde, a.shift, 1, ctx);
}

GlError gl_eval_polys_ext2(const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint64_t stride, const uint64_t *h_points,
                           uint32_t num_points, uint64_t *d_out, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !h_points || !d_out || (!d_coeffs && poly_num)) return fail(GL_E_INVALID, "null pointer");
    if (num_points == 0 || num_points > 4) return fail(GL_E_INVALID, "num_points must be 1..4");
    if (poly_num > 65535) return fail(GL_E_INVALID, "poly_num > 65535");
    if (stride < (1ull << log_n)) return fail(GL_E_INVALID, "stride smaller than the polynomial");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    hipError_t e = eval_polys_ext2(*tb, d_coeffs, poly_num, log_n, stride, h_points, num_points, d_out, S(ctx)->stream);
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "unsupported size for gl_eval_polys_ext2");
    HIP_TRY(e);
    return ok();
}

GlError gl_fri_reduce_polys_base(const uint64_t *const *d_poly_ptrs, uint32_t num_polys, uint64_t n, const uint64_t *h_alpha,
                                 uint64_t *d_out, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_poly_ptrs || !h_alpha || !d_out) return fail(GL_E_INVALID, "null pointer");
    if (num_polys == 0 || num_polys > (1u << 20) || n == 0) return fail(GL_E_INVALID, "bad sizes");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    HIP_TRY(fri_reduce_polys_base(*tb, d_poly_ptrs, num_polys, n, h_alpha, d_out, S(ctx)->stream));
    return ok();
}

GlError gl_fri_divide_by_linear(uint64_t *d_composition, uint64_t n, const uint64_t *h_point, const uint64_t *h_scale, int accumulate,
                                uint64_t *d_final, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_composition || !h_point || !h_scale || !d_final) return fail(GL_E_INVALID, "null pointer");
    if (n < 2 || n > (1ull << 30)) return fail(GL_E_INVALID, "bad length");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    hipError_t e = fri_divide_by_linear_accumulate(*tb, d_composition, n, h_point, h_scale, accumulate, d_final, S(ctx)->stream);
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "point has no inverse / workspace too small");
    HIP_TRY(e);
    return ok();
}

GlError gl_fri_fold(const uint64_t *d_coeffs, uint64_t len, uint32_t arity_bits, const uint64_t *h_beta, uint64_t *d_out, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_coeffs || !h_beta || !d_out) return fail(GL_E_INVALID, "null pointer");
    hipError_t e = fri_fold(d_coeffs, len, arity_bits, h_beta, d_out, S(ctx)->stream);
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "bad arity / length");
    HIP_TRY(e);
    return ok();
}

GlError gl_ext2_interleave(const uint64_t *d_planes, uint64_t len, uint64_t *d_rows, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_planes || !d_rows) return fail(GL_E_INVALID, "null pointer");
    HIP_TRY(fri_interleave(d_planes, len, d_rows, S(ctx)->stream));
    return ok();
}

GlError gl_fri_proof_of_work(const uint64_t *h_state, uint32_t witness_pos, uint32_t min_leading_zeros, uint64_t *h_witness, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !h_state || !h_witness) return fail(GL_E_INVALID, "null pointer");
    if (witness_pos >= 8 || min_leading_zeros > 40) return fail(GL_E_INVALID, "bad witness position / difficulty");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    HIP_TRY(fri_proof_of_work(*tb, h_state, witness_pos, min_leading_zeros, h_witness, S(ctx)->stream));
    return ok();
}

GlError gl_poseidon_permute_batch(uint64_t *d_states, uint64_t count, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || (!d_states && count)) return fail(GL_E_INVALID, "null pointer");
    HIP_TRY(poseidon_permute_batch(d_states, count, S(ctx)->stream));
    return ok();
}

GlError gl_sponge_absorb(uint64_t *h_state, const uint64_t *h_inputs, uint32_t n_blocks, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !h_state || (!h_inputs && n_blocks)) return fail(GL_E_INVALID, "null pointer");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    if (12 + 8ull * n_blocks > tb->scratch_elems) return fail(GL_E_INVALID, "too many blocks");
    hipStream_t st = S(ctx)->stream;
    uint64_t *d_state = tb->scratch, *d_in = tb->scratch + 12;
    HIP_TRY(hipMemcpyAsync(d_state, h_state, 96, hipMemcpyHostToDevice, st));
    if (n_blocks) HIP_TRY(hipMemcpyAsync(d_in, h_inputs, 64ull * n_blocks, hipMemcpyHostToDevice, st));
    HIP_TRY(sponge_absorb(d_state, d_in, n_blocks, st));
    HIP_TRY(hipMemcpyAsync(h_state, d_state, 96, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ok();
}

GlError gl_challenger_step(uint64_t *d_challenger, const GlObserveSrc *h_srcs, uint32_t n_srcs, uint32_t n_challenges, uint64_t *d_out,
                           uint32_t flags, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_challenger || (n_srcs && !h_srcs)) return fail(GL_E_INVALID, "null pointer");
    if (n_srcs > 8) return fail(GL_E_INVALID, "at most eight sources per step");
    if (flags & ~(uint32_t)(GL_CHALLENGER_RESET | GL_CHALLENGER_HASH | GL_CHALLENGER_COMPACT)) return fail(GL_E_INVALID, "unknown flag");
    if (((flags & GL_CHALLENGER_HASH) || n_challenges) && !d_out) return fail(GL_E_INVALID, "null output");
    // the kernel writes the outputs and then the transcript's words: an output inside the transcript would be overwritten, or corrupt it
    const uint64_t out_words = (flags & GL_CHALLENGER_HASH) ? 4 : (n_challenges ? n_challenges : 1);
    if (d_out && d_out + out_words > d_challenger && d_out < d_challenger + 32)
        return fail(GL_E_INVALID, "d_out overlaps the 32 words of d_challenger");
    const uint64_t *ptrs[8];
    uint64_t counts[8], planar[8];
    for (uint32_t i = 0; i < n_srcs; i++) {
        if (h_srcs[i].count && !h_srcs[i].d_ptr) return fail(GL_E_INVALID, "null source");
        if (h_srcs[i].planar_len == GL_OBSERVE_KECCAK_DIGESTS) {
            if (h_srcs[i].count & 3) return fail(GL_E_INVALID, "a Keccak digest source is observed four elements per digest: count must be a multiple of 4");
        } else if (h_srcs[i].planar_len && h_srcs[i].count > 2 * h_srcs[i].planar_len)
            return fail(GL_E_INVALID, "a planar source holds 2 * planar_len elements");
        ptrs[i] = h_srcs[i].d_ptr, counts[i] = h_srcs[i].count, planar[i] = h_srcs[i].planar_len;
    }
    HIP_TRY(challenger_step(d_challenger, ptrs, counts, planar, n_srcs, n_challenges, flags, d_out, S(ctx)->stream));
    return ok();
}

GlError gl_fri_fold_device(const uint64_t *d_coeffs, uint64_t len, uint32_t arity_bits, const uint64_t *d_beta, uint64_t *d_out, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_coeffs || !d_beta || !d_out) return fail(GL_E_INVALID, "null pointer");
    const uint64_t zero[2] = {0, 0};
    hipError_t e = fri_fold(d_coeffs, len, arity_bits, zero, d_out, S(ctx)->stream, d_beta);
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "bad arity / length");
    HIP_TRY(e);
    return ok();
}

GlError gl_fri_proof_of_work_device(const uint64_t *d_challenger, uint32_t min_leading_zeros, uint64_t *d_witness, uint64_t *h_witness, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_challenger || !d_witness || !h_witness) return fail(GL_E_INVALID, "null pointer");
    if (min_leading_zeros > 40) return fail(GL_E_INVALID, "bad difficulty");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    const uint64_t unused[12] = {0};
    HIP_TRY(fri_proof_of_work(*tb, unused, 0, min_leading_zeros, h_witness, S(ctx)->stream, d_challenger, d_witness));
    return ok();
}

GlError gl_merkle_open_batch_device(const uint64_t *d_leaves, uint64_t row_stride, uint64_t elem_stride, uint32_t leaf_len, uint64_t n_leaves,
                                    uint32_t cap_height, const uint64_t *d_digests, const uint64_t *d_indices, uint32_t count,
                                    uint32_t index_shift, uint64_t *d_out_leaves, uint64_t *d_out_siblings, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_leaves || !d_indices || !d_out_leaves || (!d_out_siblings && (n_leaves >> cap_height) > 1)) return fail(GL_E_INVALID, "null pointer");
    if (n_leaves == 0 || (n_leaves & (n_leaves - 1)) || cap_height > 63 || (1ull << cap_height) > n_leaves || index_shift > 32 ||
        (n_leaves << index_shift) >> index_shift != n_leaves)
        return fail(GL_E_INVALID, "bad tree shape");
    if (count == 0) return ok();
    if ((n_leaves >> cap_height) > 1 && !d_digests) return fail(GL_E_INVALID, "null pointer");
    HIP_TRY(merkle_open_batch(d_leaves, row_stride, elem_stride, leaf_len, n_leaves, cap_height, d_digests, d_indices, count, d_out_leaves,
                              d_out_siblings, S(ctx)->stream, (n_leaves << index_shift) - 1, index_shift));
    return ok();
}

GlError gl_merkle_open_batch(const uint64_t *d_leaves, uint64_t row_stride, uint64_t elem_stride, uint32_t leaf_len, uint64_t n_leaves,
                             uint32_t cap_height, const uint64_t *d_digests, const uint64_t *h_indices, uint32_t count,
                             uint64_t *h_out_leaves, uint64_t *h_out_siblings, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_leaves || !h_indices || !h_out_leaves || (!h_out_siblings && (n_leaves >> cap_height) > 1))
        return fail(GL_E_INVALID, "null pointer");
    if (n_leaves == 0 || (n_leaves & (n_leaves - 1)) || cap_height > 63 || (1ull << cap_height) > n_leaves)
        return fail(GL_E_INVALID, "bad tree shape");
    if (count == 0) return ok();
    for (uint32_t q = 0; q < count; q++)
        if (h_indices[q] >= n_leaves) return fail(GL_E_INVALID, "leaf index out of range");
    const uint64_t layers = glh::log2_ceil(n_leaves) - cap_height, need = (uint64_t)count * (1 + leaf_len + 4 * layers);
    if (layers && !d_digests) return fail(GL_E_INVALID, "null pointer");
    const NttTables *tb;
    HIP_TRY(get_tables(ctx, &tb));
    if (need > tb->scratch_elems) return fail(GL_E_INVALID, "too many openings for the workspace");
    hipStream_t st = S(ctx)->stream;
    uint64_t *d_idx = tb->scratch, *d_ol = d_idx + count, *d_os = d_ol + (uint64_t)count * leaf_len;
    HIP_TRY(hipMemcpyAsync(d_idx, h_indices, 8ull * count, hipMemcpyHostToDevice, st));
    HIP_TRY(merkle_open_batch(d_leaves, row_stride, elem_stride, leaf_len, n_leaves, cap_height, d_digests, d_idx, count, d_ol, d_os, st));
    HIP_TRY(hipMemcpyAsync(h_out_leaves, d_ol, 8ull * count * leaf_len, hipMemcpyDeviceToHost, st));
    if (layers) HIP_TRY(hipMemcpyAsync(h_out_siblings, d_os, 32ull * count * layers, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ok();
}

// the argument rules of gl_merkle_tree_from_{columns,leaves}[_h], checked before anything is launched. col_stride: of the columns; a
// tree from rows passes n_leaves. The hashers differ in three rules: Keccak hashes an empty leaf without reading it, so it takes
// a null input when leaf_len == 0; it checks d_digests for every tree with a layer below the cap, which the Poseidon entry
// points leave to the caller; and it has no leaf of four elements.
static const char *tree_argument_error(uint32_t hasher, const uint64_t *d_in, uint32_t leaf_len, uint64_t n_leaves, uint64_t col_stride,
                                       uint32_t cap_height, const uint64_t *d_digests, const uint64_t *d_cap, const void *ctx) {
    if (hasher != GL_HASHER_POSEIDON && hasher != GL_HASHER_KECCAK25) return "unknown hasher";
    const bool keccak = hasher == GL_HASHER_KECCAK25;
    if (!ctx || !d_cap || (!d_in && !(keccak && leaf_len == 0))) return "null pointer";
    if (n_leaves == 0 || (n_leaves & (n_leaves - 1))) return "n_leaves must be a power of two";
    if (cap_height > 63 || (1ull << cap_height) > n_leaves) return "cap_height should be at most log2(leaves.len())";
    if (keccak && (1ull << cap_height) < n_leaves && !d_digests) return "null pointer";
    if (leaf_len > 1 && col_stride < n_leaves) return "col_stride smaller than n_leaves: the columns would overlap";
    if (keccak && leaf_len == 4) return KECCAK_LEAF_LEN_4;
    return nullptr;
}

GlError gl_merkle_tree_from_columns(const uint64_t *d_cols, uint32_t leaf_len, uint64_t n_leaves, uint64_t col_stride,
                                    uint32_t cap_height, uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    return gl_merkle_tree_from_columns_h(GL_HASHER_POSEIDON, d_cols, leaf_len, n_leaves, col_stride, cap_height, d_digests, d_cap, ctx);
}

GlError gl_merkle_tree_from_leaves(const uint64_t *d_rows, uint32_t leaf_len, uint64_t n_leaves, uint32_t cap_height,
                                   uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    return gl_merkle_tree_from_leaves_h(GL_HASHER_POSEIDON, d_rows, leaf_len, n_leaves, cap_height, d_digests, d_cap, ctx);
}

GlError gl_transpose(const uint64_t *d_cols, uint64_t *d_rows, uint32_t n_cols, uint64_t n_rows, uint64_t col_stride,
                     void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_cols || !d_rows) return fail(GL_E_INVALID, "null pointer");
    if (n_cols > 1 && col_stride < n_rows) return fail(GL_E_INVALID, "col_stride smaller than n_rows: the columns would overlap");
    HIP_TRY(transpose_to_leaf_major(d_cols, d_rows, n_cols, n_rows, col_stride, S(ctx)->stream));
    return ok();
}

GlError gl_pack_leaf_ranges(const uint64_t *d_lde, uint64_t col_stride, uint32_t n_cols, uint64_t leaves_per_rank, uint32_t world,
                            uint64_t *d_out, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_lde || !d_out) return fail(GL_E_INVALID, "null pointer");
    if (world == 0 || n_cols == 0 || leaves_per_rank == 0) return ok();
    if ((leaves_per_rank & 1) || (col_stride & 1) || (((uintptr_t)d_lde | (uintptr_t)d_out) & 15))
        return fail(GL_E_INVALID, "leaf ranges and strides must be even, buffers 16-byte aligned");
    if (col_stride < (uint64_t)world * leaves_per_rank) return fail(GL_E_INVALID, "col_stride smaller than world * leaves_per_rank");
    const uint64_t total = (uint64_t)world * n_cols * (leaves_per_rank / 2);
    const unsigned grid = (unsigned)(total / 256 + 1 > 16384 ? 16384 : total / 256 + 1);
    hipLaunchKernelGGL(pack_leaf_ranges_kernel, dim3(grid), dim3(256), 0, S(ctx)->stream, d_lde, col_stride, n_cols, leaves_per_rank, world, d_out);
    HIP_TRY(hipGetLastError());
    return ok();
}

GlError gl_commit_from_coeffs(const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                              uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde,
                              uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    return gl_commit_from_coeffs_h(GL_HASHER_POSEIDON, d_coeffs, poly_num, log_n, rate_bits, cap_height, salt_size, shift, d_lde, d_leaves, d_digests, d_cap, ctx);
}

GlError gl_commit_from_values(uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                              uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde,
                              uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    return gl_commit_from_values_h(GL_HASHER_POSEIDON, d_values, poly_num, log_n, rate_bits, cap_height, salt_size, shift, d_lde, d_leaves, d_digests, d_cap, ctx);
}

GlError gl_keccak_hash_no_pad_batch(const uint64_t *d_inputs, uint32_t len, uint64_t stride, uint64_t count, uint64_t *d_out, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_out || (!d_inputs && len)) return fail(GL_E_INVALID, "null pointer");
    if (count > 1 && stride < len) return fail(GL_E_INVALID, "stride smaller than len: the inputs would overlap");
    if ((uintptr_t)d_out & 15) return fail(GL_E_INVALID, "d_out must be 16-byte aligned");
    if (count > (1ull << 40)) return fail(GL_E_INVALID, "count too large");
    HIP_TRY(keccak_hash_no_pad_batch(d_inputs, len, stride, count, d_out, S(ctx)->stream));
    return ok();
}

GlError gl_merkle_tree_from_columns_h(uint32_t hasher, const uint64_t *d_cols, uint32_t leaf_len, uint64_t n_leaves, uint64_t col_stride,
                                      uint32_t cap_height, uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    DeviceCall device_call(ctx);
    if (const char *why = tree_argument_error(hasher, d_cols, leaf_len, n_leaves, col_stride, cap_height, d_digests, d_cap, ctx))
        return fail(GL_E_INVALID, why);
    if (hasher == GL_HASHER_KECCAK25)
        HIP_TRY(keccak_merkle_tree(d_cols, 1, col_stride, leaf_len, n_leaves, cap_height, d_digests, d_cap, S(ctx)->stream));
    else
        HIP_TRY(merkle_tree_from_columns(d_cols, leaf_len, n_leaves, col_stride, cap_height, d_digests, d_cap, S(ctx)->stream));
    return ok();
}

GlError gl_merkle_tree_from_leaves_h(uint32_t hasher, const uint64_t *d_rows, uint32_t leaf_len, uint64_t n_leaves, uint32_t cap_height,
                                     uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    DeviceCall device_call(ctx);
    if (const char *why = tree_argument_error(hasher, d_rows, leaf_len, n_leaves, n_leaves, cap_height, d_digests, d_cap, ctx))
        return fail(GL_E_INVALID, why);
    if (hasher == GL_HASHER_KECCAK25)
        HIP_TRY(keccak_merkle_tree(d_rows, leaf_len, 1, leaf_len, n_leaves, cap_height, d_digests, d_cap, S(ctx)->stream));
    else
        HIP_TRY(merkle_tree_from_rows(d_rows, leaf_len, n_leaves, cap_height, d_digests, d_cap, S(ctx)->stream));
    return ok();
}

GlError gl_commit_from_coeffs_h(uint32_t hasher, const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                                uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde, uint64_t *d_leaves,
                                uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    DeviceCall device_call(ctx);
    return commit_from_coeffs(hasher, d_coeffs, poly_num, log_n, rate_bits, cap_height, salt_size, shift, d_lde, d_leaves, d_digests, d_cap, S(ctx));
}

// the argument check, then the inverse NTT in place, then the commit: a refused call leaves d_values as it was
GlError gl_commit_from_values_h(uint32_t hasher, uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                                uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde, uint64_t *d_leaves,
                                uint64_t *d_digests, uint64_t *d_cap, void *ctx) {
    DeviceCall device_call(ctx);
    if (const char *why = commit_argument_error(hasher, d_values, poly_num, log_n, rate_bits, cap_height, salt_size, d_lde, d_digests, d_cap, ctx))
        return fail(GL_E_INVALID, why);
    GlError e = gl_ntt_batch(d_values, poly_num, log_n, 1ull << log_n, 1, 0, ctx);
    if (e.code) return e;
    return commit_from_coeffs(hasher, d_values, poly_num, log_n, rate_bits, cap_height, salt_size, shift, d_lde, d_leaves, d_digests, d_cap, S(ctx));
}

// ---------------------------------------------------------------- the lookup columns of a trace (lookup.hip)
static bool words_overlap(const uint64_t *a, const uint64_t *b, uint64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * 8;
    return x < y + bytes && y < x + bytes;
}

static const char *lookup_argument_error(uint64_t n, const void *d_scratch, const void *ctx) {
    if (n < 1 || n > LOOKUP_MAX_N) return "n must be in 1 ..= 2^30";
    if (!d_scratch || !ctx) return "null pointer";
    if ((uintptr_t)d_scratch & 15) return "d_scratch must be 16-byte aligned";
    return nullptr;
}

uint64_t gl_lookup_scratch_bytes(uint64_t n) {
    if (n < 1 || n > LOOKUP_MAX_N) return 0;
    return lookup_scratch_layout(nullptr, n).words * 8;
}

GlError gl_sort_canonical(const uint64_t *d_in, uint64_t *d_out, uint64_t n, void *d_scratch, void *ctx) {
    DeviceCall device_call(ctx);
    if (const char *why = lookup_argument_error(n, d_scratch, ctx)) return fail(GL_E_INVALID, std::string("gl_sort_canonical: ") + why);
    if (!d_in || !d_out) return fail(GL_E_INVALID, "gl_sort_canonical: null pointer");
    if (d_in != d_out && words_overlap(d_in, d_out, n)) return fail(GL_E_INVALID, "gl_sort_canonical: d_out overlaps d_in without being d_in");
    HIP_TRY(lookup_sort_canonical(d_in, d_out, n, lookup_scratch_layout(d_scratch, n), S(ctx)->stream));
    return ok();
}

GlError gl_lookup_permuted_cols(const uint64_t *d_inputs, const uint64_t *d_table, uint64_t n, uint64_t *d_permuted_inputs,
                                uint64_t *d_permuted_table, void *d_scratch, void *ctx) {
    DeviceCall device_call(ctx);
    if (const char *why = lookup_argument_error(n, d_scratch, ctx)) return fail(GL_E_INVALID, std::string("gl_lookup_permuted_cols: ") + why);
    if (!d_inputs || !d_table || !d_permuted_inputs || !d_permuted_table) return fail(GL_E_INVALID, "gl_lookup_permuted_cols: null pointer");
    if (words_overlap(d_permuted_inputs, d_permuted_table, n)) return fail(GL_E_INVALID, "gl_lookup_permuted_cols: the two outputs overlap");
    for (const uint64_t *out : {d_permuted_inputs, d_permuted_table})
        if (words_overlap(out, d_inputs, n) || words_overlap(out, d_table, n))
            return fail(GL_E_INVALID, "gl_lookup_permuted_cols: an output overlaps an input");
    HIP_TRY(lookup_permuted_cols(d_inputs, d_table, n, d_permuted_inputs, d_permuted_table, lookup_scratch_layout(d_scratch, n), S(ctx)->stream));
    return ok();
}

GlError gl_stark_fill_lookups(uint64_t *d_trace, uint64_t trace_stride, uint64_t n, uint32_t num_columns, const uint32_t *h_lookups,
                              uint32_t num_lookups, void *d_scratch, void *ctx) {
    DeviceCall device_call(ctx);
    if (const char *why = lookup_argument_error(n, d_scratch, ctx)) return fail(GL_E_INVALID, std::string("gl_stark_fill_lookups: ") + why);
    if (!d_trace || (!h_lookups && num_lookups)) return fail(GL_E_INVALID, "gl_stark_fill_lookups: null pointer");
    if (trace_stride < n) return fail(GL_E_INVALID, "gl_stark_fill_lookups: trace_stride smaller than n: the columns would overlap");
    for (uint32_t i = 0; i < 4 * num_lookups; ++i)
        if (h_lookups[i] >= num_columns) return fail(GL_E_INVALID, "gl_stark_fill_lookups: column out of range");
    for (uint32_t l = 0; l < num_lookups; ++l)
        for (uint32_t w = 2; w < 4; ++w)  // a column this call writes is no other column of the call
            for (uint32_t i = 0; i < 4 * num_lookups; ++i)
                if (i != 4 * l + w && h_lookups[i] == h_lookups[4 * l + w])
                    return fail(GL_E_INVALID, "gl_stark_fill_lookups: a permuted column is also an input, table or permuted column of the call");
    const LookupScratch scratch = lookup_scratch_layout(d_scratch, n);
    for (uint32_t l = 0; l < num_lookups; ++l) {
        const uint32_t *c = h_lookups + 4 * l;
        HIP_TRY(lookup_permuted_cols(d_trace + c[0] * trace_stride, d_trace + c[1] * trace_stride, n, d_trace + c[2] * trace_stride,
                                     d_trace + c[3] * trace_stride, scratch, S(ctx)->stream));
    }
    return ok();
}

}  // extern "C"
