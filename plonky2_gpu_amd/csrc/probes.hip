// probes.hip — gl_debug_field_op / gl_debug_copy: kernels that exist only so that the tests can drive the field arithmetic and the
// NTT passes' register routines with chosen operands, and measure what a streaming copy moves.
#include "ctx.h"
#include "gl_field.h"
#include "ntt_kernels.h"

using namespace plonky2_hip;

namespace {

// Element-wise field ops, exported only so that the parity tests can drive gl_field.h with the
// reference's edge operands (field/src/prime_field_testing.rs:7-17).
template <int K>
__device__ uint64_t pow2_case(uint64_t x, int k) {
    if constexpr (K >= 192) {
        return 0;
    } else {
        return k == K ? gl::mul_pow2<K>(x) : pow2_case<K + 1>(x, k);
    }
}

// The deferred-rare-path forms (gl_field.h add_f / sub_f / mul_f / mul_pow2_f) the way the NTT passes use them: a GROUP of three
// independent operations on (x, y), (y, x), (x ^ y, x), one branch, the corrections behind it. `which` picks the member whose result is
// returned, so that the tests see the flagged operation first, in the middle and last in its group, beside unflagged neighbours.
template <int KIND>
__device__ uint64_t deferred_group(uint64_t x, uint64_t y, int which) {
    uint64_t a[3] = {x, y, x ^ y}, b[3] = {y, x, x}, r[3];
    gl::rare_mask f[3], fl[3] = {0, 0, 0};   // fl: sub_f's second mask (the missed carry)
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] = KIND == 0 ? gl::add_f(a[k], b[k], f[k]) : KIND == 1 ? gl::sub_f(a[k], b[k], f[k], fl[k]) : gl::mul_f(a[k], b[k], f[k]);
    if (GL_RARE_ANY(f[0] | f[1] | f[2] | fl[0] | fl[1] | fl[2])) {
#pragma unroll
        for (int k = 0; k < 3; k++) r[k] = KIND == 0 ? gl::add_fix(r[k], f[k]) : KIND == 1 ? gl::sub_fix(r[k], f[k], fl[k]) : gl::mul_fix(r[k], f[k]);
    }
    return which == 0 ? r[0] : which == 1 ? r[1] : r[2];
}
// canon_f / canon_fix the way the passes' tails use them: x, y and x ^ y flagged by one compare each, one branch, the exact
// conditional subtraction behind it; `which` as above. The kernel's own gl::canon of the result must then change nothing.
__device__ uint64_t canon_group(uint64_t x, uint64_t y, int which) {
    uint64_t r[3] = {x, y, x ^ y};
    gl::rare_mask f[3];
#pragma unroll
    for (int k = 0; k < 3; k++) gl::canon_f(r[k], f[k]);
    if (GL_RARE_ANY(f[0] | f[1] | f[2])) {
#pragma unroll
        for (int k = 0; k < 3; k++) r[k] = gl::canon_fix(r[k], f[k]);
    }
    return which == 0 ? r[0] : which == 1 ? r[1] : r[2];
}
template <int K>
__device__ uint64_t pow2f_case(uint64_t x, int k, bool alone) {
    if constexpr (K >= 96) {
        return 0;
    } else {
        if (k != K) return pow2f_case<K + 1>(x, k, alone);
        gl::rare_mask f0, f1;
        uint64_t r0 = gl::mul_pow2_f<K>(x, f0), r1 = gl::mul_pow2_f<K>(~x, f1);
        if (GL_RARE_ANY(f0 | f1)) r0 = gl::mul_pow2_fix<K>(r0, f0), r1 = gl::mul_pow2_fix<K>(r1, f1);
        return alone ? r0 : gl::add(r0, r1);  // x 2^K + ~x 2^K = (2^64 - 1) 2^K
    }
}

// A lazy-dot-product accumulator built from two test words, so that the parity tests can reach the
// reduction's rare wrap corrections directly (random Poseidon states hit them with probability ~2^-32).
//   mode 0: every field wide (a0 = x, a1 = y, a2 = ~x + (y << 13), small counters from the top bits)
//   mode 1: a0 = x, the other five fields packed into y as small numbers:
//           a1 = y[0:16), a2 = y[16:32), k0 = y[32:40), k1 = y[40:48), k2 = y[48:56)
__device__ gl::DotAcc dotacc_from(int mode, uint64_t x, uint64_t y) {
    gl::DotAcc d;
    if (mode == 0) {
        d.a0 = x, d.a1 = y, d.a2 = ~x + (y << 13);
        d.k0 = (uint32_t)(y >> 59), d.k1 = (uint32_t)(x >> 58), d.k2 = (uint32_t)((x ^ y) & 7);
    } else {
        d.a0 = x, d.a1 = y & 0xFFFF, d.a2 = (y >> 16) & 0xFFFF;
        d.k0 = (uint32_t)(y >> 32) & 0xFF, d.k1 = (uint32_t)(y >> 40) & 0xFF, d.k2 = (uint32_t)(y >> 48) & 0xFF;
    }
    return d;
}

// What a streaming kernel can move on this device (the measured roof next to the 8 TB/s specification): 16 B per lane,
// eight independent pieces per thread in flight, non-temporal loads and stores (the bytes are touched once: default-policy
// accesses reach 4.9-5.6 TB/s in the same shape, non-temporal ones 6.2 TB/s = the guide's 6.3 figure;
// tools/ubench_mem.hip, profiles/r02_ubench_mem.txt).
constexpr int COPY_UNROLL = 8;
__global__ __launch_bounds__(256) void copy16_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t n16) {
    const uint64_t base = (uint64_t)blockIdx.x * (256 * COPY_UNROLL) + threadIdx.x;
    uint64_t v[COPY_UNROLL][2];
#pragma unroll
    for (int u = 0; u < COPY_UNROLL; u++) {
        const uint64_t i = base + (uint64_t)u * 256;
        if (i < n16) {
            v[u][0] = __builtin_nontemporal_load(in + 2 * i);
            v[u][1] = __builtin_nontemporal_load(in + 2 * i + 1);
        }
    }
#pragma unroll
    for (int u = 0; u < COPY_UNROLL; u++) {
        const uint64_t i = base + (uint64_t)u * 256;
        if (i < n16) {
            __builtin_nontemporal_store(v[u][0], out + 2 * i);
            __builtin_nontemporal_store(v[u][1], out + 2 * i + 1);
        }
    }
}

__global__ void field_op_kernel(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t x = a[i], y = b ? b[i] : 0, r = 0;
    switch (op) {
        case 0: r = gl::add(x, y); break;
        case 1: r = gl::sub(x, y); break;
        case 2: r = gl::mul(x, y); break;
        case 3: r = gl::neg(x); break;
        case 4: r = gl::pow7(x); break;
        case 5: r = gl::mac(x, y, y); break;
        case 6: r = pow2_case<0>(x, (int)(y % 192)); break;
        case 7: r = gl::add_canonical(x, gl::canon(y)); break;
        case 8: r = gl::add_c(gl::canon_c(x), gl::canon_c(y)); break;
        case 9: r = gl::sub_c(gl::canon_c(x), gl::canon_c(y)); break;
        case 10: r = gl::mul_c(x, y); break;
        case 11: r = gl::canon_c(x); break;
        case 12: { uint64_t lo, hi; gl::mul_wide(x, y, lo, hi); r = gl::reduce128_c(lo ^ y, hi ^ x) ; } break;
        case 13: r = gl::dot_finish(dotacc_from(0, x, y)); break;
        case 14: r = gl::dot_finish_generic(dotacc_from(0, x, y)); break;
        case 15: r = gl::dot_finish(dotacc_from(1, x, y)); break;
        case 16: r = gl::dot_finish_generic(dotacc_from(1, x, y)); break;
        case 17: r = gl::fold96(x, y & 0x7FFFFFFFFFFFFFFFull); break;  // x + (y mod 2^63) * 2^32: the ACC accumulators' fold
        case 18: case 19: case 20: r = deferred_group<0>(x, y, op - 18); break;
        case 21: case 22: case 23: r = deferred_group<1>(x, y, op - 21); break;
        case 24: case 25: case 26: r = deferred_group<2>(x, y, op - 24); break;
        case 27: r = pow2f_case<0>(x, (int)((uint32_t)y % 96), (y >> 32) != 0); break;
        case 28: case 29: case 30: r = canon_group(x, y, op - 28); break;
        default: r = x; break;
    }
    out[i] = ((op >= 8 && op <= 12) || (op >= 28 && op <= 30)) ? r : gl::canon(r);  // canonical-domain ops (and canon_fix) must already be canonical
}

}  // namespace

extern "C" {

GlError gl_debug_copy(void *d_dst, const void *d_src, uint64_t bytes, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_dst || !d_src) return fail(GL_E_INVALID, "null pointer");
    if ((bytes & 15) || (((uintptr_t)d_dst | (uintptr_t)d_src) & 15)) return fail(GL_E_INVALID, "16-byte granularity");
    if (bytes == 0) return ok();
    const uint64_t n16 = bytes / 16, per_block = 256ull * COPY_UNROLL;
    hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)((n16 + per_block - 1) / per_block)), dim3(256), 0, S(ctx)->stream,
                       static_cast<const uint64_t *>(d_src), static_cast<uint64_t *>(d_dst), n16);
    HIP_TRY(hipGetLastError());
    return ok();
}

// ops 100 .. 109 of gl_debug_field_op: the register-level radix routines of the NTT passes (ntt_kernels.h) on vectors of sixteen
// elements, one vector per lane — so that the tests can drive their DEFERRED CORRECTION paths with operands that flag (inside a
// transform only the first stage of the first pass ever sees such operands):
//   100 + s (s = 0..3): radix_dif_stage<4, 0, s>      104: radix_dif<4, 0>      105: radix_dif_blocks<2>
//   106 + k (k = 0..3): shift_twiddles_radix4<k>
__global__ void radix_probe_kernel(int which, const uint64_t *in, uint64_t *out, uint64_t n_vec) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t j = i < n_vec ? i : n_vec - 1;   // every lane computes (the masks are per wave); the store is predicated
    uint64_t v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = in[j * 16 + k];
    using namespace nttk;
    switch (which) {
        case 0: radix_dif_stage<4, 0, 0>(v); break;
        case 1: radix_dif_stage<4, 0, 1>(v); break;
        case 2: radix_dif_stage<4, 0, 2>(v); break;
        case 3: radix_dif_stage<4, 0, 3>(v); break;
        case 4: radix_dif<4, 0>(v); break;
        case 5: radix_dif_blocks<2>(v); break;
        case 6: shift_twiddles_radix4<0>(v); break;
        case 7: shift_twiddles_radix4<1>(v); break;
        case 8: shift_twiddles_radix4<2>(v); break;
        default: shift_twiddles_radix4<3>(v); break;
    }
    if (i < n_vec)
#pragma unroll
        for (int k = 0; k < 16; k++) out[i * 16 + k] = gl::canon(v[k]);
}

GlError gl_debug_field_op(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, uint64_t n, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_a || !d_out) return fail(GL_E_INVALID, "null pointer");
    if (n == 0) return ok();
    if (op >= 100 && op < 110) {
        if (n % 16) return fail(GL_E_INVALID, "ops 100-109 take vectors of sixteen elements");
        const uint64_t n_vec = n / 16;
        hipLaunchKernelGGL(radix_probe_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, S(ctx)->stream, op - 100, d_a, d_out, n_vec);
        HIP_TRY(hipGetLastError());
        return ok();
    }
    hipLaunchKernelGGL(field_op_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(ctx)->stream, op, d_a, d_b,
                       d_out, n);
    HIP_TRY(hipGetLastError());
    return ok();
}

}  // extern "C"
