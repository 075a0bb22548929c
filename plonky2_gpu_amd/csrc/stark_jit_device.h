// stark_jit_device.h — what the interpreter of a STARK's register program (stark_quotient_values_kernel, stark.hip) and every
// run-time compiled STARK quotient kernel (stark_jit.hip) have in common: the per-proof arguments, the head — the point's rows, x,
// Z_H, z_last and the two Lagrange selectors from one inversion — starky's ConstraintConsumer, and the tail — the multiply by
// 1 / Z_H and the canonical store. Compiled twice: by hipcc into the library (stark_point_args fills StarkJitArgs) and, as a raw string
// behind gl_field.h and point_device.h, by hiprtc in front of the generated body. The interpreter's qdb and num_challenges are
// run-time values, the compiled kernels' literals: arguments here, which the generated text leaves to their defaults or to head<QDB>.
#pragma once
#ifndef GL_JIT
#include <stdint.h>

#include "gl_field.h"
#include "point_device.h"
#endif

// Everything that varies per proof, by value: two launches of one kernel from two host threads share nothing but the code.
struct StarkJitArgs {
    const uint64_t *pis, *trace, *zs, *twl, *twh;
    uint64_t *out;
    uint64_t stride;
    uint32_t degree_bits, pad_;
    uint64_t shift, g_inv;  // the coset shift; 1 / g = the last element of the subgroup
    uint64_t alpha[4];
    uint64_t zh[16], zh_inv[16];  // Z_H on the coset takes 2^qdb values (field/src/zero_poly_coset.rs:20-41)
    uint64_t perm_beta[64], perm_gamma[64];  // [set][challenge], num_challenges wide
    uint64_t ctl_beta[4], ctl_gamma[4];      // [challenge]
};

#if defined(GL_JIT) || defined(__HIPCC__)
namespace sj {

// The point of thread t: leaf t of the quotient domain of size n << qdb holds point i = reverse_bits(t); its next row (point
// i + 2^qdb, wrapping: prover.rs:262) is leaf t_next.
struct Point {
    uint64_t t, t_next, i, size, n;  // n: the rows of the trace
    const uint64_t *local, *next;  // the row's element of column 0
    uint64_t z_last, l_first, l_last, zh_inv;
};

// the thread's leaf (blocks of 128 threads) and the size of the domain; false: the thread is beyond the domain
__device__ __forceinline__ bool locate(const StarkJitArgs &p, uint32_t qdb, Point &q) {
    const uint32_t log_size = p.degree_bits + qdb;
    q.n = 1ull << p.degree_bits;
    q.size = 1ull << log_size;
    q.t = (uint64_t)blockIdx.x * 128u + threadIdx.x;
    return q.t < q.size;
}

// The rest of the Point of a located thread. `one_point`: the domain may be the single point of degree_bits = qdb = 0, which has no
// bits to reverse (the interpreter's; the compiled route refuses degree_bits = 0 on the host, where the test would cost two selects).
__device__ __forceinline__ void head(const StarkJitArgs &p, uint32_t qdb, Point &q, bool one_point = false) {
    const uint32_t log_size = p.degree_bits + qdb;
    q.i = one_point && !log_size ? 0 : __brevll(q.t) >> (64 - log_size);
    const uint64_t i_next = (q.i + (1ull << qdb)) & (q.size - 1);
    q.t_next = one_point && !log_size ? 0 : __brevll(i_next) >> (64 - log_size);
    q.local = p.trace + q.t, q.next = p.trace + q.t_next;
    const uint64_t x = gl::mul(p.shift, pt::root_pow(p.twl, p.twh, log_size, q.i));
    uint64_t zh = p.zh[0];
    q.zh_inv = p.zh_inv[0];
    const uint32_t which = (uint32_t)q.i & ((1u << qdb) - 1);
    for (uint32_t e = 1; e < (1u << qdb); e++) {
        zh = which == e ? p.zh[e] : zh;
        q.zh_inv = which == e ? p.zh_inv[e] : q.zh_inv;
    }
    // ConstraintConsumer::new (prover.rs:266-275): z_last = x - g^(n-1); the two Lagrange selectors in closed form,
    // L_k(x) = g^k Z_H(x) / (n (x - g^k)) for k = 0 and k = n - 1 (g^(n-1) = 1 / g) — the values the reference gets by LDE of the
    // selector columns. x lies on the coset, never in the subgroup: both denominators are non-zero and one inversion serves both.
    q.z_last = gl::sub(x, p.g_inv);
    const uint64_t d_first = gl::mul(q.n, gl::sub(x, 1)), d_last = gl::mul(q.n, q.z_last);
    const uint64_t d_inv = pt::inverse_chain(gl::mul(d_first, d_last));
    q.l_first = gl::mul(zh, gl::mul(d_inv, d_last));
    q.l_last = gl::mul(gl::mul(p.g_inv, zh), gl::mul(d_inv, d_first));
}
template <uint32_t QDB>  // what the generated text calls
__device__ __forceinline__ bool head(const StarkJitArgs &p, Point &q) {
    if (!locate(p, QDB, q)) return false;
    head(p, QDB, q);
    return true;
}

// ConstraintConsumer::constraint (constraint_consumer.rs:59-64): acc <- acc * alpha + c for the first `nch` challenges
template <uint32_t N>
__device__ __forceinline__ void constraint(uint64_t (&sums)[N], const StarkJitArgs &p, uint64_t v, uint32_t nch = N) {
#pragma unroll
    for (uint32_t c = 0; c < N; c++)
        if (c < nch) sums[c] = gl::mac(v, sums[c], p.alpha[c]);
}

// prover.rs:296-302
template <uint32_t N>
__device__ __forceinline__ void tail(const uint64_t (&sums)[N], const StarkJitArgs &p, const Point &q, uint32_t nch = N) {
#pragma unroll
    for (uint32_t c = 0; c < N; c++)
        if (c < nch) p.out[(uint64_t)c * q.size + q.i] = gl::canon(gl::mul(sums[c], q.zh_inv));
}

// ACC: plain (wrapping-free by contract) sums of the 32-bit halves, both as ONE statement of two multiply-adds with the weight a
// scalar operand — left to itself the compiler strength-reduces small constant weights into shifts and adds (gate_jit.hip)
__device__ __forceinline__ void acc(uint64_t &al, uint64_t &ah, uint64_t x, uint32_t k) {
    asm("v_mad_u64_u32 %0, vcc, %2, %4, %0\n\tv_mad_u64_u32 %1, vcc, %3, %4, %1" : "+v"(al), "+v"(ah) : "v"((uint32_t)x), "v"((uint32_t)(x >> 32)), "s"(k) : "vcc");
}

}  // namespace sj
#endif
