// stark_jit_device.h — what every run-time compiled STARK quotient kernel (stark_jit.hip) has in common with the interpreter
// (stark_quotient_values_kernel, stark.hip): the kernel's arguments, the head — the point's rows, x, Z_H, z_last and the two Lagrange
// selectors from one inversion — starky's ConstraintConsumer, and the tail — the multiply by 1 / Z_H and the canonical store.
// Compiled twice: by hipcc into the library (the host fills StarkJitArgs) and, as a raw string behind gl_field.h, by hiprtc in
// front of the generated body.
#pragma once
#ifndef GL_JIT
#include <stdint.h>

#include "gl_field.h"
#endif

// Everything that varies per proof, by value: two launches of one kernel from two host threads share nothing but the code.
struct StarkJitArgs {
    const uint64_t *pis, *trace, *zs, *twl, *twh;
    uint64_t *out;
    uint64_t stride;
    uint32_t degree_bits, pad_;
    uint64_t shift, g_inv;  // the coset shift; 1 / g = the last element of the subgroup
    uint64_t alpha[4];
    uint64_t zh[16], zh_inv[16];              // Z_H on the coset takes 2^qdb values (field/src/zero_poly_coset.rs:20-41)
    uint64_t perm_beta[64], perm_gamma[64];   // [set][challenge], num_challenges wide
    uint64_t ctl_beta[4], ctl_gamma[4];       // [challenge]
};

#if defined(GL_JIT) || defined(__HIPCC__)
namespace sj {

// w_{2^log}^i through the two-level table of w_{2^24} (plonk_device.h)
__device__ __forceinline__ uint64_t root_pow(const uint64_t *twl, const uint64_t *twh, uint32_t log, uint64_t i) {
    uint32_t e = (uint32_t)(i << (24 - log)) & 0xFFFFFFu;
    uint64_t h = twh[e >> 12];
    uint32_t lo = e & 4095u;
    return lo ? gl::mul(h, twl[lo]) : h;
}

// x^(p-2): with e_k = x^(2^k - 1), p - 2 = (2^31 - 1) 2^33 + (2^32 - 1) (plonk_device.h)
__device__ __forceinline__ uint64_t sqn(uint64_t v, int k) {
    for (int i = 0; i < k; i++) v = gl::sqr(v);
    return v;
}
__device__ __forceinline__ uint64_t inverse_chain(uint64_t x) {
    const uint64_t e2 = gl::mul(gl::sqr(x), x), e3 = gl::mul(gl::sqr(e2), x), e6 = gl::mul(sqn(e3, 3), e3), e12 = gl::mul(sqn(e6, 6), e6);
    const uint64_t e15 = gl::mul(sqn(e12, 3), e3), e30 = gl::mul(sqn(e15, 15), e15), e31 = gl::mul(gl::sqr(e30), x), e32 = gl::mul(gl::sqr(e31), x);
    return gl::mul(sqn(e31, 33), e32);
}

// The point of thread t: leaf t of the quotient domain of size n << QDB holds point i = reverse_bits(t); its next row (point
// i + 2^QDB, wrapping: prover.rs:262) is leaf t_next.
struct Point {
    uint64_t t, t_next, i, size;
    const uint64_t *local, *next;  // the row's element of column 0
    uint64_t z_last, l_first, l_last, zh_inv;
};

// false: the thread is beyond the domain
template <uint32_t QDB>
__device__ __forceinline__ bool head(const StarkJitArgs &p, Point &q) {
    const uint32_t log_size = p.degree_bits + QDB;
    const uint64_t n = 1ull << p.degree_bits;
    q.size = 1ull << log_size;
    q.t = (uint64_t)blockIdx.x * 128u + threadIdx.x;
    if (q.t >= q.size) return false;
    q.i = __brevll(q.t) >> (64 - log_size);  // degree_bits >= 1: log_size >= 1
    const uint64_t i_next = (q.i + (1ull << QDB)) & (q.size - 1);
    q.t_next = __brevll(i_next) >> (64 - log_size);
    q.local = p.trace + q.t, q.next = p.trace + q.t_next;
    const uint64_t x = gl::mul(p.shift, root_pow(p.twl, p.twh, log_size, q.i));
    uint64_t zh = p.zh[0];
    q.zh_inv = p.zh_inv[0];
    const uint32_t which = (uint32_t)q.i & ((1u << QDB) - 1);
#pragma unroll
    for (uint32_t e = 1; e < (1u << QDB); e++) {
        zh = which == e ? p.zh[e] : zh;
        q.zh_inv = which == e ? p.zh_inv[e] : q.zh_inv;
    }
    // ConstraintConsumer::new (prover.rs:266-275): z_last = x - g^(n-1); L_k(x) = g^k Z_H(x) / (n (x - g^k)) for k = 0 and
    // k = n - 1 (g^(n-1) = 1 / g). x lies on the coset, never in the subgroup: one inversion serves both.
    q.z_last = gl::sub(x, p.g_inv);
    const uint64_t d_first = gl::mul(n, gl::sub(x, 1)), d_last = gl::mul(n, q.z_last);
    const uint64_t d_inv = inverse_chain(gl::mul(d_first, d_last));
    q.l_first = gl::mul(zh, gl::mul(d_inv, d_last));
    q.l_last = gl::mul(gl::mul(p.g_inv, zh), gl::mul(d_inv, d_first));
    return true;
}

// ConstraintConsumer::constraint (constraint_consumer.rs:59-64): acc <- acc * alpha + c per challenge
template <uint32_t NCH>
__device__ __forceinline__ void constraint(uint64_t (&sums)[NCH], const StarkJitArgs &p, uint64_t v) {
#pragma unroll
    for (uint32_t c = 0; c < NCH; c++) sums[c] = gl::mac(v, sums[c], p.alpha[c]);
}

// prover.rs:296-302
template <uint32_t NCH>
__device__ __forceinline__ void tail(const uint64_t (&sums)[NCH], const StarkJitArgs &p, const Point &q) {
#pragma unroll
    for (uint32_t c = 0; c < NCH; c++) p.out[(uint64_t)c * q.size + q.i] = gl::canon(gl::mul(sums[c], q.zh_inv));
}

// ACC: plain (wrapping-free by contract) sums of the 32-bit halves, both as ONE statement of two multiply-adds with the weight a
// scalar operand — left to itself the compiler strength-reduces small constant weights into shifts and adds (gate_jit.hip)
__device__ __forceinline__ void acc(uint64_t &al, uint64_t &ah, uint64_t x, uint32_t k) {
    asm("v_mad_u64_u32 %0, vcc, %2, %4, %0\n\tv_mad_u64_u32 %1, vcc, %3, %4, %1" : "+v"(al), "+v"(ah) : "v"((uint32_t)x), "v"((uint32_t)(x >> 32)), "s"(k) : "vcc");
}

}  // namespace sj
#endif
