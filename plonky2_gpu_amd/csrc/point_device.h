// point_device.h — what a kernel needs to stand at a point of a multiplicative coset: powers of the roots of unity from the
// two-level twiddle table and the Fermat inversion chain. Compiled by hipcc into the library (plonk_device.h, stark_jit_device.h)
// and, as a raw string behind gl_field.h, by hiprtc in front of the generated STARK quotient kernels: no system header here.
#pragma once
#ifndef GL_JIT
#include <stdint.h>

#include "gl_field.h"
#endif

#if defined(GL_JIT) || defined(__HIPCC__)
namespace pt {

// w_{2^log}^i through the two-level table of w_{2^24}
__device__ __forceinline__ uint64_t root_pow(const uint64_t *twl, const uint64_t *twh, uint32_t log, uint64_t i) {
    uint32_t e = (uint32_t)(i << (24 - log)) & 0xFFFFFFu;
    uint64_t h = twh[e >> 12];
    uint32_t lo = e & 4095u;
    return lo ? gl::mul(h, twl[lo]) : h;
}

__device__ __forceinline__ uint64_t sqn(uint64_t v, int k) {
    for (int i = 0; i < k; i++) v = gl::sqr(v);
    return v;
}
// x^(p-2): with e_k = x^(2^k - 1), p - 2 = (2^31 - 1) 2^33 + (2^32 - 1)
__device__ __forceinline__ uint64_t inverse_chain(uint64_t x) {
    const uint64_t e2 = gl::mul(gl::sqr(x), x), e3 = gl::mul(gl::sqr(e2), x), e6 = gl::mul(sqn(e3, 3), e3), e12 = gl::mul(sqn(e6, 6), e6);
    const uint64_t e15 = gl::mul(sqn(e12, 3), e3), e30 = gl::mul(sqn(e15, 15), e15), e31 = gl::mul(gl::sqr(e30), x), e32 = gl::mul(gl::sqr(e31), x);
    return gl::mul(sqn(e31, 33), e32);
}

}  // namespace pt
#endif
