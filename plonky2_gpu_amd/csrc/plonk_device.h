// plonk_device.h — device helpers shared by the permutation-argument kernels of plonk.hip and stark.hip: powers of the roots of
// unity and the Fermat inversion chain (point_device.h), and the exclusive prefix product over the rows of a column (block scan +
// scan of the block totals; the caller multiplies the two in its own finalising kernel).
// Everything sits in an unnamed namespace: each translation unit that includes this gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl_field.h"
#include "point_device.h"

namespace plonky2_hip {

namespace {

using pt::inverse_chain, pt::root_pow;  // point_device.h

__device__ __forceinline__ uint64_t inverse(uint64_t x) { return gl::pow(x, gl::P - 2); }

// ---- exclusive prefix product over rows ---------------------------------------------------------
constexpr int SCAN_T = 256, SCAN_E = 4, SCAN_B = SCAN_T * SCAN_E;

__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t *lds, uint64_t *total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_T; off <<= 1) {
        uint64_t x = (t >= (uint32_t)off) ? gl::mul(lds[t - off], lds[t]) : lds[t];
        __syncthreads();
        lds[t] = x;
        __syncthreads();
    }
    uint64_t incl = lds[t];
    uint64_t excl = t ? lds[t - 1] : 1;
    if (total && t == SCAN_T - 1) *total = incl;
    __syncthreads();
    return excl;
}

// in place: v[i] <- product of the block's earlier elements; totals[blk] <- product of the block
__global__ __launch_bounds__(SCAN_T) void scan_blocks_kernel(uint64_t *v, uint64_t n, uint64_t col_stride, uint64_t *totals,
                                                             uint64_t totals_stride) {
    __shared__ uint64_t lds[SCAN_T];
    uint64_t *col = v + (uint64_t)blockIdx.y * col_stride;
    uint64_t base = (uint64_t)blockIdx.x * SCAN_B + (uint64_t)threadIdx.x * SCAN_E;
    uint64_t e[SCAN_E];
    uint64_t p = 1;
#pragma unroll
    for (int k = 0; k < SCAN_E; k++) {
        e[k] = base + k < n ? col[base + k] : 1;
        p = gl::mul(p, e[k]);
    }
    uint64_t excl = block_exclusive_scan(p, lds, totals + (uint64_t)blockIdx.y * totals_stride + blockIdx.x);
#pragma unroll
    for (int k = 0; k < SCAN_E; k++) {
        if (base + k < n) col[base + k] = gl::canon(excl);
        excl = gl::mul(excl, e[k]);
    }
}

// exclusive scan of m block totals per column by one workgroup
__global__ __launch_bounds__(SCAN_T) void scan_totals_kernel(uint64_t *totals, uint64_t m, uint64_t totals_stride) {
    __shared__ uint64_t lds[SCAN_T];
    uint64_t *t = totals + (uint64_t)blockIdx.x * totals_stride;
    uint64_t per = (m + SCAN_T - 1) / SCAN_T;
    uint64_t lo = (uint64_t)threadIdx.x * per, hi = lo + per < m ? lo + per : m;
    uint64_t p = 1;
    for (uint64_t i = lo; i < hi; i++) p = gl::mul(p, t[i]);
    uint64_t excl = block_exclusive_scan(p, lds, nullptr);
    for (uint64_t i = lo; i < hi; i++) {
        uint64_t x = t[i];
        t[i] = excl;
        excl = gl::mul(excl, x);
    }
}

}  // namespace

}  // namespace plonky2_hip
