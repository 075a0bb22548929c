// keccak_f1600.h — keccak-f[1600] on the device with the whole state in registers, shared by the Keccak-256 tree hasher
// (keccak.hip) and the Keccak sponge table's chain kernel (keccak_sponge_table.hip).
//
// 25 lanes as 50 32-bit halves, 24 rounds unrolled, the round constants literals. A 64-bit rotation written on uint64_t becomes
// a pair of 64-bit shifts and an or; on the halves it is two v_alignbit_b32, and the three-input xors of theta and the chi step
// are one v_bitop3_b32 per half.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

struct KeccakState {
    uint32_t lo[25], hi[25];  // lane x + 5 y = A[x][y]
};

__device__ __forceinline__ uint32_t funnel(uint32_t high, uint32_t low, int n) {  // bits [63 - n .. 32 - n] of high:low shifted left, 0 < n < 32
    return (high << n) | (low >> (32 - n));
}

// a ^ b ^ c in one v_bitop3_b32 (truth table 0x96); the compiler finds the chi step's b ^ (~c & d) itself, but pairs up a chain of xors
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// (lo, hi) of a lane rotated left by n; n is a constant after unrolling
__device__ __forceinline__ void rotl64(uint32_t lo, uint32_t hi, int n, uint32_t &out_lo, uint32_t &out_hi) {
    if (n == 0) {
        out_lo = lo, out_hi = hi;
    } else if (n < 32) {
        out_lo = funnel(lo, hi, n), out_hi = funnel(hi, lo, n);
    } else if (n == 32) {
        out_lo = hi, out_hi = lo;
    } else {
        out_lo = funnel(hi, lo, n - 32), out_hi = funnel(lo, hi, n - 32);
    }
}

__device__ __forceinline__ void keccak_f1600(KeccakState &s) {
    constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                                 0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                                 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                                 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll
    for (int r = 0; r < 24; r++) {
        // theta
        uint32_t cl[5], ch[5];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            cl[x] = xor3(xor3(s.lo[x], s.lo[x + 5], s.lo[x + 10]), s.lo[x + 15], s.lo[x + 20]);
            ch[x] = xor3(xor3(s.hi[x], s.hi[x + 5], s.hi[x + 10]), s.hi[x + 15], s.hi[x + 20]);
        }
        // rho and pi on A ^ D, D[x] = C[x - 1] ^ rotl(C[x + 1], 1): B[y][2x + 3y] = rotl(A[x][y] ^ D[x], RHO[x][y])
        uint32_t bl[25], bh[25];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            uint32_t rl, rh;
            rotl64(cl[(x + 1) % 5], ch[(x + 1) % 5], 1, rl, rh);
#pragma unroll
            for (int y = 0; y < 5; y++)
                rotl64(xor3(s.lo[x + 5 * y], cl[(x + 4) % 5], rl), xor3(s.hi[x + 5 * y], ch[(x + 4) % 5], rh), RHO[x + 5 * y], bl[y + 5 * ((2 * x + 3 * y) % 5)], bh[y + 5 * ((2 * x + 3 * y) % 5)]);
        }
        // chi
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++) {
                s.lo[x + 5 * y] = bl[x + 5 * y] ^ (~bl[(x + 1) % 5 + 5 * y] & bl[(x + 2) % 5 + 5 * y]);
                s.hi[x + 5 * y] = bh[x + 5 * y] ^ (~bh[(x + 1) % 5 + 5 * y] & bh[(x + 2) % 5 + 5 * y]);
            }
        // iota
        s.lo[0] ^= (uint32_t)RC[r];
        s.hi[0] ^= (uint32_t)(RC[r] >> 32);
    }
}

}  // namespace plonky2_hip
