// keccak_table.hip — the trace of the reference's Keccak-f table (evm/src/keccak/keccak_stark.rs:53-204) built on the device:
// 2430 columns, 24 rows per permutation, every cell a bit, a 32-bit limb or a round flag.
//
// One thread per ROW. Row i belongs to permutation k = i / 24 and round r = i % 24. The thread loads the 25 input words of
// permutation k (the zero state for the padding permutations behind the inputs; the lanes of a wave share two or three
// permutations, so the loads are broadcasts), runs rounds 0 .. r - 1 on 25 words in registers to obtain the round's input A,
// and then computes the one round whose intermediate values the row holds:
//     C[x]     = xor_y A[x, y]                          C'[x] = C[x] ^ C[x - 1] ^ rotl(C[x + 1], 1)
//     A'[x, y] = A[x, y] ^ C[x] ^ C'[x]                 B[x, y] = rotl(A'[a, x], R[a][x]) with a = (x + 3 y) mod 5
//     A''[x, y] = B[x, y] ^ (~B[x + 1, y] & B[x + 2, y])      A'''[0, 0] = A''[0, 0] ^ RC[r]
// Recomputing up to 23 rounds per row (about 12 on average, a few thousand 32-bit logic operations) costs far less than an
// exchange between rows would: the row then issues 2430 stores of 8 bytes, and consecutive lanes are consecutive rows of a
// column, so every store instruction of a wave writes four whole 128-byte lines. The kernel is bound by those stores:
// 2430 * 8 * n bytes. The x / y loops are unrolled so that the state is never indexed by a register; the bit index z is a
// run-time loop per 32-bit limb ((limb >> z) & 1), which keeps the code at 28 KB (394 store instructions) instead of 2430 store sequences.
#include "keccak_table.h"

#include "ctx.h"

namespace plonky2_hip {

namespace {

__constant__ uint64_t KT_RC[KECCAK_TABLE_ROUNDS] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// the rotation of lane (x, y) (columns.rs:43-49)
__device__ __forceinline__ constexpr uint32_t kt_rot(uint32_t x, uint32_t y) {
    constexpr uint8_t R[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};
    return R[x][y];
}

// One round without its constant on a[5 x + y]: every intermediate value a row of the table holds
__device__ __forceinline__ void kt_round(const uint64_t (&a)[25], uint64_t (&c)[5], uint64_t (&cp)[5], uint64_t (&ap)[25], uint64_t (&app)[25]) {
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) c[x] = a[5 * x] ^ a[5 * x + 1] ^ a[5 * x + 2] ^ a[5 * x + 3] ^ a[5 * x + 4];
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) cp[x] = c[x] ^ c[(x + 4) % 5] ^ __builtin_rotateleft64(c[(x + 1) % 5], 1);
#pragma unroll
    for (uint32_t x = 0; x < 5; x++)
#pragma unroll
        for (uint32_t y = 0; y < 5; y++) ap[5 * x + y] = a[5 * x + y] ^ c[x] ^ cp[x];
#pragma unroll
    for (uint32_t y = 0; y < 5; y++) {
        uint64_t b[5];
#pragma unroll
        for (uint32_t x = 0; x < 5; x++) b[x] = __builtin_rotateleft64(ap[5 * ((x + 3 * y) % 5) + x], kt_rot((x + 3 * y) % 5, x));
#pragma unroll
        for (uint32_t x = 0; x < 5; x++) app[5 * x + y] = b[x] ^ (~b[(x + 1) % 5] & b[(x + 2) % 5]);
    }
}

// the 64 bit columns of one word, from column `col` on, at this thread's row
__device__ __forceinline__ void kt_store_bits(uint64_t *__restrict__ col, uint64_t stride, uint64_t w) {
    const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
#pragma unroll 4
    for (uint32_t z = 0; z < 32; z++) col[(uint64_t)z * stride] = (lo >> z) & 1u;
#pragma unroll 4
    for (uint32_t z = 0; z < 32; z++) col[(uint64_t)(32 + z) * stride] = (hi >> z) & 1u;
}

__device__ __forceinline__ void kt_store_limbs(uint64_t *__restrict__ col, uint64_t stride, uint64_t w) {
    col[0] = w & 0xFFFFFFFFull;
    col[stride] = w >> 32;
}

__global__ __launch_bounds__(KECCAK_TABLE_THREADS) void keccak_table_trace_kernel(const uint64_t *__restrict__ inputs, uint64_t num_inputs, uint64_t n,
                                                                                  uint64_t *__restrict__ trace, uint64_t stride) {
    const uint64_t row = (uint64_t)blockIdx.x * KECCAK_TABLE_THREADS + threadIdx.x;
    if (row >= n) return;
    const uint64_t perm = row / KECCAK_TABLE_ROUNDS;
    const uint32_t round = (uint32_t)(row % KECCAK_TABLE_ROUNDS);

    uint64_t a[25], c[5], cp[5], ap[25], app[25];
    const bool real = perm < num_inputs;  // else a padding permutation: the zero state
#pragma unroll
    for (uint32_t x = 0; x < 5; x++)
#pragma unroll
        for (uint32_t y = 0; y < 5; y++) a[5 * x + y] = real ? inputs[perm * 25 + 5 * y + x] : 0;
    for (uint32_t r = 0; r < round; r++) {
        kt_round(a, c, cp, ap, app);
#pragma unroll
        for (uint32_t j = 0; j < 25; j++) a[j] = app[j];
        a[0] ^= KT_RC[r];
    }
    kt_round(a, c, cp, ap, app);

    uint64_t *out = trace + row;
#pragma unroll 4
    for (uint32_t i = 0; i < KECCAK_TABLE_ROUNDS; i++) out[(uint64_t)i * stride] = i == round ? 1 : 0;
#pragma unroll
    for (uint32_t j = 0; j < 25; j++) kt_store_limbs(out + (uint64_t)(KT_A + 2 * j) * stride, stride, a[j]);
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) kt_store_bits(out + (uint64_t)(KT_C + 64 * x) * stride, stride, c[x]);
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) kt_store_bits(out + (uint64_t)(KT_C_PRIME + 64 * x) * stride, stride, cp[x]);
#pragma unroll
    for (uint32_t j = 0; j < 25; j++) kt_store_bits(out + (uint64_t)(KT_A_PRIME + 64 * j) * stride, stride, ap[j]);
#pragma unroll
    for (uint32_t j = 0; j < 25; j++) kt_store_limbs(out + (uint64_t)(KT_A_PRIME2 + 2 * j) * stride, stride, app[j]);
    kt_store_bits(out + (uint64_t)KT_A_PRIME2_BITS * stride, stride, app[0]);
    kt_store_limbs(out + (uint64_t)KT_A_PRIME3_00 * stride, stride, app[0] ^ KT_RC[round]);
}

}  // namespace

hipError_t keccak_table_trace(const uint64_t *d_inputs, uint64_t num_inputs, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                              hipStream_t stream) {
    const uint64_t n = 1ull << log_n;
    if (log_n == 0 || log_n > 24 || trace_stride < n || KECCAK_TABLE_ROUNDS * num_inputs > n || !d_trace || (num_inputs && !d_inputs))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + KECCAK_TABLE_THREADS - 1) / KECCAK_TABLE_THREADS);
    hipLaunchKernelGGL(keccak_table_trace_kernel, dim3(grid), dim3(KECCAK_TABLE_THREADS), 0, stream, d_inputs, num_inputs, n, d_trace, trace_stride);
    return hipGetLastError();
}

}  // namespace plonky2_hip

using namespace plonky2_hip;

extern "C" GlError gl_keccak_table_trace(const uint64_t *d_inputs, uint64_t num_inputs, uint32_t degree_bits, uint64_t *d_trace,
                                         uint64_t trace_stride, void *ctx) {
    DeviceCall device_call(ctx);
    if (!ctx || !d_trace || (num_inputs && !d_inputs)) return fail(GL_E_INVALID, "gl_keccak_table_trace: null pointer");
    if (degree_bits == 0 || degree_bits > 24) return fail(GL_E_INVALID, "gl_keccak_table_trace: degree_bits must be in 1 ..= 24");
    const uint64_t n = 1ull << degree_bits;
    if (num_inputs > n / KECCAK_TABLE_ROUNDS)
        return fail(GL_E_INVALID, "gl_keccak_table_trace: 24 * num_inputs exceeds the 2^degree_bits rows of the trace");
    if (trace_stride < n) return fail(GL_E_INVALID, "gl_keccak_table_trace: trace_stride smaller than 2^degree_bits: the columns would overlap");
    if (trace_stride > (1ull << 40)) return fail(GL_E_INVALID, "gl_keccak_table_trace: trace_stride too large");
    if (num_inputs) {
        const uintptr_t t0 = (uintptr_t)d_trace, t1 = t0 + ((uint64_t)(KECCAK_TABLE_COLUMNS - 1) * trace_stride + n) * 8;
        const uintptr_t i0 = (uintptr_t)d_inputs, i1 = i0 + num_inputs * 25 * 8;
        if (t0 < i1 && i0 < t1) return fail(GL_E_INVALID, "gl_keccak_table_trace: d_trace overlaps d_inputs");
    }
    HIP_TRY(keccak_table_trace(d_inputs, num_inputs, degree_bits, d_trace, trace_stride, S(ctx)->stream));
    return ok();
}
