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
#include "program_asm.h"
#include "table_args.h"

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
    std::string why = degree_bits_error(degree_bits, 24);
    if (!why.empty()) return fail(GL_E_INVALID, "gl_keccak_table_trace: " + why);
    const uint64_t n = 1ull << degree_bits;
    if (num_inputs > n / KECCAK_TABLE_ROUNDS)
        return fail(GL_E_INVALID, "gl_keccak_table_trace: 24 * num_inputs exceeds the 2^degree_bits rows of the trace");
    why = trace_stride_error(trace_stride, n);
    if (!why.empty()) return fail(GL_E_INVALID, "gl_keccak_table_trace: " + why);
    if (bytes_overlap(d_trace, trace_bytes(KECCAK_TABLE_COLUMNS, trace_stride, n), d_inputs, num_inputs * 25 * 8))
        return fail(GL_E_INVALID, "gl_keccak_table_trace: d_trace overlaps d_inputs");
    HIP_TRY(keccak_table_trace(d_inputs, num_inputs, degree_bits, d_trace, trace_stride, S(ctx)->stream));
    return ok();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The constraints of the reference's Keccak-f table (evm/src/keccak/keccak_stark.rs:230-375 with round_flags.rs:12-27 and
// logic.rs) as ONE STARK program: plonky2_gpu_amd/keccak_table.py program(), call for call (tests/test_keccak_table_ref.py holds
// the two against each other word for word). Host code; the columns are keccak_table.h's.
namespace {

using namespace plonky2_hip::program_asm;

Program keccak_table_program(ImmediatePool &pool) {
    constexpr int NUM_ROUNDS = KECCAK_TABLE_ROUNDS;
    StarkAsm a(&pool);
    // eval_round_flags
    {
        const int s0 = a.local(kt_reg_step(0));
        const int one = a.imm(1);
        a.emit_first_row(a.sub(s0, one));
    }
    for (int i = 1; i < NUM_ROUNDS; i++) {
        a.release();
        a.emit_first_row(a.local(kt_reg_step(i)));
    }
    for (int i = 0; i < NUM_ROUNDS; i++) {
        a.release();
        const int nx = a.next(kt_reg_step((i + 1) % NUM_ROUNDS));
        const int lc = a.local(kt_reg_step(i));
        a.emit_transition(a.sub(nx, lc));
    }
    // C'[x, z] = xor(C[x, z], C[x - 1, z], C[x + 1, z - 1])
    for (int x = 0; x < 5; x++)
        for (int z = 0; z < 64; z++) {
            a.release();
            const int c0 = a.local(kt_reg_c(x, z));
            const int c1 = a.local(kt_reg_c((x + 4) % 5, z));
            const int c2 = a.local(kt_reg_c((x + 1) % 5, (z + 63) % 64));
            const int x3 = a.xor3(c0, c1, c2);
            const int cp = a.local(kt_reg_c_prime(x, z));
            a.emit(a.sub(cp, x3));
        }
    // A[x, y, z] = xor(A'[x, y, z], C[x, z], C'[x, z]), recomposed into the two input limbs
    for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++) {
            auto bit = [&](int z) {
                const int ap = a.local(kt_reg_a_prime(x, y, z));
                const int c = a.local(kt_reg_c(x, z));
                const int cp = a.local(kt_reg_c_prime(x, z));
                const int t = a.xor3(ap, c, cp);
                a.free({ap, c, cp});
                return t;
            };
            for (int l = 0; l < 2; l++) {
                a.release();
                const int computed = a.limb(bit, 32 * l);
                const int al = a.local(kt_reg_a(x, y) + l);
                a.emit(a.sub(computed, al));
            }
        }
    // diff (diff - 2) (diff - 4) = 0 with diff = sum_i A'[x, i, z] - C'[x, z]
    for (int x = 0; x < 5; x++)
        for (int z = 0; z < 64; z++) {
            a.release();
            const int s = a.local(kt_reg_a_prime(x, 0, z));
            for (int i = 1; i < 5; i++) {
                const int t = a.local(kt_reg_a_prime(x, i, z));
                a.add(s, t, s);
                a.free1(t);
            }
            const int cp = a.local(kt_reg_c_prime(x, z));
            const int diff = a.sub(s, cp);
            const int two = a.imm(2);
            const int d2 = a.sub(diff, two);
            const int four = a.imm(4);
            const int d4 = a.sub(diff, four);
            const int m = a.mul(diff, d2);
            a.emit(a.mul(m, d4));
        }
    // A''[x, y] = xor(B[x, y], andn(B[x + 1, y], B[x + 2, y]))
    for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++)
            for (int l = 0; l < 2; l++) {
                a.release();
                const int one = a.imm(1);
                auto bit = [&](int z) {
                    const int b0 = a.local(kt_reg_b(x, y, z));
                    const int b1 = a.local(kt_reg_b((x + 1) % 5, y, z));
                    const int b2 = a.local(kt_reg_b((x + 2) % 5, y, z));
                    const int n = a.sub(one, b1);
                    a.mul(n, b2, n);  // andn_gen(x, y) = (1 - x) y
                    const int t = a.xor2(b0, n);
                    a.free({b0, b1, b2, n});
                    return t;
                };
                const int computed = a.limb(bit, 32 * l);
                const int app = a.local(kt_reg_a_prime_prime(x, y) + l);
                a.emit(a.sub(computed, app));
            }
    // A'''[0, 0] = A''[0, 0] xor RC: the bits of A''[0, 0] recompose into its limbs ...
    for (int l = 0; l < 2; l++) {
        a.release();
        const int computed = a.limb([&](int z) { return a.local(kt_reg_a_prime_prime_0_0_bit(z)); }, 32 * l);
        const int app = a.local(kt_reg_a_prime_prime(0, 0) + l);
        a.emit(a.sub(computed, app));
    }
    // ... and xored with the round's constant into the limbs of A'''[0, 0]
    auto xored_bit = [&](int i) {
        const int b = a.local(kt_reg_a_prime_prime_0_0_bit(i));
        bool any = false;
        for (int r = 0; r < NUM_ROUNDS; r++)
            if ((KT_ROUND_CONSTANTS[r] >> i) & 1) {
                const int f = a.local(kt_reg_step(r));
                a.acc(f, 1, 1);
                a.free1(f);
                any = true;
            }
        if (!any) return b;
        const int rc = a.accr(1);
        const int t = a.xor2(b, rc);
        a.free({b, rc});
        return t;
    };
    for (int l = 0; l < 2; l++) {
        a.release();
        const int computed = a.limb(xored_bit, 32 * l);
        const int appp = a.local(kt_reg_a_prime_prime_prime(0, 0) + l);
        a.emit(a.sub(computed, appp));
    }
    // this round's output is the next round's input, except behind the last round
    for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++)
            for (int l = 0; l < 2; l++) {
                a.release();
                const int one = a.imm(1);
                const int last = a.local(kt_reg_step(NUM_ROUNDS - 1));
                const int not_last = a.sub(one, last);
                const int out = a.local(kt_reg_a_prime_prime_prime(x, y) + l);
                const int in = a.next(kt_reg_a(x, y) + l);
                const int diff = a.sub(out, in);
                a.emit_transition(a.mul(not_last, diff));
            }
    return a.instrs;
}

}  // namespace

extern "C" GlError gl_keccak_table_program(GlGatePrograms *out) { return emit_table_program("gl_keccak_table_program", keccak_table_program, out); }
