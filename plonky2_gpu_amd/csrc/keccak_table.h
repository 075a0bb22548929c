// keccak_table.h — internal interface of the Keccak-f table's trace generator (keccak_table.hip): the rows of the reference's
// KeccakStark (evm/src/keccak/keccak_stark.rs:53-204, columns of evm/src/keccak/columns.rs) written straight into HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

constexpr uint32_t KECCAK_TABLE_COLUMNS = 2430;
constexpr uint32_t KECCAK_TABLE_ROUNDS = 24;
constexpr uint32_t KECCAK_TABLE_THREADS = 256;  // one thread per row: four waves

// Column offsets of columns.rs (reg_step(i) = i)
constexpr uint32_t KT_A = 24;            // reg_a(x, y) = KT_A + (5 x + y) 2, low limb first
constexpr uint32_t KT_C = 74;            // reg_c(x, z) = KT_C + 64 x + z
constexpr uint32_t KT_C_PRIME = 394;     // reg_c_prime(x, z)
constexpr uint32_t KT_A_PRIME = 714;     // reg_a_prime(x, y, z) = KT_A_PRIME + 64 (5 x + y) + z
constexpr uint32_t KT_A_PRIME2 = 2314;   // reg_a_prime_prime(x, y) = KT_A_PRIME2 + (5 x + y) 2
constexpr uint32_t KT_A_PRIME2_BITS = 2364;  // reg_a_prime_prime_0_0_bit(i)
constexpr uint32_t KT_A_PRIME3_00 = 2428;    // the two limbs of A'''[0, 0]

// The host's statement of Keccak-f's round constants and rotations, for the program emitter (keccak_table.hip, program()). The
// trace kernel reads copies of its own (__constant__ KT_RC and kt_rot, which no constant expression can read, so no static_assert
// ties them): tests/test_gpu_keccak_table.py::test_trace_equals_generate_trace_rows holds the kernel's against the reference's
// rows, and test_keccak_table_ref.py holds this program word for word against keccak_table.py's, which states them once more.
constexpr uint64_t KT_ROUND_CONSTANTS[KECCAK_TABLE_ROUNDS] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
constexpr int KT_ROTATIONS[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};

// columns.rs's reg_* functions on the offsets above, as the program emitter names its columns
constexpr int kt_reg_step(int i) { return i; }
constexpr int kt_reg_a(int x, int y) { return (int)KT_A + (x * 5 + y) * 2; }
constexpr int kt_reg_c(int x, int z) { return (int)KT_C + x * 64 + z; }
constexpr int kt_reg_c_prime(int x, int z) { return (int)KT_C_PRIME + x * 64 + z; }
constexpr int kt_reg_a_prime(int x, int y, int z) { return (int)KT_A_PRIME + x * 64 * 5 + y * 64 + z; }
constexpr int kt_reg_b(int x, int y, int z) { return kt_reg_a_prime((x + 3 * y) % 5, x, (z + 64 - KT_ROTATIONS[(x + 3 * y) % 5][x]) % 64); }
constexpr int kt_reg_a_prime_prime(int x, int y) { return (int)KT_A_PRIME2 + x * 2 * 5 + y * 2; }
constexpr int kt_reg_a_prime_prime_0_0_bit(int i) { return (int)KT_A_PRIME2_BITS + i; }
constexpr int kt_reg_a_prime_prime_prime(int x, int y) { return x == 0 && y == 0 ? (int)KT_A_PRIME3_00 : kt_reg_a_prime_prime(x, y); }

// generate_trace_rows(inputs, min_rows) with n = 2^log_n rows: rows 24 k .. 24 k + 23 are permutation k of d_inputs [num_inputs][25]
// (input[5 y + x]), the rows behind them the permutation of the zero state, cut at n. Every word of the 2430 columns
// [pitch trace_stride >= n] is written; enqueued on `stream`, nothing is allocated, the host never waits. The caller has checked
// 24 num_inputs <= n, 1 <= log_n <= 24 and trace_stride >= n.
hipError_t keccak_table_trace(const uint64_t *d_inputs, uint64_t num_inputs, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                              hipStream_t stream);

}  // namespace plonky2_hip
