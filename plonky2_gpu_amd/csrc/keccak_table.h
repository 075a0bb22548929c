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

// generate_trace_rows(inputs, min_rows) with n = 2^log_n rows: rows 24 k .. 24 k + 23 are permutation k of d_inputs [num_inputs][25]
// (input[5 y + x]), the rows behind them the permutation of the zero state, cut at n. Every word of the 2430 columns
// [pitch trace_stride >= n] is written; enqueued on `stream`, nothing is allocated, the host never waits. The caller has checked
// 24 num_inputs <= n, 1 <= log_n <= 24 and trace_stride >= n.
hipError_t keccak_table_trace(const uint64_t *d_inputs, uint64_t num_inputs, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                              hipStream_t stream);

}  // namespace plonky2_hip
