// poseidon_table.h — internal interface of the Poseidon table's trace generator (poseidon_table.hip): the permutation unit of the
// reference's system_zero crate (generate_permutation_unit, system_zero/src/permutation_unit.rs:56-105, columns of
// system_zero/src/registers/permutation.rs with START_PERMUTATION = 0) from a compact record list, written straight into HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

constexpr uint32_t POSEIDON_TABLE_WIDTH = 12;
constexpr uint32_t POSEIDON_TABLE_HALF_FULL = 4;
constexpr uint32_t POSEIDON_TABLE_PARTIAL = 22;
constexpr uint32_t POSEIDON_TABLE_COLUMNS = 249;
constexpr uint32_t POSEIDON_TABLE_OP_WORDS = 13;  // the kind, twelve element words
constexpr uint32_t POSEIDON_TABLE_MAX_ABSORB = 8;  // SPONGE_RATE: an ABSORB overwrites at most the rate
constexpr uint32_t POSEIDON_TABLE_THREADS = 256;
constexpr uint32_t POSEIDON_TABLE_MAX_DEGREE_BITS = 23;  // gl_stark_create: degree_bits + rate_bits <= 24, and degree 3 needs rate_bits >= 1

// registers/permutation.rs:6-57; PT_IS_REAL is this project's (the reference's unit has no filter: nothing looks into it yet)
enum : uint32_t {
    PT_INPUT = 0,
    PT_FULL_FIRST = 12,    // round r: mid_sbox at PT_FULL_FIRST + 24 r + i, after_mds at PT_FULL_FIRST + 24 r + 12 + i
    PT_PARTIAL = 108,      // round r: mid_sbox at PT_PARTIAL + 2 r, after_sbox at PT_PARTIAL + 2 r + 1
    PT_FULL_SECOND = 152,  // as PT_FULL_FIRST
    PT_OUTPUT = 236,       // the second full rounds' last after_mds
    PT_IS_REAL = 248,
};
static_assert(PT_PARTIAL == PT_FULL_FIRST + 2 * POSEIDON_TABLE_HALF_FULL * POSEIDON_TABLE_WIDTH && PT_FULL_SECOND == PT_PARTIAL + 2 * POSEIDON_TABLE_PARTIAL &&
                  PT_OUTPUT == PT_FULL_SECOND + (2 * POSEIDON_TABLE_HALF_FULL - 1) * POSEIDON_TABLE_WIDTH && PT_IS_REAL == PT_OUTPUT + POSEIDON_TABLE_WIDTH &&
                  POSEIDON_TABLE_COLUMNS == PT_IS_REAL + 1,
              "registers/permutation.rs");

// What the validation kernel leaves in the caller's 16 bytes of scratch and the host reads once per call: the lowest record whose
// kind is above 8, record 0 where it is an ABSORB (PT_NONE: there is none), and the number of ABSORB records.
constexpr uint32_t PT_NONE = 0xFFFFFFFFu;
struct PoseidonTableStatus {
    uint32_t bad_kind;
    uint32_t leading_absorb;
    uint32_t absorbs;
    uint32_t unused;
};
static_assert(sizeof(PoseidonTableStatus) == 16, "GL_POSEIDON_TABLE_SCRATCH_BYTES");

// the MDS layer of the rows kernel: on the matrix cores (poseidon.h) or on the vector ALU (poseidon_vector.h)
enum PoseidonTableMds : uint32_t { PT_MDS_PRODUCT = 0, PT_MDS_MATRIX_CORES = 1, PT_MDS_VECTOR = 2 };

// One pass over d_ops [num_ops][13] on `stream`, then *h is read back and the stream awaited: the call's one host wait.
// num_ops >= 1.
hipError_t poseidon_table_validate(const uint64_t *d_ops, uint64_t num_ops, PoseidonTableStatus *d_status, PoseidonTableStatus *h, hipStream_t stream);

// After a poseidon_table_validate that found nothing (or with num_ops == 0). `absorbs` is its count: non-zero enqueues the serial
// pass, which writes the twelve INPUT words of every ABSORB row; then the rows kernel writes every word of the 249 columns
// [pitch trace_stride >= n] on all n = 2^log_n rows. Enqueued on `stream`; returns without waiting. The caller has checked
// 1 <= log_n <= 23, num_ops <= n and trace_stride >= n.
hipError_t poseidon_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t absorbs, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                               PoseidonTableMds mds, hipStream_t stream);

// validate + fill with an event between the stages: ms[0] the validation, ms[1] the serial pass (negative: it did not run),
// ms[2] the rows. Nothing is filled where *h names a fault. Waits for the stream.
hipError_t poseidon_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                   PoseidonTableStatus *d_status, PoseidonTableStatus *h, PoseidonTableMds mds, float *ms, hipStream_t stream);

// The host's copy of poseidon_constants.h (gate_emit.hip holds it for the Poseidon gate's program): poseidon_table.hip sees the
// tables as device constants, which host code cannot read, and builds the table's program from these.
struct PoseidonHostConstants {
    const uint64_t *all_round_constants;  // [30][12]
    const uint64_t *mds_circ, *mds_diag;  // [12] each
};
PoseidonHostConstants poseidon_host_constants();

}  // namespace plonky2_hip
