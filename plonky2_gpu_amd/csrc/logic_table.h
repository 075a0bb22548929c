// logic_table.h — internal interface of the logic table's trace generator (logic_table.hip): LogicStark::generate_trace_rows
// (evm/src/logic.rs:157-176, columns of logic.rs:28-52) from a compact operation list, written straight into HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

constexpr uint32_t LOGIC_TABLE_COLUMNS = 523;
constexpr uint32_t LOGIC_TABLE_OP_WORDS = 17;  // the operator, the eight limbs of input0, the eight limbs of input1
constexpr uint32_t LOGIC_TABLE_LIMBS = 8;
constexpr uint32_t LOGIC_TABLE_VAL_BITS = 32 * LOGIC_TABLE_LIMBS;  // the bit columns of one input
constexpr uint32_t LOGIC_TABLE_THREADS = 256;
constexpr uint32_t LOGIC_TABLE_MAX_DEGREE_BITS = 23;  // gl_stark_create: degree_bits + rate_bits <= 24, and degree 3 needs rate_bits >= 1

// logic.rs:34-41
enum : uint32_t {
    LT_IS_AND = 0,
    LT_IS_OR = 1,
    LT_IS_XOR = 2,
    LT_INPUT0 = 3,    // 256 bit columns, least significant first
    LT_INPUT1 = 259,  // 256 bit columns
    LT_RESULT = 515,  // eight 32-bit limbs
};

// What the validation kernel leaves in the caller's 16 bytes of scratch and the host reads once per call: the lowest record
// whose operator is not 0, 1 or 2 and the lowest record with a limb of 2^32 or more; LT_NONE: there is none.
constexpr uint32_t LT_NONE = 0xFFFFFFFFu;
struct LogicTableStatus {
    uint32_t bad_operator;
    uint32_t bad_limb;
    uint32_t unused[2];
};
static_assert(sizeof(LogicTableStatus) == 16, "GL_LOGIC_TABLE_SCRATCH_BYTES");

// One pass over d_ops [num_ops][17] on `stream`, then *h is read back and the stream awaited: the call's one host wait.
// num_ops >= 1.
hipError_t logic_table_validate(const uint64_t *d_ops, uint64_t num_ops, LogicTableStatus *d_status, LogicTableStatus *h, hipStream_t stream);

// After a logic_table_validate that found nothing (or with num_ops == 0): rows 0 .. num_ops are Operation::into_row of the
// records, rows num_ops .. 2^log_n are zero; every word of the 523 columns [pitch trace_stride >= n] is written. Enqueued on
// `stream`; returns without waiting. rows_per_thread 1: 8 bytes per lane and column store; 2: two adjacent rows per thread,
// 16 bytes per lane, which needs d_trace 16-byte aligned and an even trace_stride (hipErrorInvalidValue otherwise); 0: the
// product path, which is 1. The caller has checked 1 <= log_n <= 23, num_ops <= n and trace_stride >= n.
hipError_t logic_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                            uint32_t rows_per_thread, hipStream_t stream);

}  // namespace plonky2_hip
