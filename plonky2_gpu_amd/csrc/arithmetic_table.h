// arithmetic_table.h — internal interface of the arithmetic table's trace generator (arithmetic_table.hip): the cells that
// ArithmeticStark::generate (evm/src/arithmetic/arithmetic_stark.rs:20-66, columns of columns.rs:25-117) derives for one operation,
// for a whole list of operations, written straight into HBM as the table include/plonky2_hip.h defines.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

constexpr uint32_t ARITHMETIC_TABLE_COLUMNS = 92;
constexpr uint32_t ARITHMETIC_TABLE_OP_WORDS = 25;  // the operator, the eight 32-bit limbs of in0, in1, in2
constexpr uint32_t ARITHMETIC_TABLE_LIMBS = 16;     // 16-bit limbs of a 256-bit value
constexpr uint32_t ARITHMETIC_TABLE_THREADS = 256;
constexpr uint32_t ARITHMETIC_TABLE_FILL_THREADS = 64;  // one wave per workgroup: a lane's operation is long and its registers many
constexpr uint32_t ARITHMETIC_TABLE_MAX_DEGREE_BITS = 22;  // gl_stark_create: degree_bits + rate_bits <= 24, and degree 5 needs rate_bits >= 2
constexpr uint64_t ARITHMETIC_TABLE_MAX_OPS = 1ull << ARITHMETIC_TABLE_MAX_DEGREE_BITS;  // every operation takes a row

// columns.rs:25-59 and :103-108
enum : uint32_t {
    AT_IS_ADD = 0,
    AT_IS_MUL = 1,
    AT_IS_SUB = 2,
    AT_IS_DIV = 3,
    AT_IS_MOD = 4,
    AT_IS_ADDMOD = 5,
    AT_IS_SUBMOD = 6,
    AT_IS_MULMOD = 7,
    AT_IS_LT = 8,
    AT_IS_GT = 9,
    AT_IS_SHL = 10,
    AT_IS_SHR = 11,
    AT_NUM_FLAGS = 12,
    AT_GENERAL_INPUT_0 = 12,
    AT_GENERAL_INPUT_1 = 28,
    AT_GENERAL_INPUT_2 = 44,
    AT_GENERAL_INPUT_3 = 60,
    AT_AUX_INPUT_0_LO = 76,
    // the second row of a modular operation
    AT_MODULAR_QUO_INPUT_HI = 12,
    AT_MODULAR_AUX_INPUT = 28,  // 31 values
    AT_MODULAR_MOD_IS_ZERO = 59,
    AT_MODULAR_OUT_AUX_RED = 60,
};
static_assert(AT_AUX_INPUT_0_LO + ARITHMETIC_TABLE_LIMBS == ARITHMETIC_TABLE_COLUMNS, "columns.rs");

// operator `op` takes two rows: DIV, MOD, ADDMOD, SUBMOD, MULMOD
__host__ __device__ constexpr bool at_is_modular(uint32_t op) { return op >= AT_IS_DIV && op <= AT_IS_MULMOD; }

// What the counting pass leaves at the head of the caller's scratch and the host reads once per call: per kind of fault the lowest
// record that has it (AT_NONE: there is none) and the rows the operations take.
constexpr uint32_t AT_NONE = 0xFFFFFFFFu;
struct ArithmeticTableHeader {
    uint32_t bad_operator;  // the operator word is 10 or more
    uint32_t bad_limb;      // a limb is 2^32 or more
    uint32_t bad_zero;      // an input that must be zero is not: in2 of a one-row operator, in1 of DIV and MOD
    uint32_t unused;
    uint64_t rows;
    uint64_t unused2;
};
static_assert(sizeof(ArithmeticTableHeader) == 32, "the scratch layout");

struct ArithmeticTableScratch {
    ArithmeticTableHeader *header;
    uint64_t *totals;   // the block totals of the scan
    uint64_t *op_rows;  // num_ops + 1: rows per operation, then their exclusive prefix sums
    uint64_t words;
};
ArithmeticTableScratch arithmetic_table_scratch_layout(void *base, uint64_t num_ops);

// Validation, the per-operation row counts and their exclusive prefix sums, enqueued on `stream`; *h is read back and the stream
// awaited: the call's one host wait. num_ops >= 1.
hipError_t arithmetic_table_count(const uint64_t *d_ops, uint64_t num_ops, const ArithmeticTableScratch &s, ArithmeticTableHeader *h, hipStream_t stream);
// After an arithmetic_table_count that found nothing and rows <= 2^log_n (or with num_ops == 0 and rows == 0): one lane per
// operation writes its one or two rows, one lane per row behind `rows` a zero row. Every word of the 92 columns [pitch
// trace_stride >= n] is written. Enqueued on `stream`; returns without waiting.
hipError_t arithmetic_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint64_t rows, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                 const ArithmeticTableScratch &s, hipStream_t stream);
// Measurement: count and fill with an event between the stages; ms[2]: the counting pass, the fill (both kernels). Creates and
// destroys its events and waits for the stream at the end. The fill runs only where the count found nothing and the rows fit.
hipError_t arithmetic_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                     const ArithmeticTableScratch &s, ArithmeticTableHeader *h, float *ms, hipStream_t stream);

}  // namespace plonky2_hip
