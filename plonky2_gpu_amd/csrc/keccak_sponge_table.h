// keccak_sponge_table.h — internal interface of the Keccak sponge table's trace generator (keccak_sponge_table.hip):
// KeccakSpongeStark::generate_trace_rows (evm/src/keccak_sponge/keccak_sponge_stark.rs:190-347, columns of columns.rs:15-60) from a
// list of (address, timestamp, length) records and the concatenated input bytes, written straight into HBM, and the records the
// sponge makes the Keccak-f, logic and memory tables take (witness/util.rs:178-250), derived from the finished trace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

constexpr uint32_t KECCAK_SPONGE_TABLE_COLUMNS = 414;
constexpr uint32_t KECCAK_SPONGE_TABLE_OP_WORDS = 5;  // context, segment, virt, timestamp, len
constexpr uint32_t KECCAK_SPONGE_TABLE_THREADS = 256;
constexpr uint32_t KECCAK_SPONGE_TABLE_MAX_DEGREE_BITS = 23;  // gl_stark_create: degree_bits + rate_bits <= 24, and degree 3 needs rate_bits >= 1
constexpr uint64_t KECCAK_SPONGE_TABLE_MAX_OPS = 1ull << 30;
constexpr uint32_t KECCAK_SPONGE_RATE_BYTES = 136;
constexpr uint32_t KECCAK_SPONGE_RATE_U32S = 34;
constexpr uint32_t KECCAK_SPONGE_CAPACITY_U32S = 16;
constexpr uint32_t KECCAK_SPONGE_WIDTH_U32S = 50;

// a record's words
enum : uint32_t { KS_OP_CONTEXT = 0, KS_OP_SEGMENT = 1, KS_OP_VIRT = 2, KS_OP_TIMESTAMP = 3, KS_OP_LEN = 4 };

// columns.rs:15-60
enum : uint32_t {
    KS_IS_FULL_INPUT_BLOCK = 0,
    KS_IS_FINAL_BLOCK = 1,
    KS_CONTEXT = 2,
    KS_SEGMENT = 3,
    KS_VIRT = 4,
    KS_TIMESTAMP = 5,
    KS_LEN = 6,
    KS_ALREADY_ABSORBED_BYTES = 7,
    KS_IS_FINAL_INPUT_LEN = 8,        // 136
    KS_ORIGINAL_RATE_U32S = 144,      // 34
    KS_ORIGINAL_CAPACITY_U32S = 178,  // 16
    KS_BLOCK_BYTES = 194,             // 136
    KS_XORED_RATE_U32S = 330,         // 34
    KS_UPDATED_STATE_U32S = 364,      // 50
};
static_assert(KS_UPDATED_STATE_U32S + KECCAK_SPONGE_WIDTH_U32S == KECCAK_SPONGE_TABLE_COLUMNS, "columns.rs");

// What the counting pass leaves at the head of the caller's scratch and the host reads once per call: per kind of fault the lowest
// record that has it (KS_NONE: there is none), the rows the operations take and the bytes they hold.
constexpr uint32_t KS_NONE = 0xFFFFFFFFu;
struct KeccakSpongeTableHeader {
    uint32_t bad_word;  // a word of the record is 2^32 or more
    uint32_t bad_span;  // virt + len > 2^32
    uint32_t bad_sum;   // with this record the sum of the lengths reaches 2^32
    uint32_t unused;
    uint64_t rows;
    uint64_t total_bytes;
};
static_assert(sizeof(KeccakSpongeTableHeader) == 32, "the scratch layout");

// The caller's scratch cut into its parts. `row_words` comes first and depends on log_n alone, so that a scratch sized for any
// num_ops serves gl_keccak_sponge_table_ops at the same degree_bits.
struct KeccakSpongeTableScratch {
    KeccakSpongeTableHeader *header;
    uint64_t *row_words;  // n + 1: the row-to-operation map (n uint32_t) of the trace call; the rows' byte counts and their sums of the ops call
    uint64_t *totals;     // the block totals of the longest scan
    uint64_t *op_rows;    // num_ops + 1: rows per operation, then their exclusive prefix sums
    uint64_t *op_bytes;   // num_ops + 1: bytes per operation, then their exclusive prefix sums
    uint64_t words;
};
KeccakSpongeTableScratch keccak_sponge_table_scratch_layout(void *base, uint64_t num_ops, uint32_t log_n);

// Validation, the per-operation row and byte counts and their exclusive prefix sums, enqueued on `stream`; *h is read back and the
// stream awaited: the call's one host wait. num_ops >= 1.
hipError_t keccak_sponge_table_count(const uint64_t *d_ops, uint64_t num_ops, const KeccakSpongeTableScratch &s, KeccakSpongeTableHeader *h,
                                     hipStream_t stream);
// After a keccak_sponge_table_count that found nothing and rows <= 2^log_n (or with num_ops == 0 and rows == 0): the map, the chain
// kernel (one lane per operation: the 100 state columns of its rows) and the rows kernel (one lane per row: the other 314 columns,
// whole zero rows behind `rows`). Every word of the 414 columns [pitch trace_stride >= n] is written. Enqueued on `stream`; returns
// without waiting.
hipError_t keccak_sponge_table_fill(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint64_t rows, uint32_t log_n, uint64_t *d_trace,
                                    uint64_t trace_stride, const KeccakSpongeTableScratch &s, hipStream_t stream);
// Measurement: count and fill with an event between the stages; ms[4]: counting pass, map, chain kernel, rows kernel. Creates and
// destroys its events and waits for the stream at the end. The fill runs only where the count found nothing.
hipError_t keccak_sponge_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint32_t log_n, uint64_t *d_trace,
                                        uint64_t trace_stride, const KeccakSpongeTableScratch &s, KeccakSpongeTableHeader *h, float *ms,
                                        hipStream_t stream);
// From rows 0 .. rows of a finished trace: the Keccak-f inputs [rows][25], the logic records [5 rows][17] and the memory reads
// [sum of len][14]; any output may be null. Enqueued on `stream`; no host wait. `s` laid out for log_n (any num_ops).
hipError_t keccak_sponge_table_derive(const uint64_t *d_trace, uint64_t trace_stride, uint64_t rows, uint64_t *d_keccak_inputs, uint64_t *d_logic_ops,
                                      uint64_t *d_memory_ops, const KeccakSpongeTableScratch &s, hipStream_t stream);

}  // namespace plonky2_hip
