// memory_table.h — internal interface of the memory table's trace generator (memory_table.hip): MemoryStark::generate_trace
// (evm/src/memory/memory_stark.rs:122-236) from the unsorted operation list, in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lookup.h"

namespace plonky2_hip {

constexpr uint32_t MEMORY_TABLE_COLUMNS = 26;
constexpr uint32_t MEMORY_TABLE_OP_WORDS = 14;  // MemoryOp::into_row()[0..14]
constexpr uint32_t MEMORY_TABLE_THREADS = 256;
constexpr uint64_t MEMORY_TABLE_MAX_OPS = LOOKUP_MAX_N;
constexpr uint32_t MEMORY_TABLE_MAX_DEGREE_BITS = 23;  // gl_stark_create: degree_bits + rate_bits <= 24, and degree 3 needs rate_bits >= 1

// columns.rs
enum : uint32_t {
    MT_FILTER = 0,
    MT_TIMESTAMP = 1,
    MT_IS_READ = 2,
    MT_ADDR_CONTEXT = 3,
    MT_ADDR_SEGMENT = 4,
    MT_ADDR_VIRTUAL = 5,
    MT_VALUE_START = 6,
    MT_CONTEXT_FIRST_CHANGE = 14,
    MT_SEGMENT_FIRST_CHANGE = 15,
    MT_VIRTUAL_FIRST_CHANGE = 16,
    MT_RANGE_CHECK = 22,
    MT_COUNTER = 23,
    MT_RANGE_CHECK_PERMUTED = 24,
    MT_COUNTER_PERMUTED = 25,
};

// what the device decides before anything is written to the trace; the host reads it once per call
enum : uint32_t {
    MT_BAD_FLAG = 1,  // FILTER or IS_READ of an operation is neither 0 nor 1
    MT_BAD_WORD = 2,  // another word of an operation is 2^32 or more
    MT_BAD_GAP = 4,   // a context or segment gap whose range check would be >= n
    MT_BAD_ROWS = 8,  // operations + dummies > n
};
struct MemoryTableHeader {
    uint32_t status;
    uint32_t last_pair;  // 1 + the last pair of sorted operations that has dummies between them; 0: there are no dummies
    uint64_t rows;       // operations + dummies
};

// The caller's scratch: the lookup kernels' layout for max(n, num_ops) (the sorts, the scan and permuted_cols run in it, and
// the sorted keys and the dummies' prefix sums live in parts permuted_cols uses only afterwards), then the header.
struct MemoryTableScratch {
    LookupScratch sort;    // laid out for max(n, num_ops)
    LookupScratch lookup;  // laid out for n, from the same base
    MemoryTableHeader *header;
    uint64_t words;
};
MemoryTableScratch memory_table_scratch_layout(void *base, uint64_t num_ops, uint32_t log_n);

// Sort, gaps, their scan and the decision, enqueued on `stream`; *h is read back and the stream awaited: the call's one host
// wait. n = 0 asks for the count alone (no check against a trace's height).
hipError_t memory_table_count(const uint64_t *d_ops, uint64_t num_ops, uint64_t n, const MemoryTableScratch &s, MemoryTableHeader *h,
                              hipStream_t stream);
// After a memory_table_count that left status 0: the 26 columns, enqueued on `stream`; returns without waiting.
hipError_t memory_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                             const MemoryTableScratch &s, hipStream_t stream);

// Measurement: the whole call with an event between its stages; ms[5]: sort, gaps, rows, flags, lookup columns. Creates and
// destroys its events and waits for the stream at the end.
hipError_t memory_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                 const MemoryTableScratch &s, MemoryTableHeader *h, float *ms, hipStream_t stream);

}  // namespace plonky2_hip
