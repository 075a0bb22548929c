// lookup.h — internal interface of the lookup kernels (lookup.hip): a keys-only radix sort of canonical field elements and the
// permuted columns of the Halo2-style lookup argument (permuted_cols, evm/src/lookup.rs:67-131) without its serial merge.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plonky2_hip {

constexpr uint32_t LOOKUP_THREADS = 256;      // every kernel of lookup.hip: four waves
constexpr uint32_t LOOKUP_SORT_TILE = 2048;   // keys per workgroup of a radix pass: 8 rounds of 64 keys per wave
constexpr uint32_t LOOKUP_SCAN_BLOCK = 2048;  // elements per workgroup of a prefix scan: 8 per thread
constexpr uint64_t LOOKUP_MAX_N = 1ull << 30;
constexpr uint32_t LOOKUP_HEADER_WORDS = 1088;  // counters, the pass plan and the 8 x 256 digit histogram of the sort in flight

// The caller's scratch buffer cut into its parts (all of them functions of n alone). `words` is its size in 64-bit words.
struct LookupScratch {
    uint32_t *header;     // [0] first post-loop input, [1] number of deferred pops, [16..25) pass plan, [64..64+2048) digit histogram
    uint64_t *table;      // n: the sorted table
    uint64_t *tmp;        // 2 n: the other buffer of the sorts; the (sum, min) scan of the events between them
    uint64_t *keys;       // 2 n: level << 32 | event
    uint64_t *ranks;      // n + 1: exclusive scan of the flags, pops in the low and pushes in the high 32 bits
    uint32_t *events;     // 2 n: the index into the sorted inputs (bit 31 set: a pop) or into the sorted table (a push)
    uint64_t *stack;      // n: the table values no pop took, bottom to top
    uint32_t *deferred;   // n: the positions of the pops on an empty stack, in event order
    uint32_t *tile_hist;  // 256 x tiles of 2 n keys
    uint64_t *totals;     // the block totals of the longest scan
    uint64_t words;
};
LookupScratch lookup_scratch_layout(void *base, uint64_t n);

// Canonical values of in[0..n) ascending -> out (out == in allowed). Everything is enqueued on `stream`; nothing is allocated and
// the host never waits. 1 <= n <= 2^31 keys (the level sort of permuted_cols has 2 n of them).
hipError_t lookup_sort_canonical(const uint64_t *in, uint64_t *out, uint64_t n, const LookupScratch &s, hipStream_t stream);

// permuted_cols(inputs, table) -> (permuted_inputs, permuted_table), bit for bit. 1 <= n <= 2^30; the outputs overlap nothing.
hipError_t lookup_permuted_cols(const uint64_t *inputs, const uint64_t *table, uint64_t n, uint64_t *permuted_inputs, uint64_t *permuted_table,
                                const LookupScratch &s, hipStream_t stream);

// The two pieces the memory table's trace generator (memory_table.hip) shares with permuted_cols. Both are enqueued on `stream`.
// keys[0..n) sorted in place by their upper 32 bits alone, stably (the radix passes of digits 4 .. 7, uniform digits skipped):
// with a position in the lower 32 bits this is one round of a multi-field sort. 1 <= n <= 2^31, `s` laid out for at least n / 2.
hipError_t lookup_sort_by_upper_half(uint64_t *keys, uint64_t n, const LookupScratch &s, hipStream_t stream);
// data[0..len) becomes its exclusive prefix sums; `totals` holds ceil(len / LOOKUP_SCAN_BLOCK) words.
hipError_t lookup_exclusive_sums(uint64_t *data, uint64_t len, void *totals, hipStream_t stream);

}  // namespace plonky2_hip
