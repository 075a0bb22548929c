// keccak_sponge_table.hip — the trace of the reference's Keccak sponge table (evm/src/keccak_sponge/keccak_sponge_stark.rs:190-347)
// built on the device from a list of byte strings: 414 columns, len / 136 + 1 consecutive rows per operation, zero rows behind
// them; and the records the sponge makes the Keccak-f, logic and memory tables take (witness/util.rs:178-250), from the trace.
//
// The number of rows depends on the data. As in memory_table.hip everything that decides it runs first: one thread per record
// checks its limits (the lowest record at fault per kind of fault with a vector atomicMin) and writes its row and byte counts,
// lookup.hip's scan turns both into exclusive prefix sums, the host reads 32 bytes — the call's one wait — and nothing has
// touched the trace by then. The fill has a serial and a parallel part:
//   - chain: one lane per OPERATION walks its blocks — absorb, keccak_f1600 (keccak_f1600.h, the state in registers as 50 halves),
//     next block — and writes, per row, the state before the block and behind the permutation: 100 columns. Lanes of a wave hold
//     consecutive operations, so with one-block operations every column store is one run of 512 bytes; a wave takes as long as
//     its longest operation, and one very long input runs on one lane (DESIGN.md §3.7.7 has what that costs);
//   - rows: one lane per ROW fills the other 314 columns, consecutive lanes hold consecutive rows, every column store of a wave
//     is one run of 512 bytes — logic_table.hip's layout, bound by its stores in the same way. The row finds its operation
//     through a row-to-operation map (a binary search per row in the prefix sums, once, in a kernel of its own), reads its 136
//     block bytes, applies pad10*1, reads original_rate_u32s back from the trace for xored_rate_u32s, and writes whole zero rows
//     behind the operations.
// The input bytes have no alignment: they are read as the aligned 32-bit words around them and joined by a funnel shift.
#include "keccak_sponge_table.h"

#include <algorithm>
#include <string>

#include "ctx.h"
#include "keccak_f1600.h"
#include "logic_table.h"
#include "lookup.h"
#include "memory_table.h"
#include "program_asm.h"
#include "table_args.h"

namespace plonky2_hip {

namespace {

constexpr uint32_t T = KECCAK_SPONGE_TABLE_THREADS;
constexpr uint32_t W = KECCAK_SPONGE_TABLE_OP_WORDS;
constexpr uint32_t RATE = KECCAK_SPONGE_RATE_BYTES;
constexpr uint64_t LOW32 = 0xFFFFFFFFull;

uint32_t blocks_for(uint64_t count) { return (uint32_t)((count + T - 1) / T); }

// one thread per record, and one more for the last element of the two scans
__global__ __launch_bounds__(T) void ks_counts(const uint64_t *__restrict__ ops, uint32_t num_ops, uint64_t *__restrict__ op_rows,
                                               uint64_t *__restrict__ op_bytes, KeccakSpongeTableHeader *header) {
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    if (i > num_ops) return;
    if (i == num_ops) {
        op_rows[i] = op_bytes[i] = 0;
        return;
    }
    const uint64_t *op = ops + (uint64_t)i * W;
    bool bad = false;
#pragma unroll
    for (uint32_t c = 0; c < W; ++c) bad |= op[c] > LOW32;
    const uint64_t virt = op[KS_OP_VIRT] & LOW32, len = op[KS_OP_LEN] & LOW32;
    if (bad) atomicMin(&header->bad_word, i);
    else if (virt + len > (1ull << 32)) atomicMin(&header->bad_span, i);
    op_rows[i] = len / RATE + 1;
    op_bytes[i] = len;
}

// behind the scans: the record with which the running sum of the lengths reaches 2^32, and the two totals
__global__ __launch_bounds__(T) void ks_decide(const uint64_t *__restrict__ ops, uint32_t num_ops, const uint64_t *__restrict__ op_rows,
                                               const uint64_t *__restrict__ op_bytes, KeccakSpongeTableHeader *header) {
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    if (i > num_ops) return;
    if (i == num_ops) {
        header->rows = op_rows[i];
        header->total_bytes = op_bytes[i];
        return;
    }
    if (op_bytes[i] + (ops[(uint64_t)i * W + KS_OP_LEN] & LOW32) > LOW32) atomicMin(&header->bad_sum, i);
}

// map[r]: the operation of row r < rows — the last one whose first row is at or before r
__global__ __launch_bounds__(T) void ks_map(const uint64_t *__restrict__ op_rows, uint32_t num_ops, uint64_t rows, uint32_t *__restrict__ map) {
    const uint64_t r = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (r >= rows) return;
    uint32_t lo = 0, hi = num_ops - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (op_rows[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    map[r] = lo;
}

// The 34 little-endian u32s of a block whose first `rem` bytes are input at p, one after the other. rem == 136: a full block;
// rem < 136: the final block with its pad10*1 padding, 0x01 behind the input and 0x80 in the last byte (0x81 where the two
// meet). p has no alignment: the bytes come as the ALIGNED 32-bit words around them (35 loads for 136 bytes, where byte loads
// are 136 and kept the rows kernel at 0.36 of the memset rate), joined by a funnel shift. Only words that hold an input byte are
// loaded: such a word lies inside whatever allocation holds that byte.
struct BlockWords {
    const uint32_t *base;
    uint32_t off, rem, cur, k;
    __device__ __forceinline__ BlockWords(const uint8_t *p, uint32_t rem_) : rem(rem_), k(0) {
        const uintptr_t a = (uintptr_t)p;
        base = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
        off = (uint32_t)(a & 3);
        cur = aligned(0);
    }
    // aligned word j holds the block's bytes 4 j - off .. 4 j - off + 3
    __device__ __forceinline__ uint32_t aligned(uint32_t j) const { return (4 * j > off ? 4 * j - off : 0u) < rem ? base[j] : 0u; }
    __device__ __forceinline__ uint32_t next() {
        const uint32_t nxt = aligned(k + 1);
        uint32_t word = __funnelshift_r(cur, nxt, 8 * off);
        cur = nxt;
        const uint32_t first = 4 * k;  // the block's bytes first .. first + 3
        if (rem < first + 4) {         // behind the input: only a final block gets here
            const uint32_t valid = rem > first ? rem - first : 0;
            word = valid ? word & ((1u << (8 * valid)) - 1) : 0u;
            if (rem >= first) word |= 0x01u << (8 * (rem - first));
            if (first + 4 == RATE) word |= 0x80000000u;
        }
        k++;
        return word;
    }
};

// One lane per operation: generate_rows_for_op's sponge_state through its blocks. State limb 2 j / 2 j + 1 is the low / high
// half of lane j (keccak_util.rs:6-18): limbs 0 .. 33 are the rate, 34 .. 49 the capacity.
__global__ __launch_bounds__(T) void keccak_sponge_chain_kernel(const uint64_t *__restrict__ ops, uint32_t num_ops, const uint64_t *__restrict__ op_rows,
                                                                const uint64_t *__restrict__ op_bytes, const uint8_t *__restrict__ bytes,
                                                                uint64_t *__restrict__ trace, uint64_t stride) {
    const uint32_t op = blockIdx.x * T + threadIdx.x;
    if (op >= num_ops) return;
    uint32_t left = (uint32_t)ops[(uint64_t)op * W + KS_OP_LEN];
    const uint8_t *p = bytes + op_bytes[op];
    uint64_t *out = trace + op_rows[op];
    KeccakState s;
#pragma unroll
    for (int k = 0; k < 25; k++) s.lo[k] = s.hi[k] = 0;
    for (;;) {
        const uint32_t rem = left < RATE ? left : RATE;
#pragma unroll
        for (int k = 0; k < 25; k++) {  // KS_ORIGINAL_CAPACITY_U32S follows KS_ORIGINAL_RATE_U32S
            out[(uint64_t)(KS_ORIGINAL_RATE_U32S + 2 * k) * stride] = s.lo[k];
            out[(uint64_t)(KS_ORIGINAL_RATE_U32S + 2 * k + 1) * stride] = s.hi[k];
        }
        BlockWords block(p, rem);
#pragma unroll
        for (int k = 0; k < 17; k++) {
            s.lo[k] ^= block.next();
            s.hi[k] ^= block.next();
        }
        keccak_f1600(s);
#pragma unroll
        for (int k = 0; k < 25; k++) {
            out[(uint64_t)(KS_UPDATED_STATE_U32S + 2 * k) * stride] = s.lo[k];
            out[(uint64_t)(KS_UPDATED_STATE_U32S + 2 * k + 1) * stride] = s.hi[k];
        }
        if (left < RATE) break;
        left -= RATE, p += RATE, out += 1;
    }
}
static_assert(KS_ORIGINAL_CAPACITY_U32S == KS_ORIGINAL_RATE_U32S + KECCAK_SPONGE_RATE_U32S, "the chain kernel stores the 50 limbs in one run");

// One lane per row: everything but the state columns the chain kernel wrote (original_rate_u32s is read back); behind `rows`
// the whole row is zero.
__global__ __launch_bounds__(T) void keccak_sponge_rows_kernel(const uint64_t *__restrict__ ops, const uint64_t *__restrict__ op_rows,
                                                               const uint64_t *__restrict__ op_bytes, const uint32_t *__restrict__ map,
                                                               const uint8_t *__restrict__ bytes, uint64_t rows, uint64_t n, uint64_t *trace,
                                                               uint64_t stride) {
    const uint64_t r = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (r >= n) return;
    uint64_t *out = trace + r;
    if (r >= rows) {
#pragma unroll 8
        for (uint32_t c = 0; c < KECCAK_SPONGE_TABLE_COLUMNS; c++) out[(uint64_t)c * stride] = 0;
        return;
    }
    const uint32_t op = map[r];
    const uint64_t *record = ops + (uint64_t)op * W;
    const uint32_t len = (uint32_t)record[KS_OP_LEN];
    const uint32_t absorbed = (uint32_t)(r - op_rows[op]) * RATE;  // at most len < 2^32
    const uint32_t left = len - absorbed;
    const bool last = left < RATE;
    const uint32_t rem = last ? left : RATE;
    out[(uint64_t)KS_IS_FULL_INPUT_BLOCK * stride] = last ? 0 : 1;
    out[(uint64_t)KS_IS_FINAL_BLOCK * stride] = last ? 1 : 0;
    out[(uint64_t)KS_CONTEXT * stride] = (uint32_t)record[KS_OP_CONTEXT];
    out[(uint64_t)KS_SEGMENT * stride] = (uint32_t)record[KS_OP_SEGMENT];
    out[(uint64_t)KS_VIRT * stride] = (uint32_t)record[KS_OP_VIRT];
    out[(uint64_t)KS_TIMESTAMP * stride] = (uint32_t)record[KS_OP_TIMESTAMP];
    out[(uint64_t)KS_LEN * stride] = len;
    out[(uint64_t)KS_ALREADY_ABSORBED_BYTES * stride] = absorbed;
#pragma unroll 8
    for (uint32_t i = 0; i < RATE; i++) out[(uint64_t)(KS_IS_FINAL_INPUT_LEN + i) * stride] = i == rem ? 1 : 0;  // rem == 136 on a full row
    BlockWords block(bytes + op_bytes[op] + absorbed, rem);
#pragma unroll 2
    for (uint32_t w = 0; w < KECCAK_SPONGE_RATE_U32S; w++) {
        const uint32_t word = block.next();
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) out[(uint64_t)(KS_BLOCK_BYTES + 4 * w + j) * stride] = (word >> (8 * j)) & 0xFF;
        const uint32_t original = (uint32_t)out[(uint64_t)(KS_ORIGINAL_RATE_U32S + w) * stride];
        out[(uint64_t)(KS_XORED_RATE_U32S + w) * stride] = original ^ word;
    }
}

// ---------------------------------------------------------------- the derived records
// counts[r]: the input bytes of row r — 136 on a full row, len - already_absorbed on a final one (cut to 135, which a trace of
// this file never exceeds), 0 on a padding row; counts[rows] = 0
__global__ __launch_bounds__(T) void ks_row_byte_counts(const uint64_t *__restrict__ trace, uint64_t stride, uint64_t rows, uint64_t *__restrict__ counts) {
    const uint64_t r = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (r > rows) return;
    uint64_t count = 0;
    if (r < rows) {
        if (trace[(uint64_t)KS_IS_FULL_INPUT_BLOCK * stride + r]) count = RATE;
        else if (trace[(uint64_t)KS_IS_FINAL_BLOCK * stride + r]) {
            count = trace[(uint64_t)KS_LEN * stride + r] - trace[(uint64_t)KS_ALREADY_ABSORBED_BYTES * stride + r];
            if (count > RATE - 1) count = RATE - 1;
        }
    }
    counts[r] = count;
}

// One lane per row: what push_keccak_bytes receives (the state behind the XOR, 25 lanes) and xor_into_sponge's five XORs
__global__ __launch_bounds__(T) void ks_derive_rows(const uint64_t *__restrict__ trace, uint64_t stride, uint64_t rows, uint64_t *__restrict__ keccak_inputs,
                                                    uint64_t *__restrict__ logic_ops) {
    const uint64_t r = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (r >= rows) return;
    const uint64_t *in = trace + r;
    if (keccak_inputs) {
        uint64_t *lanes = keccak_inputs + r * 25;
        for (uint32_t j = 0; j < 25; j++) {  // KS_ORIGINAL_CAPACITY_U32S does not follow KS_XORED_RATE_U32S
            const uint32_t c = j < 17 ? KS_XORED_RATE_U32S + 2 * j : KS_ORIGINAL_CAPACITY_U32S + 2 * (j - 17);
            lanes[j] = (in[(uint64_t)c * stride] & LOW32) | in[(uint64_t)(c + 1) * stride] << 32;
        }
    }
    if (logic_ops) {
        for (uint32_t i = 0; i < 5; i++) {
            uint64_t *record = logic_ops + (r * 5 + i) * LOGIC_TABLE_OP_WORDS;
            record[0] = LT_IS_XOR;
            for (uint32_t k = 0; k < 8; k++) {
                const uint32_t limb = 8 * i + k;
                uint64_t x = 0, y = 0;
                if (limb < KECCAK_SPONGE_RATE_U32S) {
                    x = in[(uint64_t)(KS_ORIGINAL_RATE_U32S + limb) * stride];
                    for (uint32_t j = 0; j < 4; j++) y |= (in[(uint64_t)(KS_BLOCK_BYTES + 4 * limb + j) * stride] & 0xFF) << (8 * j);
                }
                record[1 + k] = x & LOW32;
                record[1 + 8 + k] = y;
            }
        }
    }
}

// One thread per (row, byte of the block): the read of input byte i of the row, at the row's place in the list
__global__ __launch_bounds__(T) void ks_derive_memory(const uint64_t *__restrict__ trace, uint64_t stride, uint64_t rows, const uint64_t *__restrict__ sums,
                                                      uint64_t *__restrict__ memory_ops) {
    const uint64_t t = (uint64_t)blockIdx.x * T + threadIdx.x;
    const uint64_t r = t / RATE;
    const uint32_t i = (uint32_t)(t % RATE);
    if (r >= rows) return;
    const uint64_t first = sums[r];
    if (i >= sums[r + 1] - first) return;
    const uint64_t *in = trace + r;
    uint64_t *record = memory_ops + (first + i) * MEMORY_TABLE_OP_WORDS;
    record[MT_FILTER] = 1;
    record[MT_TIMESTAMP] = in[(uint64_t)KS_TIMESTAMP * stride];
    record[MT_IS_READ] = 1;
    record[MT_ADDR_CONTEXT] = in[(uint64_t)KS_CONTEXT * stride];
    record[MT_ADDR_SEGMENT] = in[(uint64_t)KS_SEGMENT * stride];
    record[MT_ADDR_VIRTUAL] = in[(uint64_t)KS_VIRT * stride] + in[(uint64_t)KS_ALREADY_ABSORBED_BYTES * stride] + i;
    record[MT_VALUE_START] = in[(uint64_t)(KS_BLOCK_BYTES + i) * stride];
#pragma unroll
    for (uint32_t c = 1; c < 8; c++) record[MT_VALUE_START + c] = 0;
}

hipError_t enqueue_count(const uint64_t *d_ops, uint64_t num_ops, const KeccakSpongeTableScratch &s, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.header, 0xFF, 16, stream);
    if (e != hipSuccess) return e;
    const uint32_t blocks = blocks_for(num_ops + 1);
    ks_counts<<<dim3(blocks), dim3(T), 0, stream>>>(d_ops, (uint32_t)num_ops, s.op_rows, s.op_bytes, s.header);
    e = lookup_exclusive_sums(s.op_rows, num_ops + 1, s.totals, stream);
    if (e != hipSuccess) return e;
    e = lookup_exclusive_sums(s.op_bytes, num_ops + 1, s.totals, stream);
    if (e != hipSuccess) return e;
    ks_decide<<<dim3(blocks), dim3(T), 0, stream>>>(d_ops, (uint32_t)num_ops, s.op_rows, s.op_bytes, s.header);
    return hipGetLastError();
}

hipError_t enqueue_map(uint64_t num_ops, uint64_t rows, const KeccakSpongeTableScratch &s, hipStream_t stream) {
    if (!rows) return hipSuccess;
    ks_map<<<dim3(blocks_for(rows)), dim3(T), 0, stream>>>(s.op_rows, (uint32_t)num_ops, rows, reinterpret_cast<uint32_t *>(s.row_words));
    return hipGetLastError();
}

hipError_t enqueue_chain(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint64_t *d_trace, uint64_t trace_stride,
                         const KeccakSpongeTableScratch &s, hipStream_t stream) {
    if (!num_ops) return hipSuccess;
    keccak_sponge_chain_kernel<<<dim3(blocks_for(num_ops)), dim3(T), 0, stream>>>(d_ops, (uint32_t)num_ops, s.op_rows, s.op_bytes, d_bytes, d_trace,
                                                                                  trace_stride);
    return hipGetLastError();
}

hipError_t enqueue_rows(const uint64_t *d_ops, const uint8_t *d_bytes, uint64_t rows, uint64_t n, uint64_t *d_trace, uint64_t trace_stride,
                        const KeccakSpongeTableScratch &s, hipStream_t stream) {
    keccak_sponge_rows_kernel<<<dim3(blocks_for(n)), dim3(T), 0, stream>>>(d_ops, s.op_rows, s.op_bytes, reinterpret_cast<const uint32_t *>(s.row_words),
                                                                           d_bytes, rows, n, d_trace, trace_stride);
    return hipGetLastError();
}

bool fill_arguments_ok(const uint64_t *d_ops, uint64_t num_ops, uint64_t rows, uint32_t log_n, const uint64_t *d_trace, uint64_t trace_stride) {
    if (log_n == 0 || log_n > KECCAK_SPONGE_TABLE_MAX_DEGREE_BITS || !d_trace || (num_ops && !d_ops)) return false;
    const uint64_t n = 1ull << log_n;
    return trace_stride >= n && rows <= n && rows >= num_ops && (num_ops || !rows);
}

}  // namespace

KeccakSpongeTableScratch keccak_sponge_table_scratch_layout(void *base, uint64_t num_ops, uint32_t log_n) {
    KeccakSpongeTableScratch s;
    const uint64_t n = 1ull << log_n;
    const uint64_t longest = (n > num_ops ? n : num_ops) + 1;
    uint64_t *words = static_cast<uint64_t *>(base);
    uint64_t at = sizeof(KeccakSpongeTableHeader) / 8;
    auto take = [&](uint64_t count) {
        uint64_t *p = words ? words + at : nullptr;
        at += count;
        return p;
    };
    s.header = reinterpret_cast<KeccakSpongeTableHeader *>(words);
    s.row_words = take(n + 1);
    s.totals = take((longest + LOOKUP_SCAN_BLOCK - 1) / LOOKUP_SCAN_BLOCK);
    s.op_rows = take(num_ops + 1);
    s.op_bytes = take(num_ops + 1);
    s.words = (at + 1) & ~1ull;  // a multiple of 16 bytes
    return s;
}

hipError_t keccak_sponge_table_count(const uint64_t *d_ops, uint64_t num_ops, const KeccakSpongeTableScratch &s, KeccakSpongeTableHeader *h,
                                     hipStream_t stream) {
    if (!d_ops || !h || num_ops == 0 || num_ops > KECCAK_SPONGE_TABLE_MAX_OPS) return hipErrorInvalidValue;
    hipError_t e = enqueue_count(d_ops, num_ops, s, stream);
    if (e != hipSuccess) return e;
    return read_status(h, s.header, sizeof(KeccakSpongeTableHeader), stream);
}

hipError_t keccak_sponge_table_fill(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint64_t rows, uint32_t log_n, uint64_t *d_trace,
                                    uint64_t trace_stride, const KeccakSpongeTableScratch &s, hipStream_t stream) {
    if (!fill_arguments_ok(d_ops, num_ops, rows, log_n, d_trace, trace_stride)) return hipErrorInvalidValue;
    hipError_t e = enqueue_map(num_ops, rows, s, stream);
    if (e != hipSuccess) return e;
    e = enqueue_chain(d_ops, num_ops, d_bytes, d_trace, trace_stride, s, stream);
    if (e != hipSuccess) return e;
    return enqueue_rows(d_ops, d_bytes, rows, 1ull << log_n, d_trace, trace_stride, s, stream);
}

hipError_t keccak_sponge_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint32_t log_n, uint64_t *d_trace,
                                        uint64_t trace_stride, const KeccakSpongeTableScratch &s, KeccakSpongeTableHeader *h, float *ms,
                                        hipStream_t stream) {
    if (!d_ops || !h || !ms || num_ops == 0 || num_ops > KECCAK_SPONGE_TABLE_MAX_OPS) return hipErrorInvalidValue;
    StageClock<6> clock(stream);
    hipError_t e = clock.created;
    const uint64_t n = 1ull << log_n;
    if (e == hipSuccess) e = clock.mark(0);
    if (e == hipSuccess) e = enqueue_count(d_ops, num_ops, s, stream);
    if (e == hipSuccess) e = clock.mark(1);
    if (e == hipSuccess) e = read_status(h, s.header, sizeof(KeccakSpongeTableHeader), stream);
    const bool fill = e == hipSuccess && h->bad_word == KS_NONE && h->bad_span == KS_NONE && h->bad_sum == KS_NONE && (d_bytes || !h->total_bytes) &&
                      fill_arguments_ok(d_ops, num_ops, h->rows, log_n, d_trace, trace_stride);
    if (e == hipSuccess) e = clock.mark(2);
    if (fill && e == hipSuccess) e = enqueue_map(num_ops, h->rows, s, stream);
    if (e == hipSuccess) e = clock.mark(3);
    if (fill && e == hipSuccess) e = enqueue_chain(d_ops, num_ops, d_bytes, d_trace, trace_stride, s, stream);
    if (e == hipSuccess) e = clock.mark(4);
    if (fill && e == hipSuccess) e = enqueue_rows(d_ops, d_bytes, h->rows, n, d_trace, trace_stride, s, stream);
    if (e == hipSuccess) e = clock.mark(5);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    const int from[4] = {0, 2, 3, 4};  // the wait for the header between the count and the map belongs to no stage
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = clock.elapsed(&ms[k], from[k], from[k] + 1);
    return e;
}

hipError_t keccak_sponge_table_derive(const uint64_t *d_trace, uint64_t trace_stride, uint64_t rows, uint64_t *d_keccak_inputs, uint64_t *d_logic_ops,
                                      uint64_t *d_memory_ops, const KeccakSpongeTableScratch &s, hipStream_t stream) {
    if (!d_trace || !rows) return rows ? hipErrorInvalidValue : hipSuccess;
    if (d_keccak_inputs || d_logic_ops) ks_derive_rows<<<dim3(blocks_for(rows)), dim3(T), 0, stream>>>(d_trace, trace_stride, rows, d_keccak_inputs, d_logic_ops);
    if (d_memory_ops) {
        ks_row_byte_counts<<<dim3(blocks_for(rows + 1)), dim3(T), 0, stream>>>(d_trace, trace_stride, rows, s.row_words);
        hipError_t e = lookup_exclusive_sums(s.row_words, rows + 1, s.totals, stream);
        if (e != hipSuccess) return e;
        ks_derive_memory<<<dim3(blocks_for(rows * RATE)), dim3(T), 0, stream>>>(d_trace, trace_stride, rows, s.row_words, d_memory_ops);
    }
    return hipGetLastError();
}

}  // namespace plonky2_hip

using namespace plonky2_hip;

static_assert(GL_KECCAK_SPONGE_TABLE_COLUMNS == KECCAK_SPONGE_TABLE_COLUMNS && GL_KECCAK_SPONGE_TABLE_OP_WORDS == KECCAK_SPONGE_TABLE_OP_WORDS, "plonky2_hip.h");

static bool ks_shape_ok(uint64_t num_ops, uint32_t degree_bits) {
    return num_ops <= KECCAK_SPONGE_TABLE_MAX_OPS && degree_bits >= 1 && degree_bits <= KECCAK_SPONGE_TABLE_MAX_DEGREE_BITS;
}

extern "C" uint64_t gl_keccak_sponge_table_scratch_bytes(uint64_t num_ops, uint32_t degree_bits) {
    if (!ks_shape_ok(num_ops, degree_bits)) return 0;
    return keccak_sponge_table_scratch_layout(nullptr, num_ops, degree_bits).words * 8;
}

// what is refused before anything is launched; empty: nothing
static std::string ks_trace_argument_error(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, const uint64_t *d_trace, uint64_t trace_stride,
                                           const void *d_scratch, const void *h_out, const void *ctx) {
    if (!ctx || (num_ops && !d_ops) || !d_scratch || !h_out) return "null pointer";
    if (num_ops > KECCAK_SPONGE_TABLE_MAX_OPS) return "num_ops must be at most 2^30";
    std::string why = degree_bits_error(degree_bits, KECCAK_SPONGE_TABLE_MAX_DEGREE_BITS);
    if (why.empty()) why = scratch_alignment_error(d_scratch);
    if (!why.empty()) return why;
    const uint64_t n = 1ull << degree_bits;
    const uint64_t scratch_bytes = keccak_sponge_table_scratch_layout(nullptr, num_ops, degree_bits).words * 8;
    const uint64_t ops_bytes = num_ops * KECCAK_SPONGE_TABLE_OP_WORDS * 8;
    if (bytes_overlap(d_ops, ops_bytes, d_scratch, scratch_bytes)) return "d_scratch overlaps d_ops";
    if (d_trace) {
        why = trace_stride_error(trace_stride, n);
        if (!why.empty()) return why;
        const uint64_t bytes = trace_bytes(KECCAK_SPONGE_TABLE_COLUMNS, trace_stride, n);
        if (bytes_overlap(d_trace, bytes, d_ops, ops_bytes)) return "d_trace overlaps d_ops";
        if (bytes_overlap(d_trace, bytes, d_scratch, scratch_bytes)) return "d_trace overlaps d_scratch";
    }
    return "";
}

// the refusals the device decided, read from the header: the lowest record at fault, whatever its fault; empty: nothing
static std::string ks_data_error(const KeccakSpongeTableHeader &h) {
    const uint32_t lowest = std::min(h.bad_word, std::min(h.bad_span, h.bad_sum));
    if (lowest == KS_NONE) return "";
    const std::string record = "record " + std::to_string(lowest);
    if (lowest == h.bad_word) return "a word of " + record + " is 2^32 or more";
    if (lowest == h.bad_span) return "virt + len of " + record + " exceeds 2^32";
    return "with " + record + " the sum of the lengths reaches 2^32";
}

extern "C" GlError gl_keccak_sponge_table_trace(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint32_t degree_bits, uint64_t *d_trace,
                                                uint64_t trace_stride, void *d_scratch, uint64_t *h_rows, void *ctx) {
    DeviceCall device_call(ctx);
    const std::string why = ks_trace_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, h_rows, ctx);
    if (!why.empty()) return fail(GL_E_INVALID, "gl_keccak_sponge_table_trace: " + why);
    const KeccakSpongeTableScratch scratch = keccak_sponge_table_scratch_layout(d_scratch, num_ops, degree_bits);
    const uint64_t n = 1ull << degree_bits;
    *h_rows = 0;
    KeccakSpongeTableHeader h = {KS_NONE, KS_NONE, KS_NONE, 0, 0, 0};
    if (num_ops) {
        HIP_TRY(keccak_sponge_table_count(d_ops, num_ops, scratch, &h, S(ctx)->stream));
        const std::string bad = ks_data_error(h);
        if (!bad.empty()) return fail(GL_E_INVALID, "gl_keccak_sponge_table_trace: " + bad);
        *h_rows = h.rows;
    }
    if (!d_trace) return ok();
    if (h.total_bytes && !d_bytes)
        return fail(GL_E_INVALID, "gl_keccak_sponge_table_trace: null pointer: d_bytes, and the operations hold " + std::to_string(h.total_bytes) + " bytes");
    if (h.rows > n)
        return fail(GL_E_INVALID, "gl_keccak_sponge_table_trace: the operations take " + std::to_string(h.rows) +
                                      " rows, more than the 2^degree_bits rows of the trace (the reference would cut an operation in the middle)");
    if (bytes_overlap(d_trace, trace_bytes(KECCAK_SPONGE_TABLE_COLUMNS, trace_stride, n), d_bytes, h.total_bytes))
        return fail(GL_E_INVALID, "gl_keccak_sponge_table_trace: d_trace overlaps d_bytes");
    HIP_TRY(keccak_sponge_table_fill(d_ops, num_ops, d_bytes, h.rows, degree_bits, d_trace, trace_stride, scratch, S(ctx)->stream));
    return ok();
}

extern "C" GlError gl_keccak_sponge_table_ops(const uint64_t *d_trace, uint64_t trace_stride, uint32_t degree_bits, uint64_t rows, uint64_t *d_keccak_inputs,
                                              uint64_t *d_logic_ops, uint64_t *d_memory_ops, void *d_scratch, void *ctx) {
    DeviceCall device_call(ctx);
    std::string why = !ctx || !d_trace || !d_scratch ? "null pointer" : degree_bits_error(degree_bits, KECCAK_SPONGE_TABLE_MAX_DEGREE_BITS);
    const uint64_t n = why.empty() ? 1ull << degree_bits : 0;
    if (why.empty() && rows > n) why = "rows exceeds the 2^degree_bits rows of the trace";
    if (why.empty()) why = trace_stride_error(trace_stride, n);
    if (why.empty()) why = scratch_alignment_error(d_scratch);
    if (why.empty()) {
        const uint64_t scratch_bytes = keccak_sponge_table_scratch_layout(nullptr, 0, degree_bits).words * 8;
        const uint64_t trace_bytes = plonky2_hip::trace_bytes(KECCAK_SPONGE_TABLE_COLUMNS, trace_stride, n);
        const uint64_t keccak_bytes = rows * 25 * 8, logic_bytes = rows * 5 * LOGIC_TABLE_OP_WORDS * 8;
        // the memory list's length is known on the device alone: its first record stands for it here
        const uint64_t memory_bytes = rows ? MEMORY_TABLE_OP_WORDS * 8 : 0;
        if (bytes_overlap(d_trace, trace_bytes, d_scratch, scratch_bytes)) why = "d_trace overlaps d_scratch";
        else if (bytes_overlap(d_keccak_inputs, keccak_bytes, d_trace, trace_bytes)) why = "d_keccak_inputs overlaps d_trace";
        else if (bytes_overlap(d_logic_ops, logic_bytes, d_trace, trace_bytes)) why = "d_logic_ops overlaps d_trace";
        else if (bytes_overlap(d_memory_ops, memory_bytes, d_trace, trace_bytes)) why = "d_memory_ops overlaps d_trace";
        else if (bytes_overlap(d_keccak_inputs, keccak_bytes, d_scratch, scratch_bytes)) why = "d_keccak_inputs overlaps d_scratch";
        else if (bytes_overlap(d_logic_ops, logic_bytes, d_scratch, scratch_bytes)) why = "d_logic_ops overlaps d_scratch";
        else if (bytes_overlap(d_memory_ops, memory_bytes, d_scratch, scratch_bytes)) why = "d_memory_ops overlaps d_scratch";
        else if (bytes_overlap(d_keccak_inputs, keccak_bytes, d_logic_ops, logic_bytes)) why = "d_keccak_inputs overlaps d_logic_ops";
    }
    if (!why.empty()) return fail(GL_E_INVALID, "gl_keccak_sponge_table_ops: " + why);
    HIP_TRY(keccak_sponge_table_derive(d_trace, trace_stride, rows, d_keccak_inputs, d_logic_ops, d_memory_ops,
                                       keccak_sponge_table_scratch_layout(d_scratch, 0, degree_bits), S(ctx)->stream));
    return ok();
}

extern "C" GlError gl_debug_keccak_sponge_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint32_t degree_bits,
                                                         uint64_t *d_trace, uint64_t trace_stride, void *d_scratch, float *h_ms, void *ctx) {
    DeviceCall device_call(ctx);
    std::string why = ks_trace_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, h_ms, ctx);
    if (why.empty() && (!d_trace || !num_ops)) why = "null pointer";
    if (!why.empty()) return fail(GL_E_INVALID, "gl_debug_keccak_sponge_table_stage_ms: " + why);
    KeccakSpongeTableHeader h;
    HIP_TRY(keccak_sponge_table_stage_ms(d_ops, num_ops, d_bytes, degree_bits, d_trace, trace_stride,
                                         keccak_sponge_table_scratch_layout(d_scratch, num_ops, degree_bits), &h, h_ms, S(ctx)->stream));
    std::string bad = ks_data_error(h);
    if (bad.empty() && (h.rows > (1ull << degree_bits) || (h.total_bytes && !d_bytes))) bad = "the rows do not fit the trace or d_bytes is missing";
    if (!bad.empty()) return fail(GL_E_INVALID, "gl_debug_keccak_sponge_table_stage_ms: nothing was filled: " + bad);
    return ok();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The constraints of the Keccak sponge table as ONE STARK program: plonky2_gpu_amd/keccak_sponge_table.py program(), call for call
// (tests/test_keccak_sponge_table_ref.py holds the two against each other word for word). The reference's eval_packed_generic for
// this table is a list of TODOs (evm/src/keccak_sponge/keccak_sponge_stark.rs:363-377); this is that list written out, in its
// order — the reference's to-do list, not a soundness claim: nothing here ties xored_rate_u32s to the block, for example, which
// is the logic lookup's job. "before_rate_bits" and "block_bits" name columns the layout does not have; nothing is emitted for them.
// Host code; the columns are keccak_sponge_table.h's (the 16 of original_capacity_u32s follow the 34 of original_rate_u32s).
namespace {

using namespace plonky2_hip::program_asm;

Program keccak_sponge_table_program(ImmediatePool &pool) {
    constexpr int RATE_BYTES = KECCAK_SPONGE_RATE_BYTES, WIDTH_U32S = KECCAK_SPONGE_WIDTH_U32S;
    StarkAsm a(&pool);
    auto boolean = [&](int column) {
        a.release();
        const int flag = a.local(column);
        const int one = a.imm(1);
        const int t = a.sub(flag, one);
        a.emit(a.mul(flag, t));
    };
    // each flag is boolean, and so is the implied dummy flag 1 - F - L: F L = 0
    boolean(KS_IS_FULL_INPUT_BLOCK);
    boolean(KS_IS_FINAL_BLOCK);
    {
        a.release();
        const int full = a.local(KS_IS_FULL_INPUT_BLOCK);
        const int fin = a.local(KS_IS_FINAL_BLOCK);
        a.emit(a.mul(full, fin));
    }
    // is_final_input_len contains booleans
    for (int i = 0; i < RATE_BYTES; i++) boolean(KS_IS_FINAL_INPUT_LEN + i);
    // their sum equals is_final_block
    {
        a.release();
        for (int i = 0; i < RATE_BYTES; i++) {
            const int t = a.local(KS_IS_FINAL_INPUT_LEN + i);
            a.acc(t, 1);
            a.free1(t);
        }
        const int sum = a.accr();
        const int fin = a.local(KS_IS_FINAL_BLOCK);
        a.emit(a.sub(sum, fin));
    }
    // the columns that are zero where a sponge starts: the original state, then already_absorbed_bytes
    int fresh[WIDTH_U32S + 1];
    for (int j = 0; j < WIDTH_U32S; j++) fresh[j] = KS_ORIGINAL_RATE_U32S + j;
    fresh[WIDTH_U32S] = KS_ALREADY_ABSORBED_BYTES;
    // the first row starts a sponge
    for (int column : fresh) {
        a.release();
        a.emit_first_row(a.local(column));
    }
    // behind a final block the next row starts one
    for (int column : fresh) {
        a.release();
        const int fin = a.local(KS_IS_FINAL_BLOCK);
        const int nxt = a.next(column);
        a.emit_transition(a.mul(fin, nxt));
    }
    // behind a full-input block the next row's address, time and len match
    for (int column : {KS_CONTEXT, KS_SEGMENT, KS_VIRT, KS_TIMESTAMP, KS_LEN}) {
        a.release();
        const int full = a.local(KS_IS_FULL_INPUT_BLOCK);
        const int nxt = a.next(column);
        const int local = a.local(column);
        const int diff = a.sub(nxt, local);
        a.emit_transition(a.mul(full, diff));
    }
    // ... its "before" is our "after"
    for (int j = 0; j < WIDTH_U32S; j++) {
        a.release();
        const int full = a.local(KS_IS_FULL_INPUT_BLOCK);
        const int nxt = a.next(KS_ORIGINAL_RATE_U32S + j);
        const int updated = a.local(KS_UPDATED_STATE_U32S + j);
        const int diff = a.sub(nxt, updated);
        a.emit_transition(a.mul(full, diff));
    }
    // ... and its already_absorbed_bytes is ours plus 136
    {
        a.release();
        const int full = a.local(KS_IS_FULL_INPUT_BLOCK);
        const int nxt = a.next(KS_ALREADY_ABSORBED_BYTES);
        const int local = a.local(KS_ALREADY_ABSORBED_BYTES);
        const int diff = a.sub(nxt, local);
        const int rate = a.imm(RATE_BYTES);
        a.sub(diff, rate, diff);
        a.emit_transition(a.mul(full, diff));
    }
    // a dummy row is followed by a dummy row
    {
        a.release();
        const int dummy = a.imm(1);
        const int full = a.local(KS_IS_FULL_INPUT_BLOCK);
        a.sub(dummy, full, dummy);
        const int fin = a.local(KS_IS_FINAL_BLOCK);
        a.sub(dummy, fin, dummy);
        const int next_full = a.next(KS_IS_FULL_INPUT_BLOCK);
        const int next_fin = a.next(KS_IS_FINAL_BLOCK);
        const int next_used = a.add(next_full, next_fin);
        a.emit_transition(a.mul(dummy, next_used));
    }
    // is_final_input_len[i] implies len - already_absorbed_bytes == i
    for (int i = 0; i < RATE_BYTES; i++) {
        a.release();
        const int flag = a.local(KS_IS_FINAL_INPUT_LEN + i);
        const int len = a.local(KS_LEN);
        const int absorbed = a.local(KS_ALREADY_ABSORBED_BYTES);
        const int diff = a.sub(len, absorbed);
        const int index = a.imm(i);
        a.sub(diff, index, diff);
        a.emit(a.mul(flag, diff));
    }
    return a.instrs;
}

}  // namespace

extern "C" GlError gl_keccak_sponge_table_program(GlGatePrograms *out) {
    return emit_table_program("gl_keccak_sponge_table_program", keccak_sponge_table_program, out);
}
