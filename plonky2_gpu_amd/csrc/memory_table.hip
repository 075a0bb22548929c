// memory_table.hip — the trace of the reference's memory table (evm/src/memory/memory_stark.rs:122-236) built on the device from
// the UNSORTED operation list: 26 columns, one row per operation, dummy read or padding row.
//
// The reference sorts the operations by (context, segment, virtual address, timestamp), appends the dummy reads of fill_gaps and
// the padding rows of pad_memory_ops to the END of the vector and sorts again. One sort is enough:
//   - every dummy of the pair (curr, next) of sorted operations has a key strictly between the two, and the dummies of a pair
//     are pushed in ascending key order: they sit between curr and next, and their number is a function of the pair alone —
//     floor((dvirt - 1) / (max_rc + 1)) where the virtual address changes, (dts - 1) / max_rc where only the timestamp does,
//     0 where context or segment change (fill_gaps never looks at those gaps). Row of sorted operation j = j + the exclusive
//     prefix sum of the counts;
//   - the padding rows repeat the LAST ELEMENT OF THE VECTOR after fill_gaps — the last dummy pushed, else the largest
//     operation — as reads with filter 0: equal keys, pushed later, so the second stable sort puts them directly behind it.
// The sort is four rounds of lookup.hip's stable radix sort over `field << 32 | position`, timestamp first, context last, with
// a gather of the next field between the rounds: the record (14 words) stays where it is and only 8 bytes per operation move;
// segments and contexts are small numbers, so most of their radix passes are skipped on the device.
// Then one thread per ROW of the trace: a binary search in the prefix sums finds the row's pair and its place in it, the row
// is the operation, the k-th dummy or a padding row, and consecutive lanes store consecutive rows of a column. A second kernel
// reads rows r and r + 1 back for the first-change flags and RANGE_CHECK; permuted_cols fills the last two columns.
// The number of rows depends on the data: sort, counts, scan and every refusal are decided on the device first, the host reads
// 16 bytes (the call's one wait), and nothing has touched the trace by then.
#include "memory_table.h"

#include <string>

#include "ctx.h"
#include "program_asm.h"
#include "table_args.h"

namespace plonky2_hip {

namespace {

constexpr uint32_t T = MEMORY_TABLE_THREADS;
constexpr uint32_t W = MEMORY_TABLE_OP_WORDS;
constexpr uint64_t LOW32 = 0xFFFFFFFFull;

// the limits of an operation's words, and the first sort key: timestamp << 32 | position
__global__ __launch_bounds__(T) void mt_first_key(const uint64_t *__restrict__ ops, uint32_t num_ops, uint64_t *__restrict__ keys,
                                                  MemoryTableHeader *header) {
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    if (i >= num_ops) return;
    const uint64_t *op = ops + (uint64_t)i * W;
    uint32_t bad = 0;
    for (uint32_t c = 0; c < W; ++c) {
        const uint64_t w = op[c];
        if (c == MT_FILTER || c == MT_IS_READ) bad |= w > 1 ? MT_BAD_FLAG : 0;
        else bad |= w > LOW32 ? MT_BAD_WORD : 0;
    }
    if (bad) atomicOr(&header->status, bad);
    keys[i] = (op[MT_TIMESTAMP] & LOW32) << 32 | i;
}

// between two rounds: the key of the next field, at the place the last round gave the operation
__global__ __launch_bounds__(T) void mt_next_key(const uint64_t *__restrict__ ops, uint32_t num_ops, uint64_t *__restrict__ keys, uint32_t field) {
    const uint32_t j = blockIdx.x * T + threadIdx.x;
    if (j >= num_ops) return;
    const uint32_t i = (uint32_t)keys[j];
    keys[j] = (ops[(uint64_t)i * W + field] & LOW32) << 32 | i;
}

// counts[j]: the dummies fill_gaps pushes for the pair (j, j + 1) of sorted operations; counts[num_ops - 1] = counts[num_ops] = 0.
// n != 0: a context or segment gap whose range check (the difference - 1) is n or more is what the reference's assert in
// generate_first_change_flags_and_rc catches.
__global__ __launch_bounds__(T) void mt_pair_counts(const uint64_t *__restrict__ ops, uint32_t num_ops, const uint64_t *__restrict__ keys,
                                                    uint64_t *__restrict__ counts, uint32_t log_step, uint64_t n, MemoryTableHeader *header) {
    const uint32_t j = blockIdx.x * T + threadIdx.x;
    if (j >= num_ops) return;
    if (j == num_ops - 1) {
        counts[j] = 0;
        counts[num_ops] = 0;
        return;
    }
    const uint64_t *a = ops + (uint64_t)(uint32_t)keys[j] * W, *b = ops + (uint64_t)(uint32_t)keys[j + 1] * W;
    const uint64_t max_rc = (1ull << log_step) - 1;
    uint64_t count = 0, gap = 0;
    if ((a[MT_ADDR_CONTEXT] ^ b[MT_ADDR_CONTEXT]) & LOW32) gap = (b[MT_ADDR_CONTEXT] & LOW32) - (a[MT_ADDR_CONTEXT] & LOW32) - 1;
    else if ((a[MT_ADDR_SEGMENT] ^ b[MT_ADDR_SEGMENT]) & LOW32) gap = (b[MT_ADDR_SEGMENT] & LOW32) - (a[MT_ADDR_SEGMENT] & LOW32) - 1;
    else if ((a[MT_ADDR_VIRTUAL] ^ b[MT_ADDR_VIRTUAL]) & LOW32) count = ((b[MT_ADDR_VIRTUAL] & LOW32) - (a[MT_ADDR_VIRTUAL] & LOW32) - 1) >> log_step;
    else {
        const uint64_t dts = (b[MT_TIMESTAMP] & LOW32) - (a[MT_TIMESTAMP] & LOW32);
        count = dts ? (dts - 1) / max_rc : 0;
    }
    counts[j] = count;
    if (count) atomicMax(&header->last_pair, j + 1);
    if (n && gap >= n) atomicOr(&header->status, (uint32_t)MT_BAD_GAP);
}

// sums: the exclusive prefix sums of the counts
__global__ void mt_decide(uint32_t num_ops, const uint64_t *__restrict__ sums, uint64_t n, MemoryTableHeader *header) {
    const uint64_t rows = num_ops + sums[num_ops];
    header->rows = rows;
    if (n && rows > n) header->status |= MT_BAD_ROWS;
}

// One thread per row. The rows without the padding are operation j at j + sums[j] and its dummies behind it; the padding rows
// stand behind the last dummy (at last_pair + sums[last_pair], where the next operation would be), or behind everything.
__global__ __launch_bounds__(T) void mt_rows(const uint64_t *__restrict__ ops, uint32_t num_ops, const uint64_t *__restrict__ keys,
                                             const uint64_t *__restrict__ sums, uint32_t log_step, uint64_t n, uint64_t *__restrict__ trace,
                                             uint64_t stride, const MemoryTableHeader *header) {
    if (header->status) return;
    const uint64_t r = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (r >= n) return;
    const uint64_t rows = header->rows, padding = n - rows;
    const uint32_t last_pair = header->last_pair;
    const uint64_t pad_start = last_pair ? last_pair + sums[last_pair] : rows;
    const bool is_padding = r >= pad_start && r < pad_start + padding;
    const uint64_t q = is_padding ? pad_start - 1 : (r < pad_start ? r : r - padding);  // the row among operations and dummies
    uint32_t lo = 0, hi = num_ops - 1;  // the last operation at or before row q
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (mid + sums[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t k = q - (lo + sums[lo]);  // 0: the operation itself; else its k-th dummy
    const uint64_t *op = ops + (uint64_t)(uint32_t)keys[lo] * W;
    uint64_t w[W];
#pragma unroll
    for (uint32_t c = 0; c < W; ++c) w[c] = op[c];
    if (k) {
        const uint64_t next_virtual = ops[(uint64_t)(uint32_t)keys[lo + 1] * W + MT_ADDR_VIRTUAL];
        const uint64_t max_rc = (1ull << log_step) - 1;
        if (next_virtual != w[MT_ADDR_VIRTUAL]) {
            w[MT_ADDR_VIRTUAL] += k << log_step;
            w[MT_TIMESTAMP] = 0;
        } else {
            w[MT_TIMESTAMP] += k * max_rc;
        }
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) w[MT_VALUE_START + c] = 0;
    }
    if (k || is_padding) {
        w[MT_FILTER] = 0;
        w[MT_IS_READ] = 1;
    }
#pragma unroll
    for (uint32_t c = 0; c < W; ++c) trace[c * stride + r] = w[c];
    for (uint32_t c = MT_VIRTUAL_FIRST_CHANGE + 1; c < MT_RANGE_CHECK; ++c) trace[c * stride + r] = 0;
    trace[MT_COUNTER * stride + r] = r;
}

// generate_first_change_flags_and_rc (memory_stark.rs:72-117); the last row keeps the zeros of into_row
__global__ __launch_bounds__(T) void mt_flags(uint64_t n, uint64_t *__restrict__ trace, uint64_t stride, const MemoryTableHeader *header) {
    if (header->status) return;
    const uint64_t r = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (r >= n) return;
    uint64_t context_first_change = 0, segment_first_change = 0, virtual_first_change = 0, range_check = 0;
    if (r + 1 < n) {
        const uint64_t context = trace[MT_ADDR_CONTEXT * stride + r], next_context = trace[MT_ADDR_CONTEXT * stride + r + 1];
        const uint64_t segment = trace[MT_ADDR_SEGMENT * stride + r], next_segment = trace[MT_ADDR_SEGMENT * stride + r + 1];
        const uint64_t virt = trace[MT_ADDR_VIRTUAL * stride + r], next_virt = trace[MT_ADDR_VIRTUAL * stride + r + 1];
        const uint64_t timestamp = trace[MT_TIMESTAMP * stride + r], next_timestamp = trace[MT_TIMESTAMP * stride + r + 1];
        context_first_change = context != next_context;
        segment_first_change = segment != next_segment && !context_first_change;
        virtual_first_change = virt != next_virt && !segment_first_change && !context_first_change;
        if (context_first_change) range_check = next_context - context - 1;
        else if (segment_first_change) range_check = next_segment - segment - 1;
        else if (virtual_first_change) range_check = next_virt - virt - 1;
        else range_check = next_timestamp - timestamp;
    }
    trace[MT_CONTEXT_FIRST_CHANGE * stride + r] = context_first_change;
    trace[MT_SEGMENT_FIRST_CHANGE * stride + r] = segment_first_change;
    trace[MT_VIRTUAL_FIRST_CHANGE * stride + r] = virtual_first_change;
    trace[MT_RANGE_CHECK * stride + r] = range_check;
}

uint32_t blocks_for(uint64_t count) { return (uint32_t)((count + T - 1) / T); }

// fill_gaps: max_rc = num_ops.next_power_of_two() - 1; returns log2(max_rc + 1)
uint32_t log_step_of(uint64_t num_ops) {
    uint32_t log = 0;
    while ((1ull << log) < num_ops) ++log;
    return log;
}

}  // namespace

MemoryTableScratch memory_table_scratch_layout(void *base, uint64_t num_ops, uint32_t log_n) {
    MemoryTableScratch s;
    const uint64_t n = 1ull << log_n;
    s.sort = lookup_scratch_layout(base, n > num_ops ? n : num_ops);
    s.lookup = lookup_scratch_layout(base, n);
    s.header = base ? reinterpret_cast<MemoryTableHeader *>(static_cast<uint64_t *>(base) + s.sort.words) : nullptr;
    s.words = s.sort.words + sizeof(MemoryTableHeader) / 8;
    return s;
}

namespace {

// the limits, the first key and the four rounds, least significant field first
hipError_t enqueue_sort(const uint64_t *d_ops, uint64_t num_ops, const MemoryTableScratch &s, hipStream_t stream) {
    const uint32_t ops32 = (uint32_t)num_ops, blocks = blocks_for(num_ops);
    hipError_t e = hipMemsetAsync(s.header, 0, sizeof(MemoryTableHeader), stream);
    if (e != hipSuccess) return e;
    mt_first_key<<<dim3(blocks), dim3(T), 0, stream>>>(d_ops, ops32, s.sort.keys, s.header);
    for (uint32_t field : {MT_ADDR_VIRTUAL, MT_ADDR_SEGMENT, MT_ADDR_CONTEXT}) {
        e = lookup_sort_by_upper_half(s.sort.keys, num_ops, s.sort, stream);
        if (e != hipSuccess) return e;
        mt_next_key<<<dim3(blocks), dim3(T), 0, stream>>>(d_ops, ops32, s.sort.keys, field);
    }
    return lookup_sort_by_upper_half(s.sort.keys, num_ops, s.sort, stream);
}

// the dummies of every pair, their prefix sums, the number of rows and the decision
hipError_t enqueue_gaps(const uint64_t *d_ops, uint64_t num_ops, uint64_t n, const MemoryTableScratch &s, hipStream_t stream) {
    uint64_t *counts = s.sort.ranks;
    mt_pair_counts<<<dim3(blocks_for(num_ops)), dim3(T), 0, stream>>>(d_ops, (uint32_t)num_ops, s.sort.keys, counts, log_step_of(num_ops), n, s.header);
    hipError_t e = lookup_exclusive_sums(counts, num_ops + 1, s.sort.totals, stream);
    if (e != hipSuccess) return e;
    mt_decide<<<dim3(1), dim3(1), 0, stream>>>((uint32_t)num_ops, counts, n, s.header);
    return hipGetLastError();
}

hipError_t enqueue_rows(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride, const MemoryTableScratch &s,
                        hipStream_t stream) {
    const uint64_t n = 1ull << log_n;
    mt_rows<<<dim3(blocks_for(n)), dim3(T), 0, stream>>>(d_ops, (uint32_t)num_ops, s.sort.keys, s.sort.ranks, log_step_of(num_ops), n, d_trace,
                                                         trace_stride, s.header);
    return hipGetLastError();
}

hipError_t enqueue_flags(uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride, const MemoryTableScratch &s, hipStream_t stream) {
    const uint64_t n = 1ull << log_n;
    mt_flags<<<dim3(blocks_for(n)), dim3(T), 0, stream>>>(n, d_trace, trace_stride, s.header);
    return hipGetLastError();
}

hipError_t enqueue_lookup(uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride, const MemoryTableScratch &s, hipStream_t stream) {
    return lookup_permuted_cols(d_trace + MT_RANGE_CHECK * trace_stride, d_trace + MT_COUNTER * trace_stride, 1ull << log_n,
                                d_trace + MT_RANGE_CHECK_PERMUTED * trace_stride, d_trace + MT_COUNTER_PERMUTED * trace_stride, s.lookup, stream);
}

}  // namespace

hipError_t memory_table_count(const uint64_t *d_ops, uint64_t num_ops, uint64_t n, const MemoryTableScratch &s, MemoryTableHeader *h,
                              hipStream_t stream) {
    if (num_ops < 2 || num_ops > MEMORY_TABLE_MAX_OPS) return hipErrorInvalidValue;
    hipError_t e = enqueue_sort(d_ops, num_ops, s, stream);
    if (e != hipSuccess) return e;
    e = enqueue_gaps(d_ops, num_ops, n, s, stream);
    if (e != hipSuccess) return e;
    return read_status(h, s.header, sizeof(MemoryTableHeader), stream);
}

hipError_t memory_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                             const MemoryTableScratch &s, hipStream_t stream) {
    if (trace_stride < (1ull << log_n) || !d_trace) return hipErrorInvalidValue;
    hipError_t e = enqueue_rows(d_ops, num_ops, log_n, d_trace, trace_stride, s, stream);
    if (e != hipSuccess) return e;
    e = enqueue_flags(log_n, d_trace, trace_stride, s, stream);
    if (e != hipSuccess) return e;
    return enqueue_lookup(log_n, d_trace, trace_stride, s, stream);
}

hipError_t memory_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                 const MemoryTableScratch &s, MemoryTableHeader *h, float *ms, hipStream_t stream) {
    StageClock<7> clock(stream);
    hipError_t e = clock.created;
    const uint64_t n = 1ull << log_n;
    if (e == hipSuccess) e = clock.mark(0);
    if (e == hipSuccess) e = enqueue_sort(d_ops, num_ops, s, stream);
    if (e == hipSuccess) e = clock.mark(1);
    if (e == hipSuccess) e = enqueue_gaps(d_ops, num_ops, n, s, stream);
    if (e == hipSuccess) e = clock.mark(2);
    if (e == hipSuccess) e = read_status(h, s.header, sizeof(MemoryTableHeader), stream);
    const bool fill = e == hipSuccess && h->status == 0;
    if (e == hipSuccess) e = clock.mark(3);
    if (fill && e == hipSuccess) e = enqueue_rows(d_ops, num_ops, log_n, d_trace, trace_stride, s, stream);
    if (e == hipSuccess) e = clock.mark(4);
    if (fill && e == hipSuccess) e = enqueue_flags(log_n, d_trace, trace_stride, s, stream);
    if (e == hipSuccess) e = clock.mark(5);
    if (fill && e == hipSuccess) e = enqueue_lookup(log_n, d_trace, trace_stride, s, stream);
    if (e == hipSuccess) e = clock.mark(6);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    const int from[5] = {0, 1, 3, 4, 5};  // the wait for the header between the gaps and the rows belongs to no stage
    for (int k = 0; k < 5 && e == hipSuccess; ++k) e = clock.elapsed(&ms[k], from[k], from[k] + 1);
    return e;
}

}  // namespace plonky2_hip

using namespace plonky2_hip;

static bool memory_table_shape_ok(uint64_t num_ops, uint32_t degree_bits) {
    return num_ops >= 2 && num_ops <= MEMORY_TABLE_MAX_OPS && degree_bits >= 1 && degree_bits <= MEMORY_TABLE_MAX_DEGREE_BITS;
}

extern "C" uint64_t gl_memory_table_scratch_bytes(uint64_t num_ops, uint32_t degree_bits) {
    if (!memory_table_shape_ok(num_ops, degree_bits)) return 0;
    return memory_table_scratch_layout(nullptr, num_ops, degree_bits).words * 8;
}

// what is refused before anything is launched; empty: nothing
static std::string memory_table_argument_error(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, const uint64_t *d_trace,
                                               uint64_t trace_stride, const void *d_scratch, const void *h_out, const void *ctx) {
    if (!ctx || !d_ops || !d_scratch || !h_out) return "null pointer";
    if (num_ops < 2 || num_ops > MEMORY_TABLE_MAX_OPS) return "num_ops must be in 2 ..= 2^30";
    std::string why = degree_bits_error(degree_bits, MEMORY_TABLE_MAX_DEGREE_BITS);
    if (why.empty()) why = scratch_alignment_error(d_scratch);
    if (!why.empty()) return why;
    const uint64_t n = 1ull << degree_bits;
    const uint64_t scratch_bytes = memory_table_scratch_layout(nullptr, num_ops, degree_bits).words * 8;
    const uint64_t ops_bytes = num_ops * MEMORY_TABLE_OP_WORDS * 8;
    if (bytes_overlap(d_ops, ops_bytes, d_scratch, scratch_bytes)) return "d_scratch overlaps d_ops";
    if (d_trace) {
        why = trace_stride_error(trace_stride, n);
        if (!why.empty()) return why;
        const uint64_t bytes = trace_bytes(MEMORY_TABLE_COLUMNS, trace_stride, n);
        if (bytes_overlap(d_trace, bytes, d_ops, ops_bytes)) return "d_trace overlaps d_ops";
        if (bytes_overlap(d_trace, bytes, d_scratch, scratch_bytes)) return "d_trace overlaps d_scratch";
    }
    return "";
}

// the refusals the device decided, read from the header
static GlError memory_table_data_error(const MemoryTableHeader &h) {
    if (h.status & MT_BAD_FLAG) return fail(GL_E_INVALID, "gl_memory_table_trace: FILTER or IS_READ of an operation is neither 0 nor 1");
    if (h.status & MT_BAD_WORD)
        return fail(GL_E_INVALID, "gl_memory_table_trace: a timestamp, address part or value limb of an operation is 2^32 or more");
    if (h.status & MT_BAD_ROWS)
        return fail(GL_E_INVALID, "gl_memory_table_trace: the operations and the dummy reads that fill their gaps take " + std::to_string(h.rows) +
                                      " rows, more than the 2^degree_bits rows of the trace");
    if (h.status & MT_BAD_GAP)
        return fail(GL_E_INVALID, "gl_memory_table_trace: a context or segment gap whose range check would not be below the 2^degree_bits rows of the "
                                  "trace (fill_gaps never fills those; the reference asserts \"Range check ... is too large\")");
    return ok();
}

extern "C" GlError gl_memory_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                         void *d_scratch, uint64_t *h_rows, void *ctx) {
    DeviceCall device_call(ctx);
    const std::string why = memory_table_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, h_rows, ctx);
    if (!why.empty()) return fail(GL_E_INVALID, "gl_memory_table_trace: " + why);
    const MemoryTableScratch scratch = memory_table_scratch_layout(d_scratch, num_ops, degree_bits);
    *h_rows = 0;
    MemoryTableHeader h;
    HIP_TRY(memory_table_count(d_ops, num_ops, d_trace ? 1ull << degree_bits : 0, scratch, &h, S(ctx)->stream));
    if (!(h.status & (MT_BAD_FLAG | MT_BAD_WORD))) *h_rows = h.rows;
    if (h.status) return memory_table_data_error(h);
    if (d_trace) HIP_TRY(memory_table_fill(d_ops, num_ops, degree_bits, d_trace, trace_stride, scratch, S(ctx)->stream));
    return ok();
}

extern "C" GlError gl_debug_memory_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                                  uint64_t trace_stride, void *d_scratch, float *h_ms, void *ctx) {
    DeviceCall device_call(ctx);
    std::string why = memory_table_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, h_ms, ctx);
    if (why.empty() && !d_trace) why = "null pointer";
    if (!why.empty()) return fail(GL_E_INVALID, "gl_debug_memory_table_stage_ms: " + why);
    MemoryTableHeader h;
    HIP_TRY(memory_table_stage_ms(d_ops, num_ops, degree_bits, d_trace, trace_stride, memory_table_scratch_layout(d_scratch, num_ops, degree_bits), &h,
                                  h_ms, S(ctx)->stream));
    return h.status ? memory_table_data_error(h) : ok();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The constraints of the reference's memory table (evm/src/memory/memory_stark.rs:242-319 with lookup.rs:19-33) as ONE STARK
// program: plonky2_gpu_amd/memory_table.py program(), call for call (tests/test_memory_table_ref.py holds the two against each
// other word for word). Host code; the columns are memory_table.h's.
namespace {

using namespace plonky2_hip::program_asm;

Program memory_table_program(ImmediatePool &pool) {
    StarkAsm a(&pool);
    const int one = a.imm(1);
    // the filter is 0 or 1
    const int filter = a.local(MT_FILTER);
    {
        const int t = a.sub(filter, one);
        a.mul(filter, t, t);
        a.emit(t);
        a.free1(t);
    }
    // a dummy row (filter off) is a read
    {
        const int is_dummy = a.sub(one, filter);
        const int is_read = a.local(MT_IS_READ);
        const int is_write = a.sub(one, is_read);
        const int t = a.mul(is_dummy, is_write);
        a.emit(t);
        a.free({t, is_dummy, is_write, is_read, filter});
    }
    // first set of ordering constraints: the first_change flags and address_unchanged are boolean
    const int context_first_change = a.local(MT_CONTEXT_FIRST_CHANGE);
    const int segment_first_change = a.local(MT_SEGMENT_FIRST_CHANGE);
    const int virtual_first_change = a.local(MT_VIRTUAL_FIRST_CHANGE);
    const int address_unchanged = a.sub(one, context_first_change);
    a.sub(address_unchanged, segment_first_change, address_unchanged);
    a.sub(address_unchanged, virtual_first_change, address_unchanged);
    for (int flag : {context_first_change, segment_first_change, virtual_first_change, address_unchanged}) {
        const int t = a.sub(one, flag);
        a.mul(flag, t, t);
        a.emit(t);
        a.free1(t);
    }
    // second set: no change before the column of the flag that is set
    int diffs[4];
    const int diff_columns[4] = {MT_ADDR_CONTEXT, MT_ADDR_SEGMENT, MT_ADDR_VIRTUAL, MT_TIMESTAMP};
    for (int k = 0; k < 4; k++) {
        const int nxt = a.next(diff_columns[k]);
        const int local = a.local(diff_columns[k]);
        a.sub(nxt, local, nxt);
        a.free1(local);
        diffs[k] = nxt;
    }
    const int d_context = diffs[0], d_segment = diffs[1], d_virtual = diffs[2], d_timestamp = diffs[3];
    const int transitions[6][2] = {{segment_first_change, d_context}, {virtual_first_change, d_context}, {virtual_first_change, d_segment},
                                   {address_unchanged, d_context},    {address_unchanged, d_segment},    {address_unchanged, d_virtual}};
    for (const auto &fd : transitions) {
        const int t = a.mul(fd[0], fd[1]);
        a.emit_transition(t);
        a.free1(t);
    }
    // third set: the range check is the difference of the column that should be increasing
    {
        const int computed = a.sub(d_context, one);
        a.mul(context_first_change, computed, computed);
        const int terms[2][2] = {{segment_first_change, d_segment}, {virtual_first_change, d_virtual}};
        for (const auto &fd : terms) {
            const int t = a.sub(fd[1], one);
            a.mul(fd[0], t, t);
            a.add(computed, t, computed);
            a.free1(t);
        }
        const int t = a.mul(address_unchanged, d_timestamp);
        a.add(computed, t, computed);
        a.free1(t);
        const int range_check = a.local(MT_RANGE_CHECK);
        a.sub(range_check, computed, computed);
        a.emit_transition(computed);
        a.free({computed, range_check});
    }
    // the purportedly ordered log: a read of an unchanged address sees the value of the row before
    const int gate = a.next(MT_IS_READ);
    a.mul(gate, address_unchanged, gate);
    for (int i = 0; i < 8; i++) {
        const int nxt = a.next(MT_VALUE_START + i);
        const int local = a.local(MT_VALUE_START + i);
        a.sub(nxt, local, nxt);
        a.mul(gate, nxt, nxt);
        a.emit(nxt);
        a.free({nxt, local});
    }
    a.release();
    a.eval_lookups(MT_RANGE_CHECK_PERMUTED, MT_COUNTER_PERMUTED);
    return a.instrs;
}

}  // namespace

extern "C" GlError gl_memory_table_program(GlGatePrograms *out) { return emit_table_program("gl_memory_table_program", memory_table_program, out); }
