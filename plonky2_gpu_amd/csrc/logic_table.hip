// logic_table.hip — the trace of the reference's logic table (evm/src/logic.rs:111-176) built on the device from a compact
// operation list: 523 columns, one row per AND / OR / XOR of two 256-bit words, zero rows behind them.
//
// A record is 17 words (the operator and the 2 x 8 limbs of the inputs, 136 bytes); its row is 523 words (4184 bytes): three
// flags, the 512 bits of the inputs and the eight limbs of the result, which the device computes. The kernel is bound by its
// stores, as keccak_table.hip's is: 523 * 8 * n bytes against 136 * num_ops bytes of loads.
//   - validation: one thread per WORD of the list (coalesced), the lowest record at fault per kind of fault with a vector
//     atomicMin into the 16 bytes of scratch; the host reads them — the call's one wait — before anything touches the trace;
//   - rows: one thread per row, consecutive lanes hold consecutive rows, so every column store of a wave is one contiguous run
//     of 512 bytes. The same template with two adjacent rows per thread — 16 bytes per lane, 1 KiB per wave and store; it needs
//     a 16-byte aligned d_trace and an even pitch, and its rows are operations or padding one by one, so a pair may straddle —
//     was measured against it and takes 5 to 23 % longer: gl_logic_table_trace never takes it, it stays
//     behind gl_debug_logic_table_fill for tools/bench_logic_table.py.
// The record loads are strided by 136 bytes per thread — 3 % of the traffic; staging them through LDS (coalesced loads, a
// barrier, reads at a pitch of 17 words) was measured and changed nothing beyond the spread at 2^18 and 2^20 rows and cost 7 to
// 11 % at 2^14 and 2^16. The limb loops are unrolled so that the limbs are never indexed by a register; the
// bit index is a run-time loop per limb, as in keccak_table.hip.
#include "logic_table.h"

#include <string>

#include "ctx.h"
#include "program_asm.h"
#include "table_args.h"

namespace plonky2_hip {

namespace {

constexpr uint32_t T = LOGIC_TABLE_THREADS;
constexpr uint32_t W = LOGIC_TABLE_OP_WORDS;
constexpr uint32_t LIMBS = LOGIC_TABLE_LIMBS;
constexpr uint64_t LOW32 = 0xFFFFFFFFull;

__global__ __launch_bounds__(T) void lt_validate(const uint64_t *__restrict__ ops, uint64_t words, LogicTableStatus *status) {
    const uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (i >= words) return;
    const uint64_t w = ops[i];
    const uint32_t record = (uint32_t)(i / W);
    if (i % W == 0) {
        if (w > 2) atomicMin(&status->bad_operator, record);
    } else if (w > LOW32) {
        atomicMin(&status->bad_limb, record);
    }
}

// R adjacent rows of one column: 8 bytes, or one 16-byte store
template <uint32_t R>
__device__ __forceinline__ void lt_store(uint64_t *__restrict__ p, const uint64_t (&v)[R]) {
    if constexpr (R == 1) p[0] = v[0];
    else *reinterpret_cast<ulonglong2 *>(p) = make_ulonglong2(v[0], v[1]);
}

// the 256 bit columns of one input, from column `col` on, at this thread's rows
template <uint32_t R>
__device__ __forceinline__ void lt_store_bits(uint64_t *__restrict__ col, uint64_t stride, const uint32_t (&limbs)[R][LIMBS]) {
#pragma unroll
    for (uint32_t i = 0; i < LIMBS; i++) {
#pragma unroll 4
        for (uint32_t z = 0; z < 32; z++) {
            uint64_t v[R];
#pragma unroll
            for (uint32_t j = 0; j < R; j++) v[j] = (limbs[j][i] >> z) & 1u;
            lt_store<R>(col + (uint64_t)(32 * i + z) * stride, v);
        }
    }
}

// n is even and R divides it: a thread's R rows are all below n or none is
template <uint32_t R>
__global__ __launch_bounds__(T) void logic_table_rows_kernel(const uint64_t *__restrict__ ops, uint64_t num_ops, uint64_t n,
                                                             uint64_t *__restrict__ trace, uint64_t stride) {
    const uint64_t row = ((uint64_t)blockIdx.x * T + threadIdx.x) * R;
    if (row >= n) return;
    uint32_t op[R], x[R][LIMBS], y[R][LIMBS];
#pragma unroll
    for (uint32_t j = 0; j < R; j++) {
        const bool real = row + j < num_ops;  // else a padding row: all zero
        const uint64_t *record = ops + (row + j) * W;
        op[j] = real ? (uint32_t)record[0] : 3u;
#pragma unroll
        for (uint32_t i = 0; i < LIMBS; i++) {
            x[j][i] = real ? (uint32_t)record[1 + i] : 0u;
            y[j][i] = real ? (uint32_t)record[1 + LIMBS + i] : 0u;
        }
    }

    uint64_t *out = trace + row;
    uint64_t v[R];
#pragma unroll
    for (uint32_t f = 0; f < 3; f++) {
#pragma unroll
        for (uint32_t j = 0; j < R; j++) v[j] = op[j] == f ? 1 : 0;
        lt_store<R>(out + (uint64_t)(LT_IS_AND + f) * stride, v);
    }
    lt_store_bits<R>(out + (uint64_t)LT_INPUT0 * stride, stride, x);
    lt_store_bits<R>(out + (uint64_t)LT_INPUT1 * stride, stride, y);
#pragma unroll
    for (uint32_t i = 0; i < LIMBS; i++) {
#pragma unroll
        for (uint32_t j = 0; j < R; j++) {
            const uint32_t a = x[j][i], b = y[j][i];
            v[j] = op[j] == LT_IS_AND ? (a & b) : op[j] == LT_IS_OR ? (a | b) : op[j] == LT_IS_XOR ? (a ^ b) : 0u;
        }
        lt_store<R>(out + (uint64_t)(LT_RESULT + i) * stride, v);
    }
}

}  // namespace

hipError_t logic_table_validate(const uint64_t *d_ops, uint64_t num_ops, LogicTableStatus *d_status, LogicTableStatus *h, hipStream_t stream) {
    if (!d_ops || !d_status || !h || num_ops == 0 || num_ops > (1ull << LOGIC_TABLE_MAX_DEGREE_BITS)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_status, 0xFF, sizeof(LogicTableStatus), stream);
    if (e != hipSuccess) return e;
    const uint64_t words = num_ops * W;
    lt_validate<<<dim3((unsigned)((words + T - 1) / T)), dim3(T), 0, stream>>>(d_ops, words, d_status);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return read_status(h, d_status, sizeof(LogicTableStatus), stream);
}

hipError_t logic_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                            uint32_t rows_per_thread, hipStream_t stream) {
    const uint64_t n = 1ull << log_n;
    if (log_n == 0 || log_n > LOGIC_TABLE_MAX_DEGREE_BITS || trace_stride < n || num_ops > n || !d_trace || (num_ops && !d_ops) || rows_per_thread > 2)
        return hipErrorInvalidValue;
    if (rows_per_thread == 2 && (((uintptr_t)d_trace & 15) || (trace_stride & 1))) return hipErrorInvalidValue;
    if (rows_per_thread == 0) rows_per_thread = 1;  // the measured choice (profiles/logic_table.json)
    const unsigned grid = (unsigned)((n / rows_per_thread + T - 1) / T);
    if (rows_per_thread == 2) logic_table_rows_kernel<2><<<dim3(grid), dim3(T), 0, stream>>>(d_ops, num_ops, n, d_trace, trace_stride);
    else logic_table_rows_kernel<1><<<dim3(grid), dim3(T), 0, stream>>>(d_ops, num_ops, n, d_trace, trace_stride);
    return hipGetLastError();
}

}  // namespace plonky2_hip

using namespace plonky2_hip;

static_assert(GL_LOGIC_TABLE_COLUMNS == LOGIC_TABLE_COLUMNS && GL_LOGIC_TABLE_OP_WORDS == LOGIC_TABLE_OP_WORDS &&
                  GL_LOGIC_TABLE_SCRATCH_BYTES == sizeof(LogicTableStatus),
              "plonky2_hip.h");

// what is refused before anything is launched; empty: nothing. d_scratch is checked where `with_scratch`.
static std::string logic_table_argument_error(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, const uint64_t *d_trace,
                                              uint64_t trace_stride, const void *d_scratch, bool with_scratch, const void *ctx) {
    if (!ctx || !d_trace || (num_ops && !d_ops) || (with_scratch && !d_scratch)) return "null pointer";
    std::string why = degree_bits_error(degree_bits, LOGIC_TABLE_MAX_DEGREE_BITS);
    if (!why.empty()) return why;
    const uint64_t n = 1ull << degree_bits;
    if (num_ops > n) return "num_ops exceeds the 2^degree_bits rows of the trace";
    why = trace_stride_error(trace_stride, n);
    if (why.empty() && with_scratch) why = scratch_alignment_error(d_scratch);
    if (!why.empty()) return why;
    const uint64_t ops_bytes = num_ops * LOGIC_TABLE_OP_WORDS * 8;
    const uint64_t bytes = trace_bytes(LOGIC_TABLE_COLUMNS, trace_stride, n);
    const uint64_t scratch_bytes = with_scratch ? sizeof(LogicTableStatus) : 0;
    if (bytes_overlap(d_trace, bytes, d_ops, ops_bytes)) return "d_trace overlaps d_ops";
    if (bytes_overlap(d_scratch, scratch_bytes, d_ops, ops_bytes)) return "d_scratch overlaps d_ops";
    if (bytes_overlap(d_trace, bytes, d_scratch, scratch_bytes)) return "d_trace overlaps d_scratch";
    return "";
}

extern "C" GlError gl_logic_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                        void *d_scratch, void *ctx) {
    DeviceCall device_call(ctx);
    const std::string why = logic_table_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, true, ctx);
    if (!why.empty()) return fail(GL_E_INVALID, "gl_logic_table_trace: " + why);
    if (num_ops) {
        LogicTableStatus h;
        HIP_TRY(logic_table_validate(d_ops, num_ops, static_cast<LogicTableStatus *>(d_scratch), &h, S(ctx)->stream));
        // the lowest record at fault; where it has both faults, its operator is named
        if (h.bad_operator != LT_NONE && h.bad_operator <= h.bad_limb)
            return fail(GL_E_INVALID, "gl_logic_table_trace: the operator of record " + std::to_string(h.bad_operator) + " is not 0 (AND), 1 (OR) or 2 (XOR)");
        if (h.bad_limb != LT_NONE)
            return fail(GL_E_INVALID, "gl_logic_table_trace: a limb of record " + std::to_string(h.bad_limb) + " is 2^32 or more");
    }
    HIP_TRY(logic_table_fill(d_ops, num_ops, degree_bits, d_trace, trace_stride, 0, S(ctx)->stream));
    return ok();
}

extern "C" GlError gl_debug_logic_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                             uint64_t trace_stride, uint32_t rows_per_thread, void *ctx) {
    DeviceCall device_call(ctx);
    std::string why = logic_table_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, nullptr, false, ctx);
    if (why.empty() && rows_per_thread != 1 && rows_per_thread != 2) why = "rows_per_thread must be 1 or 2";
    if (why.empty() && rows_per_thread == 2 && (((uintptr_t)d_trace & 15) || (trace_stride & 1)))
        why = "two rows per thread need a 16-byte aligned d_trace and an even trace_stride";
    if (!why.empty()) return fail(GL_E_INVALID, "gl_debug_logic_table_fill: " + why);
    HIP_TRY(logic_table_fill(d_ops, num_ops, degree_bits, d_trace, trace_stride, rows_per_thread, S(ctx)->stream));
    return ok();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The constraints of the reference's logic table (evm/src/logic.rs:182-231) as ONE STARK program:
// plonky2_gpu_amd/logic_table.py program(), call for call (tests/test_logic_table_ref.py holds the two against each other word
// for word). Host code; the columns are logic_table.h's.
namespace {

using namespace plonky2_hip::program_asm;

Program logic_table_program(ImmediatePool &pool) {
    StarkAsm a(&pool);
    // all bits are indeed bits
    for (int start : {LT_INPUT0, LT_INPUT1})
        for (int i = 0; i < (int)LOGIC_TABLE_VAL_BITS; i++) {
            a.release();
            const int bit = a.local(start + i);
            const int one = a.imm(1);
            const int t = a.sub(bit, one);
            a.emit(a.mul(bit, t));
        }
    // RESULT[i] = sum_coeff (x + y) + and_coeff (x AND y) on the limb's 32 bits
    for (int i = 0; i < (int)LOGIC_TABLE_LIMBS; i++) {
        a.release();
        const int x = a.limb([&](int z) { return a.local(LT_INPUT0 + z); }, 32 * i);
        const int y = a.limb([&](int z) { return a.local(LT_INPUT1 + z); }, 32 * i);
        const int x_land_y = a.limb(
            [&](int z) {
                const int x_bit = a.local(LT_INPUT0 + z);
                const int y_bit = a.local(LT_INPUT1 + z);
                a.mul(x_bit, y_bit, x_bit);
                a.free1(y_bit);
                return x_bit;
            },
            32 * i);
        const int is_and = a.local(LT_IS_AND);
        const int is_or = a.local(LT_IS_OR);
        const int is_xor = a.local(LT_IS_XOR);
        const int sum_coeff = a.add(is_or, is_xor);
        const int and_coeff = a.sub(is_and, is_or);
        a.mulk(is_xor, 1, is_xor);
        a.sub(and_coeff, is_xor, and_coeff);
        a.add(x, y, x);
        a.mul(sum_coeff, x, x);
        a.mul(and_coeff, x_land_y, x_land_y);
        a.add(x, x_land_y, x);
        const int result = a.local(LT_RESULT + i);
        a.emit(a.sub(result, x));
    }
    return a.instrs;
}

}  // namespace

extern "C" GlError gl_logic_table_program(GlGatePrograms *out) { return emit_table_program("gl_logic_table_program", logic_table_program, out); }
