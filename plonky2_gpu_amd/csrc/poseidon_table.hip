// poseidon_table.hip — the trace of the Poseidon table built on the device from a compact record list: the permutation unit of the
// reference's system_zero crate (generate_permutation_unit, system_zero/src/permutation_unit.rs:56-105), 248 columns that hold
// every cell a degree-3 constraint system needs for one width-12 permutation, and IS_REAL behind them; one row per record, the
// permutation of the all-zero state with IS_REAL = 0 on the rows behind them.
//
// A record is 13 words (104 bytes); its row is 249 words (1 992 bytes) and a whole permutation of arithmetic.
//   - validation: one thread per record, the lowest record at fault with a vector atomicMin and the number of ABSORB records
//     (one atomicAdd per wave) into the 16 bytes of scratch; the host reads them — the call's one wait — before anything
//     touches the trace;
//   - serial pass, only where a record is an ABSORB: one lane per record; the lane of a START that an ABSORB follows walks its
//     run — permute (poseidon_vector.h: it needs no full wave, so lanes may diverge), overwrite the absorbed elements, store the
//     twelve INPUT words of the continuation row — until the next START. A run as long as the list runs on one lane
//     (DESIGN.md §3.7.9 has what that costs);
//   - rows: one lane per row, consecutive lanes hold consecutive rows, so every column store of a wave is one contiguous run of
//     512 bytes. START rows take their input from the record, ABSORB rows from the INPUT columns the serial pass wrote, padding
//     rows take zero. The thirty rounds keep the state in registers and store mid_sbox, after_mds and after_sbox as they
//     appear. The full rounds record the state behind the MDS layer and BEFORE the next round's constants, so their layer runs
//     without the folded constants of poseidon::mds_layer and the constants are added afterwards; the partial rounds record
//     nothing behind their layer and keep the fused form. The kernel exists with the MDS layer on the matrix cores (poseidon.h)
//     and on the vector ALU (poseidon_vector.h); DESIGN.md §3.7.9 says which is the product's and by how much. The matrix-core
//     layer needs every lane of the wave active: the row index is clamped and the stores are predicated, nothing returns early.
// Every stored word is canonical: a record's element words are any u64 and are reduced once, where they are read.
#include "poseidon_table.h"

#include <string>

#include "ctx.h"
#include "poseidon.h"
#include "program_asm.h"
#include "table_args.h"

namespace plonky2_hip {

namespace {

constexpr uint32_t T = POSEIDON_TABLE_THREADS;
constexpr uint32_t OPW = POSEIDON_TABLE_OP_WORDS;
constexpr int SW = (int)POSEIDON_TABLE_WIDTH;
constexpr int HALF_FULL = (int)POSEIDON_TABLE_HALF_FULL;
constexpr int N_PARTIAL = (int)POSEIDON_TABLE_PARTIAL;
static_assert(SW == poseidon::W && HALF_FULL == poseidon::HALF_FULL && N_PARTIAL == poseidon::N_PARTIAL, "poseidon.h");

__device__ const uint32_t PT_ZERO_XY[2 * SW] __attribute__((aligned(64))) = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

__global__ __launch_bounds__(T) void pt_validate(const uint64_t *__restrict__ ops, uint64_t num_ops, PoseidonTableStatus *status) {
    const uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x;
    const uint64_t kind = i < num_ops ? ops[i * OPW] : 0;  // a kind word is not cut to 32 bits
    if (kind > POSEIDON_TABLE_MAX_ABSORB) atomicMin(&status->bad_kind, (uint32_t)i);
    const bool absorb = kind >= 1 && kind <= POSEIDON_TABLE_MAX_ABSORB;
    if (absorb && i == 0) atomicMin(&status->leading_absorb, 0u);
    const uint64_t in_wave = __ballot(absorb);  // no lane has returned: lane 0 adds for the wave
    if ((threadIdx.x & 63) == 0 && in_wave) atomicAdd(&status->absorbs, (uint32_t)__popcll(in_wave));
}

// One lane per record; the lane of a START that an ABSORB follows computes the INPUT words of its run's continuation rows.
__global__ __launch_bounds__(T) void poseidon_table_serial_kernel(const uint64_t *__restrict__ ops, uint64_t num_ops, uint64_t *__restrict__ trace,
                                                                  uint64_t stride) {
    const uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (i + 1 >= num_ops) return;
    if (ops[i * OPW] != 0 || ops[(i + 1) * OPW] == 0) return;
    uint64_t s[SW];
#pragma unroll
    for (int e = 0; e < SW; e++) s[e] = gl::canon(ops[i * OPW + 1 + e]);
    uint64_t j = i + 1;
    for (;;) {
        poseidon_vector::permute(s);
        const uint64_t *record = ops + j * OPW;
        const uint32_t k = (uint32_t)record[0];  // 1 .. 8: the validation has passed
#pragma unroll
        for (int e = 0; e < (int)POSEIDON_TABLE_MAX_ABSORB; e++)
            if ((uint32_t)e < k) s[e] = record[1 + e];
#pragma unroll
        for (int e = 0; e < SW; e++) {
            s[e] = gl::canon(s[e]);
            trace[(uint64_t)(PT_INPUT + e) * stride + j] = s[e];
        }
        j++;
        if (j >= num_ops || ops[j * OPW] == 0) break;
    }
}

// the MDS layer alone: what after_mds records
template <bool MATRIX>
__device__ __forceinline__ void pt_mds_plain(uint64_t (&s)[SW], const poseidon::MdsOperands &mo) {
    if constexpr (MATRIX) poseidon::mds_layer(s, mo, PT_ZERO_XY);
    else poseidon_vector::mds_layer(s, poseidon_vector::POSEIDON_ZERO_ROW);
}

// the MDS layer of round `round` with the constants of round + 1 folded in
template <bool MATRIX>
__device__ __forceinline__ void pt_mds_fused(uint64_t (&s)[SW], const poseidon::MdsOperands &mo, int round) {
    if constexpr (MATRIX) poseidon::mds_layer(s, mo, POSEIDON_MDS_XY + 2 * SW * round);
    else poseidon_vector::mds_layer(s, POSEIDON_ALL_ROUND_CONSTANTS + SW * (round + 1));
}

// One lane per row. `out` is the row's word of column 0; nothing is stored where !live (a lane beyond the trace, clamped to its
// last row so that the wave stays whole).
template <bool MATRIX>
__global__ __launch_bounds__(T) void poseidon_table_rows_kernel(const uint64_t *ops, uint64_t num_ops, uint64_t n, uint64_t *trace, uint64_t stride) {
    poseidon::MdsOperands mo = {};
    if constexpr (MATRIX) mo = poseidon::mds_operands();
    const uint64_t t = (uint64_t)blockIdx.x * T + threadIdx.x;
    const bool live = t < n;
    const uint64_t row = live ? t : n - 1;
    const bool real = row < num_ops;  // else a padding row: the permutation of the all-zero state
    uint64_t *out = trace + row;
    uint64_t s[SW];
    {
        const uint64_t *record = ops + (real ? row : 0) * OPW;
        const bool start = real && record[0] == 0;
#pragma unroll
        for (int i = 0; i < SW; i++) {
            uint64_t v = 0;
            if (start) v = gl::canon(record[1 + i]);
            else if (real) v = out[(uint64_t)(PT_INPUT + i) * stride];  // the serial pass wrote it, canonical
            s[i] = v;
        }
    }
    if constexpr (MATRIX) poseidon::require_full_wave();
    auto put = [&](uint32_t column, uint64_t v) {
        if (live) out[(uint64_t)column * stride] = gl::canon(v);
    };
#pragma unroll
    for (int i = 0; i < SW; i++) put(PT_INPUT + i, s[i]);
    put(PT_IS_REAL, real ? 1 : 0);

    // s has the round's constants: cube, record, to the seventh power; the layer; record; the next round's constants
    auto full_round = [&](int round, uint32_t column, bool last) {
#pragma unroll
        for (int i = 0; i < SW; i++) {
            const uint64_t x2 = gl::sqr(s[i]), x3 = gl::mul(s[i], x2);
            put(column + i, x3);
            s[i] = gl::mul(x3, gl::sqr(x2));
        }
        pt_mds_plain<MATRIX>(s, mo);
#pragma unroll
        for (int i = 0; i < SW; i++) {
            put(column + SW + i, s[i]);
            if (!last) s[i] = gl::add_canonical(s[i], POSEIDON_ALL_ROUND_CONSTANTS[SW * (round + 1) + i]);
        }
    };

#pragma unroll
    for (int i = 0; i < SW; i++) s[i] = gl::add_canonical(s[i], POSEIDON_ALL_ROUND_CONSTANTS[i]);
#pragma unroll 1
    for (int r = 0; r < HALF_FULL; r++) full_round(r, PT_FULL_FIRST + 2 * SW * r, false);
#pragma unroll 1
    for (int r = 0; r < N_PARTIAL; r++) {
        const uint64_t x2 = gl::sqr(s[0]), x3 = gl::mul(s[0], x2);
        put(PT_PARTIAL + 2 * r, x3);
        s[0] = gl::mul(x3, gl::sqr(x2));
        put(PT_PARTIAL + 2 * r + 1, s[0]);
        pt_mds_fused<MATRIX>(s, mo, HALF_FULL + r);
    }
#pragma unroll 1
    for (int r = 0; r < HALF_FULL; r++) full_round(HALF_FULL + N_PARTIAL + r, PT_FULL_SECOND + 2 * SW * r, r == HALF_FULL - 1);
}

uint32_t blocks_for(uint64_t count) { return (uint32_t)((count + T - 1) / T); }

hipError_t enqueue_validate(const uint64_t *d_ops, uint64_t num_ops, PoseidonTableStatus *d_status, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_status, 0xFF, 8, stream);  // bad_kind, leading_absorb: PT_NONE
    if (e == hipSuccess) e = hipMemsetAsync(&d_status->absorbs, 0, 8, stream);
    if (e != hipSuccess) return e;
    pt_validate<<<dim3(blocks_for(num_ops)), dim3(T), 0, stream>>>(d_ops, num_ops, d_status);
    return hipGetLastError();
}

hipError_t enqueue_serial(const uint64_t *d_ops, uint64_t num_ops, uint64_t *d_trace, uint64_t trace_stride, hipStream_t stream) {
    poseidon_table_serial_kernel<<<dim3(blocks_for(num_ops)), dim3(T), 0, stream>>>(d_ops, num_ops, d_trace, trace_stride);
    return hipGetLastError();
}

hipError_t enqueue_rows(const uint64_t *d_ops, uint64_t num_ops, uint64_t n, uint64_t *d_trace, uint64_t trace_stride, PoseidonTableMds mds,
                        hipStream_t stream) {
    if (mds == PT_MDS_PRODUCT) mds = PT_MDS_MATRIX_CORES;  // the measured choice (profiles/poseidon_table.json)
    if (mds == PT_MDS_MATRIX_CORES) poseidon_table_rows_kernel<true><<<dim3(blocks_for(n)), dim3(T), 0, stream>>>(d_ops, num_ops, n, d_trace, trace_stride);
    else poseidon_table_rows_kernel<false><<<dim3(blocks_for(n)), dim3(T), 0, stream>>>(d_ops, num_ops, n, d_trace, trace_stride);
    return hipGetLastError();
}

bool fill_arguments_ok(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, const uint64_t *d_trace, uint64_t trace_stride, PoseidonTableMds mds) {
    if (log_n == 0 || log_n > POSEIDON_TABLE_MAX_DEGREE_BITS || !d_trace || (num_ops && !d_ops) || mds > PT_MDS_VECTOR) return false;
    const uint64_t n = 1ull << log_n;
    return trace_stride >= n && num_ops <= n;
}

bool status_clean(const PoseidonTableStatus &h) { return h.bad_kind == PT_NONE && h.leading_absorb == PT_NONE; }

}  // namespace

hipError_t poseidon_table_validate(const uint64_t *d_ops, uint64_t num_ops, PoseidonTableStatus *d_status, PoseidonTableStatus *h, hipStream_t stream) {
    if (!d_ops || !d_status || !h || num_ops == 0 || num_ops > (1ull << POSEIDON_TABLE_MAX_DEGREE_BITS)) return hipErrorInvalidValue;
    hipError_t e = enqueue_validate(d_ops, num_ops, d_status, stream);
    if (e != hipSuccess) return e;
    return read_status(h, d_status, sizeof(PoseidonTableStatus), stream);
}

hipError_t poseidon_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t absorbs, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                               PoseidonTableMds mds, hipStream_t stream) {
    if (!fill_arguments_ok(d_ops, num_ops, log_n, d_trace, trace_stride, mds)) return hipErrorInvalidValue;
    if (absorbs) {
        hipError_t e = enqueue_serial(d_ops, num_ops, d_trace, trace_stride, stream);
        if (e != hipSuccess) return e;
    }
    return enqueue_rows(d_ops, num_ops, 1ull << log_n, d_trace, trace_stride, mds, stream);
}

hipError_t poseidon_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                   PoseidonTableStatus *d_status, PoseidonTableStatus *h, PoseidonTableMds mds, float *ms, hipStream_t stream) {
    if (!d_ops || !d_status || !h || !ms || num_ops == 0 || !fill_arguments_ok(d_ops, num_ops, log_n, d_trace, trace_stride, mds)) return hipErrorInvalidValue;
    StageClock<5> clock(stream);
    hipError_t e = clock.created;
    if (e == hipSuccess) e = clock.mark(0);
    if (e == hipSuccess) e = enqueue_validate(d_ops, num_ops, d_status, stream);
    if (e == hipSuccess) e = clock.mark(1);
    if (e == hipSuccess) e = read_status(h, d_status, sizeof(PoseidonTableStatus), stream);
    const bool fill = e == hipSuccess && status_clean(*h);
    const bool serial = fill && h->absorbs;
    if (e == hipSuccess) e = clock.mark(2);
    if (serial && e == hipSuccess) e = enqueue_serial(d_ops, num_ops, d_trace, trace_stride, stream);
    if (e == hipSuccess) e = clock.mark(3);
    if (fill && e == hipSuccess) e = enqueue_rows(d_ops, num_ops, 1ull << log_n, d_trace, trace_stride, mds, stream);
    if (e == hipSuccess) e = clock.mark(4);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = clock.elapsed(&ms[0], 0, 1);  // the wait for the status words behind it belongs to no stage
    if (e == hipSuccess) e = clock.elapsed(&ms[1], 2, 3);
    if (e == hipSuccess) e = clock.elapsed(&ms[2], 3, 4);
    if (e == hipSuccess && !serial) ms[1] = -1.0f;  // not run
    return e;
}

}  // namespace plonky2_hip

using namespace plonky2_hip;

static_assert(GL_POSEIDON_TABLE_COLUMNS == POSEIDON_TABLE_COLUMNS && GL_POSEIDON_TABLE_OP_WORDS == POSEIDON_TABLE_OP_WORDS &&
                  GL_POSEIDON_TABLE_SCRATCH_BYTES == sizeof(PoseidonTableStatus) && GL_POSEIDON_TABLE_MAX_DEGREE_BITS == POSEIDON_TABLE_MAX_DEGREE_BITS,
              "plonky2_hip.h");

// what is refused before anything is launched; empty: nothing
static std::string poseidon_table_argument_error(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, const uint64_t *d_trace,
                                                 uint64_t trace_stride, const void *d_scratch, const void *ctx) {
    if (!ctx || !d_trace || (num_ops && !d_ops) || !d_scratch) return "null pointer";
    std::string why = degree_bits_error(degree_bits, POSEIDON_TABLE_MAX_DEGREE_BITS);
    if (!why.empty()) return why;
    const uint64_t n = 1ull << degree_bits;
    if (num_ops > n) return "num_ops exceeds the 2^degree_bits rows of the trace";
    why = trace_stride_error(trace_stride, n);
    if (why.empty()) why = scratch_alignment_error(d_scratch);
    if (!why.empty()) return why;
    const uint64_t ops_bytes = num_ops * POSEIDON_TABLE_OP_WORDS * 8;
    const uint64_t bytes = trace_bytes(POSEIDON_TABLE_COLUMNS, trace_stride, n);
    const uint64_t scratch_bytes = sizeof(PoseidonTableStatus);
    if (bytes_overlap(d_trace, bytes, d_ops, ops_bytes)) return "d_trace overlaps d_ops";
    if (bytes_overlap(d_scratch, scratch_bytes, d_ops, ops_bytes)) return "d_scratch overlaps d_ops";
    if (bytes_overlap(d_trace, bytes, d_scratch, scratch_bytes)) return "d_trace overlaps d_scratch";
    return "";
}

// the refusals the device decided: the lowest record at fault; empty: nothing
static std::string poseidon_table_data_error(const PoseidonTableStatus &h) {
    if (h.leading_absorb != PT_NONE) return "record 0 is an ABSORB: it continues a sponge that no record starts";
    if (h.bad_kind != PT_NONE) return "the kind of record " + std::to_string(h.bad_kind) + " is not 0 (START) or 1 .. 8 (ABSORB)";
    return "";
}

extern "C" GlError gl_poseidon_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                           void *d_scratch, void *ctx) {
    DeviceCall device_call(ctx);
    const std::string why = poseidon_table_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, ctx);
    if (!why.empty()) return fail(GL_E_INVALID, "gl_poseidon_table_trace: " + why);
    PoseidonTableStatus h = {PT_NONE, PT_NONE, 0, 0};
    if (num_ops) {
        HIP_TRY(poseidon_table_validate(d_ops, num_ops, static_cast<PoseidonTableStatus *>(d_scratch), &h, S(ctx)->stream));
        const std::string bad = poseidon_table_data_error(h);
        if (!bad.empty()) return fail(GL_E_INVALID, "gl_poseidon_table_trace: " + bad);
    }
    HIP_TRY(poseidon_table_fill(d_ops, num_ops, h.absorbs, degree_bits, d_trace, trace_stride, PT_MDS_PRODUCT, S(ctx)->stream));
    return ok();
}

extern "C" GlError gl_debug_poseidon_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                                    uint64_t trace_stride, void *d_scratch, uint32_t mds, float *h_ms, void *ctx) {
    DeviceCall device_call(ctx);
    std::string why = poseidon_table_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, ctx);
    if (why.empty() && (!h_ms || !num_ops)) why = "null pointer";
    if (why.empty() && mds > PT_MDS_VECTOR) why = "mds must be 0 (the product's), 1 (matrix cores) or 2 (vector ALU)";
    if (!why.empty()) return fail(GL_E_INVALID, "gl_debug_poseidon_table_stage_ms: " + why);
    PoseidonTableStatus h;
    HIP_TRY(poseidon_table_stage_ms(d_ops, num_ops, degree_bits, d_trace, trace_stride, static_cast<PoseidonTableStatus *>(d_scratch), &h,
                                    (PoseidonTableMds)mds, h_ms, S(ctx)->stream));
    const std::string bad = poseidon_table_data_error(h);
    if (!bad.empty()) return fail(GL_E_INVALID, "gl_debug_poseidon_table_stage_ms: nothing was filled: " + bad);
    return ok();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The constraints of the reference's permutation unit (eval_permutation_unit, system_zero/src/permutation_unit.rs:108-172) as ONE
// STARK program, 236 constraints in the reference's order, and IS_REAL (IS_REAL - 1) behind them: plonky2_gpu_amd/poseidon_table.py
// program(), call for call (tests/test_poseidon_table_ref.py holds the two against each other word for word). Host code; the
// columns are poseidon_table.h's, the constants gate_emit.hip's host copy of poseidon_constants.h.
namespace {

using namespace plonky2_hip::program_asm;

Program poseidon_table_program(ImmediatePool &pool) {
    const PoseidonHostConstants k = poseidon_host_constants();
    StarkAsm a(&pool);
    int state[SW];
    for (int i = 0; i < SW; i++) state[i] = a.local(PT_INPUT + i);
    auto constant_layer = [&](int round) {
        for (int i = 0; i < SW; i++) {
            const int c = a.imm(k.all_round_constants[round * SW + i]);
            a.add(state[i], c, state[i]);
            a.free1(c);
        }
    };
    // state_cubed - mid_sbox; then state * mid_sbox^2 from the column
    auto sbox = [&](int i, int column) {
        const int x2 = a.mul(state[i], state[i]);
        a.mul(x2, state[i], x2);
        const int mid = a.local(column);
        a.emit(a.sub(x2, mid, x2));
        a.mul(mid, mid, x2);
        a.mul(state[i], x2, state[i]);
        a.free({x2, mid});
    };
    // row r = MDS_DIAG[r] state[r] + sum_i MDS_CIRC[i] state[(i + r) % 12] through accumulator 0: the weights of a row sum to 264
    auto mds_layer = [&]() {
        int fresh[SW];
        for (int r = 0; r < SW; r++) {
            std::vector<std::pair<int, uint64_t>> terms;
            for (int i = 0; i < SW; i++) terms.push_back({state[(i + r) % SW], k.mds_circ[i]});
            if (k.mds_diag[r]) terms.push_back({state[r], k.mds_diag[r]});
            fresh[r] = a.weighted_sum(terms);
        }
        for (int i = 0; i < SW; i++) {
            a.free1(state[i]);
            state[i] = fresh[i];
        }
    };
    // state - column; the column from here on
    auto check_against = [&](int i, int column) {
        const int cell = a.local(column);
        a.emit(a.sub(state[i], cell, state[i]));
        a.free1(state[i]);
        state[i] = cell;
    };
    auto full_rounds = [&](int first_round, int first_column) {
        for (int r = 0; r < HALF_FULL; r++) {
            constant_layer(first_round + r);
            for (int i = 0; i < SW; i++) sbox(i, first_column + 2 * SW * r + i);
            mds_layer();
            for (int i = 0; i < SW; i++) check_against(i, first_column + 2 * SW * r + SW + i);
        }
    };
    full_rounds(0, PT_FULL_FIRST);
    for (int r = 0; r < N_PARTIAL; r++) {
        constant_layer(HALF_FULL + r);
        sbox(0, PT_PARTIAL + 2 * r);
        check_against(0, PT_PARTIAL + 2 * r + 1);
        mds_layer();
    }
    full_rounds(HALF_FULL + N_PARTIAL, PT_FULL_SECOND);
    a.release();
    const int real = a.local(PT_IS_REAL);
    const int one = a.imm(1);
    const int t = a.sub(real, one);
    a.emit(a.mul(real, t));
    return a.instrs;
}

}  // namespace

extern "C" GlError gl_poseidon_table_program(GlGatePrograms *out) { return emit_table_program("gl_poseidon_table_program", poseidon_table_program, out); }
