// arithmetic_table.hip — the trace of the reference's arithmetic table (evm/src/arithmetic/, 92 columns) built on the device from a
// compact operation list: one row per ADD / MUL / SUB / LT / GT, two rows per DIV / MOD / ADDMOD / SUBMOD / MULMOD, zero rows
// behind them. The reference's snapshot derives one operation's cells (ArithmeticStark::generate) and has no generate_trace: the
// rows of the table are defined in include/plonky2_hip.h; the cells are the reference's bit for bit.
//
// The number of rows depends on the data. As in keccak_sponge_table.hip everything that decides it runs first: one thread per
// record checks its limits (the lowest record at fault per kind of fault with a vector atomicMin) and writes its row count,
// lookup.hip's scan turns the counts into exclusive prefix sums, the host reads 32 bytes — the call's one wait — and nothing has
// touched the trace by then. The fill is one lane per OPERATION — the witness of an operation is real arithmetic on its own
// operands and nothing of it is shared between lanes — and one lane per zero row behind the operations. A lane branches once, by
// operator family:
//   - carry (ADD, SUB, LT, GT): one 256-bit add or subtract in 32-bit limbs, whose 16-bit digits are those of the reference's
//     16-bit carry chains;
//   - MUL: pol_mul_lo's sixteen coefficients (136 products of 16-bit limbs), the carries, pol_remove_root_2exp;
//   - modular: the integer operation(in0, in1) as a magnitude of up to 512 bits and a sign, its division by the effective
//     modulus (at_divide), the floor correction of a negative input, out_aux_red, and the 31 values of
//     pol_remove_root_2exp(operation(a, b)(x) - c(x) - q(x) m(x)) in 64-bit integers.
// at_divide is Knuth's algorithm D on 32-bit limbs with FIXED trip counts: the divisor is moved to exactly eight limbs by
// conditional moves of 4, 2 and 1 limbs and a bit shift (the numerator follows and grows to 24 limbs), then sixteen quotient
// digits, each an estimate from the top two limbs of a nine-limb window, at most two corrections by Knuth's test against the
// divisor's second limb, an eight-limb multiply-subtract and a masked add-back. Every loop is unrolled and every array index is a
// constant, so the limbs stay in registers (the kernel's private segment is 0 bytes).
// tests/arithmetic_table_model.py is this division step for step, with its branches counted.
#include "arithmetic_table.h"

#include <algorithm>
#include <functional>
#include <string>

#include "ctx.h"
#include "lookup.h"
#include "program_asm.h"
#include "table_args.h"

namespace plonky2_hip {

namespace {

constexpr uint32_t T = ARITHMETIC_TABLE_THREADS;
constexpr uint32_t TF = ARITHMETIC_TABLE_FILL_THREADS;
constexpr uint32_t W = ARITHMETIC_TABLE_OP_WORDS;
constexpr uint32_t N16 = ARITHMETIC_TABLE_LIMBS;
constexpr uint64_t LOW32 = 0xFFFFFFFFull;
constexpr uint64_t GL_ORDER = 0xFFFFFFFF00000001ull;

uint32_t blocks_for(uint64_t count, uint32_t threads = T) { return (uint32_t)((count + threads - 1) / threads); }

// one thread per record, and one more for the last element of the scan
__global__ __launch_bounds__(T) void at_counts(const uint64_t *__restrict__ ops, uint32_t num_ops, uint64_t *__restrict__ op_rows,
                                               ArithmeticTableHeader *header) {
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    if (i > num_ops) return;
    if (i == num_ops) {
        op_rows[i] = 0;
        return;
    }
    const uint64_t *op = ops + (uint64_t)i * W;
    const uint64_t code = op[0];
    bool wide = false;
    uint64_t in1 = 0, in2 = 0;
#pragma unroll
    for (uint32_t c = 1; c < W; ++c) wide |= op[c] > LOW32;
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
        in1 |= op[9 + c];
        in2 |= op[17 + c];
    }
    const bool modular = code <= AT_IS_GT && at_is_modular((uint32_t)code);
    if (code > AT_IS_GT) atomicMin(&header->bad_operator, i);
    else if (wide) atomicMin(&header->bad_limb, i);
    else if (modular ? ((code == AT_IS_DIV || code == AT_IS_MOD) && in1 != 0) : in2 != 0) atomicMin(&header->bad_zero, i);
    op_rows[i] = modular ? 2 : 1;
}

__global__ __launch_bounds__(T) void at_total(const uint64_t *__restrict__ op_rows, uint32_t num_ops, ArithmeticTableHeader *header) {
    if (blockIdx.x == 0 && threadIdx.x == 0) header->rows = op_rows[num_ops];
}

// ---------------------------------------------------------------- the fill
// a signed value as the field element the reference's from_noncanonical_i64 gives: p - |v| below zero
__device__ __forceinline__ uint64_t at_canonical(int64_t v) { return v < 0 ? GL_ORDER - (uint64_t)(-v) : (uint64_t)v; }
// 16-bit limb k of a value in 32-bit limbs; k is a constant wherever this is called
template <uint32_t L>
__device__ __forceinline__ uint32_t at_limb16(const uint32_t (&x)[L], uint32_t k) {
    return (x[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
}
// the sixteen 16-bit limbs of x into columns col .. col + 15
__device__ __forceinline__ void at_store_value(uint64_t *__restrict__ out, uint64_t stride, uint32_t col, const uint32_t (&x)[8]) {
#pragma unroll
    for (uint32_t k = 0; k < N16; k++) out[(uint64_t)(col + k) * stride] = at_limb16(x, k);
}
__device__ __forceinline__ void at_store_zeros(uint64_t *__restrict__ out, uint64_t stride, uint32_t col, uint32_t count) {
#pragma unroll 16
    for (uint32_t k = 0; k < count; k++) out[(uint64_t)(col + k) * stride] = 0;
}

// x + y (subtract == false) or x - y in 32-bit limbs; returns the carry or the borrow out of limb L - 1
template <uint32_t L>
__device__ __forceinline__ uint32_t at_add_sub(const uint32_t (&x)[L], const uint32_t (&y)[L], bool subtract, uint32_t (&out)[L]) {
    uint32_t c = subtract ? 1u : 0u;  // x - y = x + ~y + 1
#pragma unroll
    for (uint32_t i = 0; i < L; i++) {
        const uint64_t s = (uint64_t)x[i] + (subtract ? ~y[i] : y[i]) + c;
        out[i] = (uint32_t)s;
        c = (uint32_t)(s >> 32);
    }
    return subtract ? 1u - c : c;
}

// the divisor (and the numerator with it) moved up by K limbs where its top K limbs are zero
template <int K>
__device__ __forceinline__ void at_shift_up(uint32_t (&d)[8], uint32_t (&n)[24], uint32_t &shift) {
    uint32_t top = 0;
#pragma unroll
    for (int i = 8 - K; i < 8; i++) top |= d[i];
    const bool z = top == 0;
#pragma unroll
    for (int i = 7; i >= 0; i--) d[i] = z ? (i >= K ? d[i - K] : 0u) : d[i];
#pragma unroll
    for (int i = 23; i >= 0; i--) n[i] = z ? (i >= K ? n[i - K] : 0u) : n[i];
    shift += z ? K : 0;
}

// num / div and num % div for num below 2^512 and div in 1 .. 2^256 - 1 (the head of this file; tests/arithmetic_table_model.py)
__device__ __forceinline__ void at_divide(const uint32_t (&num)[16], const uint32_t (&div)[8], uint32_t (&q)[16], uint32_t (&rem)[8]) {
    uint32_t d[8], n[24];
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = div[i];
#pragma unroll
    for (int i = 0; i < 24; i++) n[i] = i < 16 ? num[i] : 0u;
    uint32_t limb_shift = 0;
    at_shift_up<4>(d, n, limb_shift);
    at_shift_up<2>(d, n, limb_shift);
    at_shift_up<1>(d, n, limb_shift);
    const uint32_t bits = __clz(d[7]);  // d[7] != 0: the divisor is not zero
#pragma unroll
    for (int i = 7; i >= 1; i--) d[i] = __funnelshift_l(d[i - 1], d[i], bits);
    d[0] <<= bits;
#pragma unroll
    for (int i = 23; i >= 1; i--) n[i] = __funnelshift_l(n[i - 1], n[i], bits);
    n[0] <<= bits;

    uint32_t r[8];  // the running remainder: below d, because the quotient is below 2^512
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = n[16 + i];
#pragma unroll
    for (int j = 15; j >= 0; j--) {
        uint32_t w[9];  // the window r 2^32 + n[j], below d 2^32
        w[0] = n[j];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i + 1] = r[i];
        const uint64_t top = ((uint64_t)w[8] << 32) | w[7];
        uint64_t qhat = w[8] >= d[7] ? LOW32 : top / d[7];
        uint64_t rhat = top - qhat * d[7];
#pragma unroll
        for (int c = 0; c < 2; c++) {  // Knuth's test: the estimate is at most two too large before it, at most one after it
            const bool over = (rhat >> 32) == 0 && qhat * d[6] > ((rhat << 32) | w[6]);
            qhat -= over ? 1 : 0;
            rhat += over ? d[7] : 0;
        }
        uint32_t digit = (uint32_t)qhat;
        uint64_t carry = 0;
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {  // w -= digit * d
            const uint64_t p = (uint64_t)digit * d[i] + carry;
            carry = p >> 32;
            const uint64_t t = (uint64_t)w[i] - (uint32_t)p - borrow;
            w[i] = (uint32_t)t;
            borrow = (uint32_t)(t >> 32) & 1u;
        }
        const uint64_t t8 = (uint64_t)w[8] - carry - borrow;
        const bool back = (t8 >> 32) & 1u;  // the digit was one too large: add the divisor back
        digit -= back ? 1u : 0u;
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint64_t s = (uint64_t)w[i] + (back ? d[i] : 0u) + c;
            r[i] = (uint32_t)s;
            c = (uint32_t)(s >> 32);
        }
        q[j] = digit;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) rem[i] = __funnelshift_r(r[i], r[i + 1], bits);
    rem[7] = r[7] >> bits;
#pragma unroll
    for (int i = 0; i < 8; i++) rem[i] = (limb_shift & 4) ? (i + 4 < 8 ? rem[i + 4] : 0u) : rem[i];
#pragma unroll
    for (int i = 0; i < 8; i++) rem[i] = (limb_shift & 2) ? (i + 2 < 8 ? rem[i + 2] : 0u) : rem[i];
#pragma unroll
    for (int i = 0; i < 8; i++) rem[i] = (limb_shift & 1) ? (i + 1 < 8 ? rem[i + 1] : 0u) : rem[i];
}

// ADD, SUB, LT, GT: add::generate, sub::generate, compare::generate
__device__ __forceinline__ void at_carry_row(uint32_t op, const uint32_t (&a)[8], const uint32_t (&b)[8], uint64_t *__restrict__ out, uint64_t stride) {
    const bool swap = op == AT_IS_GT;  // GT: in1 - in0
    uint32_t x[8], y[8], s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        x[i] = swap ? b[i] : a[i];
        y[i] = swap ? a[i] : b[i];
    }
    const uint32_t br = at_add_sub<8>(x, y, op != AT_IS_ADD, s);
    const bool compare = op == AT_IS_LT || op == AT_IS_GT;
#pragma unroll
    for (uint32_t k = 0; k < N16; k++) {
        const uint32_t limb = at_limb16(s, k);
        out[(uint64_t)(AT_GENERAL_INPUT_2 + k) * stride] = compare ? (k == 0 ? br : 0u) : limb;
        out[(uint64_t)(AT_GENERAL_INPUT_3 + k) * stride] = compare ? limb : 0u;
    }
}

// MUL: mul::generate (mul.rs:69-100)
__device__ __forceinline__ void at_mul_row(const uint32_t (&a)[8], const uint32_t (&b)[8], uint64_t *__restrict__ out, uint64_t stride) {
    int64_t cy = 0, aux = 0;
#pragma unroll
    for (uint32_t d = 0; d < N16; d++) {
        uint64_t unreduced = 0;  // below 16 * 2^32
#pragma unroll
        for (uint32_t i = 0; i <= d; i++) unreduced += (uint64_t)(at_limb16(a, i) * at_limb16(b, d - i));
        const int64_t t = (int64_t)unreduced + cy;
        cy = t >> 16;
        const int64_t limb = t & 0xFFFF;
        out[(uint64_t)(AT_GENERAL_INPUT_2 + d) * stride] = (uint64_t)limb;
        const int64_t c = (int64_t)unreduced - limb;  // pol_remove_root_2exp of unreduced_prod - output
        aux = d == 0 ? -(c >> 16) : d < N16 - 1 ? (aux - c) >> 16 : -cy;
        out[(uint64_t)(AT_GENERAL_INPUT_3 + d) * stride] = at_canonical(aux);
    }
}

// DIV, MOD, ADDMOD, SUBMOD, MULMOD: generate_modular_op (modular.rs:193-287); `out` is the operation's first row
__device__ __forceinline__ void at_modular_rows(uint32_t op, const uint32_t (&a)[8], const uint32_t (&b)[8], const uint32_t (&m)[8],
                                                uint64_t *__restrict__ out, uint64_t stride) {
    // |operation(in0, in1)| and its sign
    uint32_t num[16];
    bool negative = false;
    if (op == AT_IS_MULMOD) {
#pragma unroll
        for (int k = 0; k < 16; k++) num[k] = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {  // schoolbook rows: a[i] * b[j] + num[i + j] + carry is below 2^64
            uint64_t carry = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint64_t t = (uint64_t)a[i] * b[j] + num[i + j] + carry;
                num[i + j] = (uint32_t)t;
                carry = t >> 32;
            }
            num[i + 8] = (uint32_t)carry;
        }
    } else {
        uint32_t s[8], t[8];
        const bool subtract = op == AT_IS_SUBMOD;
        const uint32_t c = at_add_sub<8>(a, b, subtract, s);  // ADDMOD: the carry is limb 8; SUBMOD: a borrow makes b - a the magnitude
        (void)at_add_sub<8>(b, a, true, t);
        negative = subtract && c;
        const bool first = op == AT_IS_MOD || op == AT_IS_DIV;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            num[i] = first ? a[i] : negative ? t[i] : s[i];
            num[8 + i] = 0;
        }
        num[8] = op == AT_IS_ADDMOD ? c : 0u;
    }

    // the effective modulus: 1 in place of zero (2^256 for DIV: the quotient is zero and the input is the remainder)
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) any |= m[i];
    const bool mod_is_zero = any == 0;
    const bool div_by_zero = mod_is_zero && op == AT_IS_DIV;
    uint32_t modulus[8];  // modulus_limbs of the witness: the zero of a DIV stays
#pragma unroll
    for (int i = 0; i < 8; i++) modulus[i] = m[i];
    modulus[0] |= (mod_is_zero && !div_by_zero) ? 1u : 0u;
    uint32_t divisor[8];
#pragma unroll
    for (int i = 0; i < 8; i++) divisor[i] = modulus[i];
    divisor[0] |= div_by_zero ? 1u : 0u;
    uint32_t quot[16], output[8];
    at_divide(num, divisor, quot, output);
    if (div_by_zero) {
#pragma unroll
        for (int i = 0; i < 16; i++) quot[i] = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) output[i] = num[i];
    }
    // floor division of a negative input: -(q + 1) and m - r where r is not zero
    uint32_t rest = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) rest |= output[i];
    const bool up = negative && rest != 0;
    uint32_t flipped[8];
    (void)at_add_sub<8>(modulus, output, true, flipped);
    uint32_t c = up ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint64_t s = (uint64_t)quot[i] + c;
        quot[i] = (uint32_t)s;
        c = (uint32_t)(s >> 32);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) output[i] = up ? flipped[i] : output[i];
    // out_aux_red = 2^256 + output - modulus, with 2^256 for the modulus of a DIV by zero
    uint32_t reduced[8];
    (void)at_add_sub<8>(output, modulus, true, reduced);

    at_store_value(out, stride, AT_GENERAL_INPUT_2, m);
    at_store_value(out, stride, AT_GENERAL_INPUT_3, output);
    uint64_t *next = out + 1;
    at_store_zeros(next, stride, 0, AT_NUM_FLAGS);
    next[(uint64_t)AT_MODULAR_MOD_IS_ZERO * stride] = mod_is_zero ? 1 : 0;
    at_store_value(next, stride, AT_MODULAR_OUT_AUX_RED, reduced);
    at_store_zeros(next, stride, AT_AUX_INPUT_0_LO, N16);
    const int32_t sign = negative ? -1 : 1;
#pragma unroll
    for (uint32_t k = 0; k < N16; k++) {
        out[(uint64_t)(AT_AUX_INPUT_0_LO + k) * stride] = at_canonical(sign * (int32_t)at_limb16(quot, k));
        next[(uint64_t)(AT_MODULAR_QUO_INPUT_HI + k) * stride] = at_canonical(sign * (int32_t)at_limb16(quot, N16 + k));
    }

    // aux = pol_remove_root_2exp(operation(a, b)(x) - c(x) - q(x) m(x)): 31 values, every coefficient below 2^37 in magnitude
    const bool is_mulmod = op == AT_IS_MULMOD;
    const int64_t b_sign = op == AT_IS_ADDMOD ? 1 : op == AT_IS_SUBMOD ? -1 : 0;
    int64_t aux = 0;
#pragma unroll
    for (uint32_t k = 0; k < 2 * N16 - 1; k++) {
        int64_t coeff = 0;
        if (k < N16) coeff = (int64_t)at_limb16(a, k) * (is_mulmod ? 0 : 1) + b_sign * (int64_t)at_limb16(b, k) - (int64_t)at_limb16(output, k);
        if (is_mulmod) {
            uint64_t prod = 0;
#pragma unroll
            for (uint32_t i = 0; i < N16; i++)
                if (k >= i && k - i < N16) prod += (uint64_t)(at_limb16(a, i) * at_limb16(b, k - i));
            coeff += (int64_t)prod;
        }
        uint64_t qm = 0;  // |q|(x) m(x), coefficient k
#pragma unroll
        for (uint32_t j = 0; j < N16; j++)
            if (k >= j) qm += (uint64_t)(at_limb16(quot, k - j) * at_limb16(modulus, j));
        coeff -= sign * (int64_t)qm;
        aux = k == 0 ? -(coeff >> 16) : (aux - coeff) >> 16;
        next[(uint64_t)(AT_MODULAR_AUX_INPUT + k) * stride] = at_canonical(aux);
    }
}

// One lane per operation: its one or two rows, all 92 columns
__global__ __launch_bounds__(TF) void arithmetic_table_ops_kernel(const uint64_t *__restrict__ ops, uint32_t num_ops, const uint64_t *__restrict__ op_rows,
                                                                  uint64_t *__restrict__ trace, uint64_t stride) {
    const uint32_t k = blockIdx.x * TF + threadIdx.x;
    if (k >= num_ops) return;
    const uint64_t *record = ops + (uint64_t)k * W;
    const uint32_t op = (uint32_t)record[0];
    uint32_t a[8], b[8], m[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        a[i] = (uint32_t)record[1 + i];
        b[i] = (uint32_t)record[9 + i];
        m[i] = (uint32_t)record[17 + i];
    }
    uint64_t *out = trace + op_rows[k];
#pragma unroll
    for (uint32_t f = 0; f < AT_NUM_FLAGS; f++) out[(uint64_t)f * stride] = op == f ? 1 : 0;
    at_store_value(out, stride, AT_GENERAL_INPUT_0, a);
    at_store_value(out, stride, AT_GENERAL_INPUT_1, b);
    if (at_is_modular(op)) {
        at_modular_rows(op, a, b, m, out, stride);
    } else {
        if (op == AT_IS_MUL) at_mul_row(a, b, out, stride);
        else at_carry_row(op, a, b, out, stride);
        at_store_zeros(out, stride, AT_AUX_INPUT_0_LO, N16);
    }
}

// One lane per row behind the operations: a zero row
__global__ __launch_bounds__(T) void arithmetic_table_zero_rows_kernel(uint64_t rows, uint64_t n, uint64_t *__restrict__ trace, uint64_t stride) {
    const uint64_t r = rows + (uint64_t)blockIdx.x * T + threadIdx.x;
    if (r >= n) return;
    at_store_zeros(trace + r, stride, 0, ARITHMETIC_TABLE_COLUMNS);
}

hipError_t enqueue_count(const uint64_t *d_ops, uint64_t num_ops, const ArithmeticTableScratch &s, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.header, 0xFF, 16, stream);
    if (e != hipSuccess) return e;
    at_counts<<<dim3(blocks_for(num_ops + 1)), dim3(T), 0, stream>>>(d_ops, (uint32_t)num_ops, s.op_rows, s.header);
    e = lookup_exclusive_sums(s.op_rows, num_ops + 1, s.totals, stream);
    if (e != hipSuccess) return e;
    at_total<<<dim3(1), dim3(T), 0, stream>>>(s.op_rows, (uint32_t)num_ops, s.header);
    return hipGetLastError();
}

bool fill_arguments_ok(const uint64_t *d_ops, uint64_t num_ops, uint64_t rows, uint32_t log_n, const uint64_t *d_trace, uint64_t trace_stride) {
    if (log_n == 0 || log_n > ARITHMETIC_TABLE_MAX_DEGREE_BITS || !d_trace || (num_ops && !d_ops)) return false;
    const uint64_t n = 1ull << log_n;
    return trace_stride >= n && rows <= n && rows >= num_ops && rows <= 2 * num_ops;
}

hipError_t enqueue_fill(const uint64_t *d_ops, uint64_t num_ops, uint64_t rows, uint64_t n, uint64_t *d_trace, uint64_t trace_stride,
                        const ArithmeticTableScratch &s, hipStream_t stream) {
    if (num_ops)
        arithmetic_table_ops_kernel<<<dim3(blocks_for(num_ops, TF)), dim3(TF), 0, stream>>>(d_ops, (uint32_t)num_ops, s.op_rows, d_trace, trace_stride);
    if (rows < n) arithmetic_table_zero_rows_kernel<<<dim3(blocks_for(n - rows)), dim3(T), 0, stream>>>(rows, n, d_trace, trace_stride);
    return hipGetLastError();
}

}  // namespace

ArithmeticTableScratch arithmetic_table_scratch_layout(void *base, uint64_t num_ops) {
    ArithmeticTableScratch s;
    uint64_t *words = static_cast<uint64_t *>(base);
    uint64_t at = sizeof(ArithmeticTableHeader) / 8;
    auto take = [&](uint64_t count) {
        uint64_t *p = words ? words + at : nullptr;
        at += count;
        return p;
    };
    s.header = reinterpret_cast<ArithmeticTableHeader *>(words);
    s.totals = take((num_ops + 1 + LOOKUP_SCAN_BLOCK - 1) / LOOKUP_SCAN_BLOCK);
    s.op_rows = take(num_ops + 1);
    s.words = (at + 1) & ~1ull;  // a multiple of 16 bytes
    return s;
}

hipError_t arithmetic_table_count(const uint64_t *d_ops, uint64_t num_ops, const ArithmeticTableScratch &s, ArithmeticTableHeader *h, hipStream_t stream) {
    if (!d_ops || !h || num_ops == 0 || num_ops > ARITHMETIC_TABLE_MAX_OPS) return hipErrorInvalidValue;
    hipError_t e = enqueue_count(d_ops, num_ops, s, stream);
    if (e != hipSuccess) return e;
    return read_status(h, s.header, sizeof(ArithmeticTableHeader), stream);
}

hipError_t arithmetic_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint64_t rows, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                 const ArithmeticTableScratch &s, hipStream_t stream) {
    if (!fill_arguments_ok(d_ops, num_ops, rows, log_n, d_trace, trace_stride)) return hipErrorInvalidValue;
    return enqueue_fill(d_ops, num_ops, rows, 1ull << log_n, d_trace, trace_stride, s, stream);
}

hipError_t arithmetic_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t log_n, uint64_t *d_trace, uint64_t trace_stride,
                                     const ArithmeticTableScratch &s, ArithmeticTableHeader *h, float *ms, hipStream_t stream) {
    if (!d_ops || !h || !ms || num_ops == 0 || num_ops > ARITHMETIC_TABLE_MAX_OPS) return hipErrorInvalidValue;
    StageClock<4> clock(stream);
    hipError_t e = clock.created;
    if (e == hipSuccess) e = clock.mark(0);
    if (e == hipSuccess) e = enqueue_count(d_ops, num_ops, s, stream);
    if (e == hipSuccess) e = clock.mark(1);
    if (e == hipSuccess) e = read_status(h, s.header, sizeof(ArithmeticTableHeader), stream);
    const bool fill = e == hipSuccess && h->bad_operator == AT_NONE && h->bad_limb == AT_NONE && h->bad_zero == AT_NONE &&
                      fill_arguments_ok(d_ops, num_ops, h->rows, log_n, d_trace, trace_stride);
    if (e == hipSuccess) e = clock.mark(2);
    if (fill && e == hipSuccess) e = enqueue_fill(d_ops, num_ops, h->rows, 1ull << log_n, d_trace, trace_stride, s, stream);
    if (e == hipSuccess) e = clock.mark(3);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = clock.elapsed(&ms[0], 0, 1);  // the wait for the header between the stages belongs to neither
    if (e == hipSuccess) e = clock.elapsed(&ms[1], 2, 3);
    return e;
}

}  // namespace plonky2_hip

using namespace plonky2_hip;

static_assert(GL_ARITHMETIC_TABLE_COLUMNS == ARITHMETIC_TABLE_COLUMNS && GL_ARITHMETIC_TABLE_OP_WORDS == ARITHMETIC_TABLE_OP_WORDS, "plonky2_hip.h");

static bool at_shape_ok(uint64_t num_ops, uint32_t degree_bits) {
    return num_ops <= ARITHMETIC_TABLE_MAX_OPS && degree_bits >= 1 && degree_bits <= ARITHMETIC_TABLE_MAX_DEGREE_BITS;
}

extern "C" uint64_t gl_arithmetic_table_scratch_bytes(uint64_t num_ops, uint32_t degree_bits) {
    if (!at_shape_ok(num_ops, degree_bits)) return 0;
    return arithmetic_table_scratch_layout(nullptr, num_ops).words * 8;
}

// what is refused before anything is launched; empty: nothing
static std::string at_trace_argument_error(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, const uint64_t *d_trace, uint64_t trace_stride,
                                           const void *d_scratch, const void *h_out, const void *ctx) {
    if (!ctx || (num_ops && !d_ops) || !d_scratch || !h_out) return "null pointer";
    if (num_ops > ARITHMETIC_TABLE_MAX_OPS) return "num_ops must be at most 2^22";
    std::string why = degree_bits_error(degree_bits, ARITHMETIC_TABLE_MAX_DEGREE_BITS);
    if (why.empty()) why = scratch_alignment_error(d_scratch);
    if (!why.empty()) return why;
    const uint64_t n = 1ull << degree_bits;
    const uint64_t scratch_bytes = arithmetic_table_scratch_layout(nullptr, num_ops).words * 8;
    const uint64_t ops_bytes = num_ops * ARITHMETIC_TABLE_OP_WORDS * 8;
    if (bytes_overlap(d_ops, ops_bytes, d_scratch, scratch_bytes)) return "d_scratch overlaps d_ops";
    if (d_trace) {
        why = trace_stride_error(trace_stride, n);
        if (!why.empty()) return why;
        const uint64_t bytes = trace_bytes(ARITHMETIC_TABLE_COLUMNS, trace_stride, n);
        if (bytes_overlap(d_trace, bytes, d_ops, ops_bytes)) return "d_trace overlaps d_ops";
        if (bytes_overlap(d_trace, bytes, d_scratch, scratch_bytes)) return "d_trace overlaps d_scratch";
    }
    return "";
}

// the refusals the device decided, read from the header: the lowest record at fault, whatever its fault; empty: nothing
static std::string at_data_error(const ArithmeticTableHeader &h) {
    const uint32_t lowest = std::min(h.bad_operator, std::min(h.bad_limb, h.bad_zero));
    if (lowest == AT_NONE) return "";
    const std::string record = "record " + std::to_string(lowest);
    if (lowest == h.bad_operator) return "the operator of " + record + " is not one of 0 .. 9 (SHL and SHR, 10 and 11, are not generated)";
    if (lowest == h.bad_limb) return "a limb of " + record + " is 2^32 or more";
    return "an input of " + record + " that must be zero is not (in2 of ADD, MUL, SUB, LT, GT; in1 of DIV, MOD)";
}

extern "C" GlError gl_arithmetic_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                             void *d_scratch, uint64_t *h_rows, void *ctx) {
    DeviceCall device_call(ctx);
    const std::string why = at_trace_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, h_rows, ctx);
    if (!why.empty()) return fail(GL_E_INVALID, "gl_arithmetic_table_trace: " + why);
    const ArithmeticTableScratch scratch = arithmetic_table_scratch_layout(d_scratch, num_ops);
    const uint64_t n = 1ull << degree_bits;
    *h_rows = 0;
    ArithmeticTableHeader h = {AT_NONE, AT_NONE, AT_NONE, 0, 0, 0};
    if (num_ops) {
        HIP_TRY(arithmetic_table_count(d_ops, num_ops, scratch, &h, S(ctx)->stream));
        const std::string bad = at_data_error(h);
        if (!bad.empty()) return fail(GL_E_INVALID, "gl_arithmetic_table_trace: " + bad);
        *h_rows = h.rows;
    }
    if (!d_trace) return ok();
    if (h.rows > n)
        return fail(GL_E_INVALID, "gl_arithmetic_table_trace: the operations take " + std::to_string(h.rows) +
                                      " rows, more than the 2^degree_bits rows of the trace");
    HIP_TRY(arithmetic_table_fill(d_ops, num_ops, h.rows, degree_bits, d_trace, trace_stride, scratch, S(ctx)->stream));
    return ok();
}

extern "C" GlError gl_debug_arithmetic_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                                      uint64_t trace_stride, void *d_scratch, float *h_ms, void *ctx) {
    DeviceCall device_call(ctx);
    std::string why = at_trace_argument_error(d_ops, num_ops, degree_bits, d_trace, trace_stride, d_scratch, h_ms, ctx);
    if (why.empty() && (!d_trace || !num_ops)) why = "null pointer";
    if (!why.empty()) return fail(GL_E_INVALID, "gl_debug_arithmetic_table_stage_ms: " + why);
    ArithmeticTableHeader h;
    HIP_TRY(arithmetic_table_stage_ms(d_ops, num_ops, degree_bits, d_trace, trace_stride, arithmetic_table_scratch_layout(d_scratch, num_ops), &h, h_ms,
                                      S(ctx)->stream));
    std::string bad = at_data_error(h);
    if (bad.empty() && h.rows > (1ull << degree_bits)) bad = "the rows do not fit the trace";
    if (!bad.empty()) return fail(GL_E_INVALID, "gl_debug_arithmetic_table_stage_ms: nothing was filled: " + bad);
    return ok();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The constraints of the reference's arithmetic table (arithmetic_stark.rs:72-87: add, sub, mul, compare and
// modular::eval_packed_generic) as ONE STARK program: plonky2_gpu_amd/arithmetic_table.py program(), call for call
// (tests/test_arithmetic_table_ref.py holds the two against each other word for word). Host code; the columns are
// arithmetic_table.h's.
namespace {

using namespace plonky2_hip::program_asm;

typedef std::function<int(int)> Limb;     // limb i in a fresh register, consumed by whoever asked
typedef std::function<void(int)> Emit;

constexpr int LIMB_BITS = 16;
constexpr int NL = (int)ARITHMETIC_TABLE_LIMBS;

// eval_packed_generic_are_equal (add.rs:33-62); returns the register of the last carry
int are_equal(StarkAsm &a, int is_op, const Limb &larger, const Limb &smaller, const Emit &emit) {
    const int overflow = a.imm((u128)1 << LIMB_BITS);
    const int overflow_inv = a.imm((u128)glh::inv(1ull << LIMB_BITS));
    int cy = -1;
    for (int i = 0; i < NL; i++) {
        const int t = larger(i);
        const int s = smaller(i);
        if (cy >= 0) {
            a.add(t, cy, t);
            a.free1(cy);
        }
        a.sub(t, s, t);
        a.free1(s);
        const int u = a.sub(overflow, t);
        a.mul(u, t, u);
        a.mul(u, is_op, u);
        emit(u);
        a.free1(u);
        a.mul(t, overflow_inv, t);
        cy = t;
    }
    a.free({overflow, overflow_inv});
    return cy;
}

// i -> local(c0 + i) + or - local(c1 + i)
Limb pair(StarkAsm &a, bool subtract, int c0, int c1) {
    return [&a, subtract, c0, c1](int i) {
        const int x = a.local(c0 + i);
        const int y = a.local(c1 + i);
        if (subtract) a.sub(x, y, x);
        else a.add(x, y, x);
        a.free1(y);
        return x;
    };
}

// sum over i + j = d of left(i) * right(j); -1 where the sum is empty
int conv(StarkAsm &a, int d, const Limb &left, int num_left, const Limb &right, int num_right) {
    int total = -1;
    for (int i = std::max(0, d - num_right + 1); i <= std::min(d, num_left - 1); i++) {
        const int x = left(i);
        const int y = right(d - i);
        a.mul(x, y, x);
        a.free1(y);
        if (total < 0) {
            total = x;
        } else {
            a.add(total, x, total);
            a.free1(x);
        }
    }
    return total;
}

// eval_packed_generic_lt (compare.rs:53-81)
void less_than(StarkAsm &a, int is_op, const Limb &in0, const Limb &in1, const Limb &aux, const std::function<int()> &output, const Emit &emit) {
    const Limb lhs = [&](int i) {
        const int x = in0(i);
        const int y = in1(i);
        a.sub(x, y, x);
        a.free1(y);
        return x;
    };
    const int cy = are_equal(a, is_op, aux, lhs, emit);
    const int out = output();
    a.sub(cy, out, cy);
    a.free1(out);
    a.mul(cy, is_op, cy);
    emit(cy);
    a.free1(cy);
}

Program arithmetic_table_program(ImmediatePool &pool) {
    StarkAsm a(&pool);
    const auto local_col = [&a](int c) -> Limb { return [&a, c](int i) { return a.local(c + i); }; };
    const auto next_col = [&a](int c) -> Limb { return [&a, c](int i) { return a.next(c + i); }; };
    const Limb in0 = local_col(AT_GENERAL_INPUT_0), in1 = local_col(AT_GENERAL_INPUT_1), in2 = local_col(AT_GENERAL_INPUT_2),
               in3 = local_col(AT_GENERAL_INPUT_3);
    const Emit plain = [&a](int r) { a.emit(r); };
    const Emit transition = [&a](int r) { a.emit_transition(r); };

    // add.rs:116-140: in0 + in1 against the output
    a.release();
    int flag = a.local(AT_IS_ADD);
    a.free1(are_equal(a, flag, pair(a, false, AT_GENERAL_INPUT_0, AT_GENERAL_INPUT_1), in2, plain));
    // sub.rs:40-62: the output against in0 - in1
    a.release();
    flag = a.local(AT_IS_SUB);
    a.free1(are_equal(a, flag, in2, pair(a, true, AT_GENERAL_INPUT_0, AT_GENERAL_INPUT_1), plain));
    // mul.rs:102-146: a(x) b(x) - c(x) - (x - 2^16) s(x), the sixteen low coefficients
    a.release();
    flag = a.local(AT_IS_MUL);
    for (int d = 0; d < NL; d++) {
        const int c = conv(a, d, in0, NL, in1, NL);
        int t = a.local(AT_GENERAL_INPUT_2 + d);
        a.sub(c, t, c);
        a.free1(t);
        t = a.local(AT_GENERAL_INPUT_3 + d);  // pol_adjoin_root: s[d - 1] - 2^16 s[d]
        a.mulk(t, LIMB_BITS, t);
        a.add(c, t, c);
        a.free1(t);
        if (d) {
            t = a.local(AT_GENERAL_INPUT_3 + d - 1);
            a.sub(c, t, c);
            a.free1(t);
        }
        a.mul(c, flag, c);
        a.emit(c);
        a.free1(c);
    }
    // compare.rs:83-104
    a.release();
    const int is_lt = a.local(AT_IS_LT);
    const int is_gt = a.local(AT_IS_GT);
    {
        const int t = a.add(is_lt, is_gt);
        const int out = a.local(AT_GENERAL_INPUT_2);
        a.mul(t, out, t);
        const int one = a.imm(1);
        a.sub(out, one, out);
        a.mul(t, out, t);
        a.emit(t);
        a.free({t, out, one});
    }
    const std::function<int()> output = [&a]() { return a.local(AT_GENERAL_INPUT_2); };
    less_than(a, is_lt, in0, in1, in3, output, plain);
    less_than(a, is_gt, in1, in0, in3, output, plain);

    // modular.rs:407-459
    a.release();
    const int flt = a.local(AT_IS_ADDMOD);
    for (int f : {AT_IS_MULMOD, AT_IS_MOD, AT_IS_SUBMOD, AT_IS_DIV}) {
        const int t = a.local(f);
        a.add(flt, t, flt);
        a.free1(t);
    }
    a.emit_last_row(flt);
    // modular_constr_poly (:316-404)
    const int miz = a.next(AT_MODULAR_MOD_IS_ZERO);
    {
        const int t = a.mul(miz, miz);
        a.sub(t, miz, t);
        a.mul(t, flt, t);
        a.emit_transition(t);
        a.free1(t);
    }
    {
        const int t = a.local(AT_GENERAL_INPUT_2);
        for (int i = 1; i < NL; i++) {
            const int u = a.local(AT_GENERAL_INPUT_2 + i);
            a.add(t, u, t);
            a.free1(u);
        }
        a.mul(t, flt, t);
        a.mul(t, miz, t);
        a.emit_transition(t);
        a.free1(t);
    }
    const int is_div = a.local(AT_IS_DIV);
    const int zd = a.mul(miz, is_div);  // mod_is_zero * lv[IS_DIV]
    a.free1(is_div);
    const Limb modulus = [&a, miz](int i) {  // modulus[0] += mod_is_zero
        const int r = a.local(AT_GENERAL_INPUT_2 + i);
        if (i == 0) a.add(r, miz, r);
        return r;
    };
    const Limb reduced = [&a, zd, &modulus](int i) {  // output - modulus, with output[0] += mod_is_zero * lv[IS_DIV]
        const int x = a.local(AT_GENERAL_INPUT_3 + i);
        if (i == 0) a.add(x, zd, x);
        const int y = modulus(i);
        a.sub(x, y, x);
        a.free1(y);
        return x;
    };
    {
        const int cy = are_equal(a, flt, next_col(AT_MODULAR_OUT_AUX_RED), reduced, transition);
        const int t = a.imm(1);  // is_less_than = 1 - mod_is_zero * lv[IS_DIV]
        a.sub(t, zd, t);
        a.sub(cy, t, cy);
        a.free1(t);
        a.mul(cy, flt, cy);
        a.emit_transition(cy);
        a.free({cy, zd});
    }
    const Limb quot = [&a](int i) { return i < NL ? a.local(AT_AUX_INPUT_0_LO + i) : a.next(AT_MODULAR_QUO_INPUT_HI + i - NL); };
    // the higher order terms of q(x) m(x) must be zero
    for (int d = 2 * NL; d < 3 * NL - 1; d++) {
        const int t = conv(a, d, quot, 2 * NL, modulus, NL);
        a.mul(t, flt, t);
        a.emit_transition(t);
        a.free1(t);
    }
    a.free1(flt);
    // constr_poly = c(x) + q(x) m(x) + (x - 2^16) s(x): 32 registers
    int constr[2 * NL];
    for (int d = 0; d < 2 * NL; d++) {
        const int c = conv(a, d, quot, 2 * NL, modulus, NL);
        if (d < NL) {
            const int t = a.local(AT_GENERAL_INPUT_3 + d);
            a.add(c, t, c);
            a.free1(t);
        }
        if (d < 2 * NL - 1) {
            const int t = a.next(AT_MODULAR_AUX_INPUT + d);
            a.mulk(t, LIMB_BITS, t);
            a.sub(c, t, c);
            a.free1(t);
        }
        if (d) {
            const int t = a.next(AT_MODULAR_AUX_INPUT + d - 1);
            a.add(c, t, c);
            a.free1(t);
        }
        constr[d] = c;
    }
    a.free1(miz);
    // the four operations' inputs against it, each under its own filter
    const Limb add_input = pair(a, false, AT_GENERAL_INPUT_0, AT_GENERAL_INPUT_1), sub_input = pair(a, true, AT_GENERAL_INPUT_0, AT_GENERAL_INPUT_1);
    struct Input {
        std::vector<int> flags;
        Limb operation;  // -1: the coefficient is zero
    };
    const Input inputs[4] = {
        {{AT_IS_ADDMOD}, [&](int d) { return d < NL ? add_input(d) : -1; }},
        {{AT_IS_SUBMOD}, [&](int d) { return d < NL ? sub_input(d) : -1; }},
        {{AT_IS_MULMOD}, [&](int d) { return conv(a, d, in0, NL, in1, NL); }},
        {{AT_IS_MOD, AT_IS_DIV}, [&](int d) { return d < NL ? in0(d) : -1; }},
    };
    for (const Input &input : inputs) {
        const int f = a.local(input.flags[0]);
        for (size_t k = 1; k < input.flags.size(); k++) {
            const int t = a.local(input.flags[k]);
            a.add(f, t, f);
            a.free1(t);
        }
        for (int d = 0; d < 2 * NL; d++) {
            int t = input.operation(d);
            if (t < 0) {
                t = a.mul(constr[d], f);
            } else {
                a.sub(constr[d], t, t);
                a.mul(t, f, t);
            }
            a.emit_transition(t);
            a.free1(t);
        }
        a.free1(f);
    }
    return a.instrs;
}

}  // namespace

extern "C" GlError gl_arithmetic_table_program(GlGatePrograms *out) {
    return emit_table_program("gl_arithmetic_table_program", arithmetic_table_program, out);
}
