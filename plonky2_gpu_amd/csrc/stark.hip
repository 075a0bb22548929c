// stark.hip — the data-parallel parts of starky's prove() (starky/src/prover.rs:32-195) on the device:
//   (1) the permutation Z polynomials   compute_permutation_z_polys (starky/src/permutation.rs:66-118) over the batches of
//                                        get_permutation_batches (:229-250)
//   (2) the constraint quotient values   compute_quotient_polys (prover.rs:199-319) over eval_vanishing_poly
//                                        (vanishing_poly.rs:16-41) = the STARK's own constraints, then eval_permutation_checks
//                                        (permutation.rs:263-323), all through starky's ConstraintConsumer (constraint_consumer.rs:53-76)
// The STARK's constraints (Stark::eval_packed_generic) are ONE register program in device memory, interpreted per point: the
// GlGateInstr encoding of the gate programs (plonk.hip) with two rows to load from — LOAD_WIRE reads local_values, LOAD_NEXT
// next_values — the public inputs themselves behind LOAD_PI, and four ways to emit (plain, transition, first row, last row).
// All lanes of a wavefront run the same instruction stream, so the interpreter does not diverge.
//
// The consumer is not plonk's reduce_with_powers: for every challenge acc <- acc * alpha + constraint in emission order, so a
// point keeps num_challenges running sums whatever the number of constraints.
//
// (2) is one thread per LEAF t of the quotient domain, as in plonk.hip: point i = reverse_bits(t) of the domain of size
// n << qdb sits at LDE index i * step, whose row is reverse_bits(i * step, degree_bits + rate_bits) = t. Consecutive threads read
// consecutive rows of every column of the column-major LDE; the next row (point i + 2^qdb, wrapping at the end of the domain)
// is row reverse_bits(i + 2^qdb) of the same columns; only the 8-byte results are scattered.
#include "stark.h"

#include "gl_field.h"
#include "plonk_device.h"

namespace plonky2_hip {

namespace {

constexpr int SP_MAX_REGS = 64;
enum : uint16_t {
    SP_LOAD_WIRE,
    SP_LOAD_CONST,  // invalid in a STARK program
    SP_LOAD_PI,
    SP_LOAD_IMM,
    SP_ADD,
    SP_SUB,
    SP_MUL,
    SP_EMIT,
    SP_MULK,
    SP_ACC,
    SP_ACCR,
    SP_LOAD_NEXT,
    SP_EMIT_TRANSITION,
    SP_EMIT_FIRST_ROW,
    SP_EMIT_LAST_ROW
};

struct PermChallenges {  // [set][challenge]
    uint64_t beta[STARK_MAX_QDF * STARK_MAX_CHALLENGES], gamma[STARK_MAX_QDF * STARK_MAX_CHALLENGES];
};

// The two products of batch b at one row (permutation.rs:97-103, 299-320): over the instances f = b * qdf + k of the batch,
// instance f = (pair f / num_challenges, challenge f % num_challenges) with the challenges of SET k, the reduced values
// gamma + sum_j beta^j row[col_j] of the pair's left and right columns. `row` points at the row's element of column 0.
__device__ __forceinline__ void batch_products(const StarkPairsDev &pairs, const PermChallenges &ch, uint32_t num_challenges, uint32_t qdf,
                                               uint32_t b, const uint64_t *row, uint64_t stride, uint64_t &lhs, uint64_t &rhs) {
    lhs = rhs = 1;
    const uint32_t instances = pairs.num_pairs * num_challenges;
    for (uint32_t k = 0; k < qdf; k++) {
        const uint32_t f = b * qdf + k;
        if (f >= instances) break;  // the last batch may be short
        const uint32_t pair = f / num_challenges, c = f % num_challenges;
        const uint64_t beta = ch.beta[k * num_challenges + c], gamma = ch.gamma[k * num_challenges + c];
        uint64_t l = 0, r = 0;
        for (uint32_t j = pairs.pair_bounds[pair + 1]; j-- > pairs.pair_bounds[pair];) {  // Horner from the last column pair
            l = gl::mac(row[pairs.column_pairs[2 * j] * stride], l, beta);
            r = gl::mac(row[pairs.column_pairs[2 * j + 1] * stride], r, beta);
        }
        lhs = gl::mul(lhs, gl::add(l, gamma));
        rhs = gl::mul(rhs, gl::add(r, gamma));
    }
}

struct CtlChallenges {  // [challenge]
    uint64_t beta[STARK_MAX_CHALLENGES], gamma[STARK_MAX_CHALLENGES];
};

// Column::eval (cross_table_lookup.rs:100-119) of CTL column k at one row; `row` points at the row's element of column 0. The
// descriptors are read at wave-uniform addresses.
__device__ __forceinline__ uint64_t ctl_column(const StarkCtlDev &d, uint32_t k, const uint64_t *row, uint64_t stride) {
    uint64_t v = d.column_constants[k];
    for (uint32_t j = d.column_bounds[k]; j < d.column_bounds[k + 1]; j++) v = gl::mac(v, row[d.term_columns[j] * stride], d.term_coeffs[j]);
    return v;
}

// GrandProductChallenge::combine (evm/src/permutation.rs:61-73) over the columns of TWC t: gamma + sum_j beta^j column_j
__device__ __forceinline__ uint64_t ctl_combine(const StarkCtlDev &d, uint32_t t, uint64_t beta, uint64_t gamma, const uint64_t *row, uint64_t stride) {
    uint64_t acc = 0;
    for (uint32_t k = d.twc_column_bounds[t + 1]; k-- > d.twc_column_bounds[t];) acc = gl::add(gl::mul(acc, beta), ctl_column(d, k, row, stride));
    return gl::add(acc, gamma);
}

// challenge c of at most four, without indexing the kernel parameters by a register
__device__ __forceinline__ void ctl_challenge(const CtlChallenges &ch, uint32_t c, uint64_t &beta, uint64_t &gamma) {
    beta = ch.beta[0], gamma = ch.gamma[0];
#pragma unroll
    for (uint32_t e = 1; e < STARK_MAX_CHALLENGES; e++) {
        beta = c == e ? ch.beta[e] : beta;
        gamma = c == e ? ch.gamma[e] : gamma;
    }
}

// the factor s_r of CTL Z number z at one row (partial_products, cross_table_lookup.rs:323-337): the filter is compared as a field
// element; one that is neither 0 nor 1 raises *flag
__device__ __forceinline__ uint64_t ctl_factor(const StarkCtlDev &d, const CtlChallenges &ch, uint32_t z, const uint64_t *row, uint64_t stride,
                                               uint64_t *flag) {
    const uint32_t t = d.zs[2 * z], filter = d.twc_filter[t];
    uint64_t f = 1;
    if (filter != STARK_CTL_NO_FILTER) f = gl::canon(ctl_column(d, filter, row, stride));
    if (f > 1 && flag) *flag = 1;
    if (f != 1) return 1;
    uint64_t beta, gamma;
    ctl_challenge(ch, d.zs[2 * z + 1], beta, gamma);
    return ctl_combine(d, t, beta, gamma, row, stride);
}

// One thread per (row i, CTL Z z): the row's factor into the Z slot; the prefix product over the rows follows.
__global__ __launch_bounds__(256) void stark_ctl_factors_kernel(const uint64_t *__restrict__ trace, uint64_t trace_stride, StarkCtlDev ctl,
                                                                CtlChallenges ch, uint32_t log_n, uint64_t *__restrict__ out, uint64_t *flag) {
    const uint64_t n = 1ull << log_n;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * ctl.num_zs) return;
    out[g] = gl::canon(ctl_factor(ctl, ch, (uint32_t)(g >> log_n), trace + (g & (n - 1)), trace_stride, flag));
}

// The scan is exclusive and the CTL Zs are inclusive: Z[i] = (product of the earlier blocks) * (product of the block's earlier
// rows) * s_i, with s_i evaluated once more (the scan overwrote it).
__global__ __launch_bounds__(256) void stark_ctl_finalize_kernel(const uint64_t *__restrict__ trace, uint64_t trace_stride, StarkCtlDev ctl,
                                                                 CtlChallenges ch, uint32_t log_n, uint64_t *out, const uint64_t *totals,
                                                                 uint64_t totals_stride) {
    const uint64_t n = 1ull << log_n;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * ctl.num_zs) return;
    const uint64_t i = g & (n - 1);
    const uint32_t z = (uint32_t)(g >> log_n);
    const uint64_t s = ctl_factor(ctl, ch, z, trace + i, trace_stride, nullptr);
    out[g] = gl::canon(gl::mul(gl::mul(out[g], totals[(uint64_t)z * totals_stride + i / SCAN_B]), s));
}

// One thread per (row i, Z polynomial b): the row's quotient numerator / denominator into the Z slot; the exclusive prefix
// product over the rows follows (plonk_device.h). A zero denominator (the reference's batch inversion asserts) gives quotient 0.
__global__ __launch_bounds__(256) void stark_perm_quotients_kernel(const uint64_t *__restrict__ trace, uint64_t trace_stride, StarkPairsDev pairs,
                                                                   PermChallenges ch, uint32_t num_challenges, uint32_t qdf, uint32_t num_zs,
                                                                   uint32_t log_n, uint64_t *__restrict__ out) {
    const uint64_t n = 1ull << log_n;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * num_zs) return;
    const uint64_t i = g & (n - 1);
    const uint32_t b = (uint32_t)(g >> log_n);
    uint64_t lhs, rhs;
    batch_products(pairs, ch, num_challenges, qdf, b, trace + i, trace_stride, lhs, rhs);
    out[(uint64_t)b * n + i] = gl::canon(gl::mul(lhs, inverse_chain(rhs)));
}

// Z[i] = (product of the earlier blocks) * (product of the block's earlier rows)
__global__ __launch_bounds__(256) void stark_perm_finalize_kernel(uint64_t *out, const uint64_t *totals, uint64_t totals_stride, uint32_t num_zs,
                                                                  uint32_t log_n) {
    const uint64_t n = 1ull << log_n;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * num_zs) return;
    const uint64_t i = g & (n - 1);
    const uint32_t b = (uint32_t)(g >> log_n);
    out[g] = gl::canon(gl::mul(out[g], totals[(uint64_t)b * totals_stride + i / SCAN_B]));
}

struct StarkQuotientParams {
    const uint16_t *instrs;
    const uint64_t *imms, *pis, *trace, *zs, *twl, *twh;
    uint64_t *out;
    uint64_t stride;
    StarkPairsDev pairs;
    uint32_t num_instrs, num_zs, num_challenges, qdf, degree_bits, qdb;
    uint64_t shift, g_inv;  // the coset shift; 1 / g = the last element of the subgroup
    uint64_t alpha[STARK_MAX_CHALLENGES];
    uint64_t zh[16], zh_inv[16];  // Z_H on the coset takes 2^qdb values (field/src/zero_poly_coset.rs:20-41)
    PermChallenges ch;
    StarkCtlDev ctl;  // num_zs = 0 without cross-table lookups
    CtlChallenges ctl_ch;
};

__global__ __launch_bounds__(128) void stark_quotient_values_kernel(const StarkQuotientParams p) {
    const uint32_t log_size = p.degree_bits + p.qdb;
    const uint64_t size = 1ull << log_size, n = 1ull << p.degree_bits;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= size) return;
    const uint64_t i = log_size ? (__brevll(t) >> (64 - log_size)) : 0;
    const uint64_t i_next = (i + (1ull << p.qdb)) & (size - 1);  // next_step points on, wrapping (prover.rs:262)
    const uint64_t t_next = log_size ? (__brevll(i_next) >> (64 - log_size)) : 0;
    const uint64_t *local = p.trace + t, *next = p.trace + t_next;

    const uint64_t x = gl::mul(p.shift, root_pow(p.twl, p.twh, log_size, i));
    uint64_t zh = p.zh[0], zh_inv = p.zh_inv[0];
    const uint32_t which = (uint32_t)i & ((1u << p.qdb) - 1);
    for (uint32_t e = 1; e < (1u << p.qdb); e++) {
        zh = which == e ? p.zh[e] : zh;
        zh_inv = which == e ? p.zh_inv[e] : zh_inv;
    }
    // ConstraintConsumer::new (prover.rs:266-275): z_last = x - g^(n-1); the two Lagrange selectors in closed form,
    // L_k(x) = g^k Z_H(x) / (n (x - g^k)) for k = 0 and k = n - 1 (g^(n-1) = 1 / g) — the values the reference gets by LDE of the
    // selector columns. x lies on the coset, never in the subgroup: both denominators are non-zero and one inversion serves both.
    const uint64_t z_last = gl::sub(x, p.g_inv);
    const uint64_t d_first = gl::mul(n, gl::sub(x, 1)), d_last = gl::mul(n, z_last);
    const uint64_t d_inv = inverse_chain(gl::mul(d_first, d_last));
    const uint64_t l_first = gl::mul(zh, gl::mul(d_inv, d_last));
    const uint64_t l_last = gl::mul(gl::mul(p.g_inv, zh), gl::mul(d_inv, d_first));

    uint64_t sums[STARK_MAX_CHALLENGES] = {0, 0, 0, 0};
    auto constraint = [&](uint64_t v) {  // ConstraintConsumer::constraint (constraint_consumer.rs:59-64)
#pragma unroll
        for (uint32_t c = 0; c < STARK_MAX_CHALLENGES; c++)
            if (c < p.num_challenges) sums[c] = gl::mac(v, sums[c], p.alpha[c]);
    };

    uint64_t regs[SP_MAX_REGS];
    uint64_t acc_lo[4] = {0, 0, 0, 0}, acc_hi[4] = {0, 0, 0, 0};  // ACC: plain (wrapping-free by contract) sums of the 32-bit halves
    for (uint32_t pc = 0; pc < p.num_instrs; pc++) {
        const uint16_t *in = p.instrs + 4 * pc;
        const uint16_t op = in[0], dst = in[1] & (SP_MAX_REGS - 1), a = in[2], b = in[3];
        switch (op) {
            case SP_LOAD_WIRE: regs[dst] = local[a * p.stride]; break;
            case SP_LOAD_NEXT: regs[dst] = next[a * p.stride]; break;
            case SP_LOAD_PI: regs[dst] = p.pis[a]; break;
            case SP_LOAD_IMM: regs[dst] = p.imms[a]; break;
            case SP_ADD: regs[dst] = gl::add(regs[a & (SP_MAX_REGS - 1)], regs[b & (SP_MAX_REGS - 1)]); break;
            case SP_SUB: regs[dst] = gl::sub(regs[a & (SP_MAX_REGS - 1)], regs[b & (SP_MAX_REGS - 1)]); break;
            case SP_MUL: regs[dst] = gl::mul(regs[a & (SP_MAX_REGS - 1)], regs[b & (SP_MAX_REGS - 1)]); break;
            case SP_MULK: regs[dst] = gl::mul(regs[a & (SP_MAX_REGS - 1)], 1ull << (b & 63)); break;
            case SP_ACC: {
                const uint64_t k = p.imms[b];
                acc_lo[dst & 3] += (regs[a & (SP_MAX_REGS - 1)] & 0xFFFFFFFFull) * k;
                acc_hi[dst & 3] += (regs[a & (SP_MAX_REGS - 1)] >> 32) * k;
                break;
            }
            case SP_ACCR:
                regs[dst] = gl::fold96(acc_lo[a & 3], acc_hi[a & 3]);
                acc_lo[a & 3] = acc_hi[a & 3] = 0;
                break;
            case SP_EMIT: constraint(regs[a & (SP_MAX_REGS - 1)]); break;
            case SP_EMIT_TRANSITION: constraint(gl::mul(regs[a & (SP_MAX_REGS - 1)], z_last)); break;
            case SP_EMIT_FIRST_ROW: constraint(gl::mul(regs[a & (SP_MAX_REGS - 1)], l_first)); break;
            case SP_EMIT_LAST_ROW: constraint(gl::mul(regs[a & (SP_MAX_REGS - 1)], l_last)); break;
            default: break;  // refused by stark_program_validate
        }
    }
    // eval_permutation_checks (permutation.rs:284-322): Z(1) = 1 for every Z, then per batch Z(g x) prod rhs = Z(x) prod lhs
    for (uint32_t z = 0; z < p.num_zs; z++) constraint(gl::mul(gl::sub(p.zs[z * p.stride + t], 1), l_first));
    for (uint32_t z = 0; z < p.num_zs; z++) {
        uint64_t lhs, rhs;
        batch_products(p.pairs, p.ch, p.num_challenges, p.qdf, z, local, p.stride, lhs, rhs);
        constraint(gl::sub(gl::mul(p.zs[z * p.stride + t_next], rhs), gl::mul(p.zs[z * p.stride + t], lhs)));
    }
    // eval_cross_table_lookup_checks (evm/src/cross_table_lookup.rs:421-450), the CTL Zs behind the permutation Zs: with
    // select(f, x) = f x + 1 - f, Z(1) = select(filter, combine) on the first row and Z(g x) = Z(x) select(filter', combine') on
    // every row but the last
    for (uint32_t z = 0; z < p.ctl.num_zs; z++) {
        const uint32_t tw = p.ctl.zs[2 * z], filter = p.ctl.twc_filter[tw];
        uint64_t beta, gamma;
        ctl_challenge(p.ctl_ch, p.ctl.zs[2 * z + 1], beta, gamma);
        uint64_t sel_local = ctl_combine(p.ctl, tw, beta, gamma, local, p.stride), sel_next = ctl_combine(p.ctl, tw, beta, gamma, next, p.stride);
        if (filter != STARK_CTL_NO_FILTER) {
            const uint64_t f_local = ctl_column(p.ctl, filter, local, p.stride), f_next = ctl_column(p.ctl, filter, next, p.stride);
            sel_local = gl::sub(gl::mac(1, f_local, sel_local), f_local);
            sel_next = gl::sub(gl::mac(1, f_next, sel_next), f_next);
        }
        const uint64_t z_local = p.zs[(p.num_zs + z) * p.stride + t], z_next = p.zs[(p.num_zs + z) * p.stride + t_next];
        constraint(gl::mul(gl::sub(z_local, sel_local), l_first));
        constraint(gl::mul(gl::sub(z_next, gl::mul(z_local, sel_next)), z_last));
    }
#pragma unroll
    for (uint32_t c = 0; c < STARK_MAX_CHALLENGES; c++)
        if (c < p.num_challenges) p.out[(uint64_t)c * size + i] = gl::canon(gl::mul(sums[c], zh_inv));  // prover.rs:296-302
}

unsigned grid_for(uint64_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

bool load_challenges(PermChallenges *ch, const uint64_t *h_challenges, uint32_t num_challenges, uint32_t qdf) {
    if (num_challenges == 0 || num_challenges > STARK_MAX_CHALLENGES || qdf == 0 || qdf > STARK_MAX_QDF) return false;
    for (uint32_t k = 0; k < qdf * num_challenges; k++) {
        ch->beta[k] = h_challenges[2 * k] % glh::P;
        ch->gamma[k] = h_challenges[2 * k + 1] % glh::P;
    }
    return true;
}

bool load_ctl_challenges(CtlChallenges *ch, const uint64_t *h_challenges, uint32_t num_challenges) {
    if (!h_challenges || num_challenges == 0 || num_challenges > STARK_MAX_CHALLENGES) return false;
    for (uint32_t c = 0; c < num_challenges; c++) {
        ch->beta[c] = h_challenges[2 * c] % glh::P;
        ch->gamma[c] = h_challenges[2 * c + 1] % glh::P;
    }
    return true;
}

}  // namespace

bool stark_program_validate(const uint16_t *instrs, uint32_t num_instrs, const uint64_t *imms, uint32_t num_imms, uint32_t num_columns,
                            uint32_t num_public_inputs, std::string *error) {
    bool written[SP_MAX_REGS] = {};
    unsigned __int128 acc_bound[4] = {0, 0, 0, 0};  // 128 bits as in gate_jit.hip: two weights near 2^32 pass 2^64
    bool acc_used[4] = {false, false, false, false};
    uint32_t emitted = 0;
    auto bad = [&](uint32_t pc, const std::string &what) {
        *error = "STARK program, instruction " + std::to_string(pc) + ": " + what;
        return false;
    };
    for (uint32_t pc = 0; pc < num_instrs; pc++) {
        const uint16_t op = instrs[4 * pc], dst = instrs[4 * pc + 1], a = instrs[4 * pc + 2], b = instrs[4 * pc + 3];
        if (op == SP_LOAD_CONST) return bad(pc, "LOAD_CONST: a STARK has no constants columns");
        if (op > SP_EMIT_LAST_ROW) return bad(pc, "unknown opcode");
        const bool is_emit = op == SP_EMIT || op >= SP_EMIT_TRANSITION;
        const bool reads_a = op == SP_ADD || op == SP_SUB || op == SP_MUL || op == SP_MULK || op == SP_ACC || is_emit;
        const bool reads_b = op == SP_ADD || op == SP_SUB || op == SP_MUL;
        if ((reads_a && a >= SP_MAX_REGS) || (reads_b && b >= SP_MAX_REGS)) return bad(pc, "register out of range");
        if ((reads_a && !written[a]) || (reads_b && !written[b])) return bad(pc, "register read before any write");
        if ((op == SP_LOAD_WIRE || op == SP_LOAD_NEXT) && a >= num_columns) return bad(pc, "column out of range");
        if (op == SP_LOAD_PI && a >= num_public_inputs) return bad(pc, "public input out of range");
        if (op == SP_LOAD_IMM && a >= num_imms) return bad(pc, "LOAD_IMM index out of range");
        if (op == SP_MULK && b >= 64) return bad(pc, "MULK shift out of range");
        if (op == SP_ACC) {
            if (dst >= 4) return bad(pc, "ACC: accumulator out of range");
            if (b >= num_imms || imms[b] % glh::P >= (1ull << 32)) return bad(pc, "ACC: the immediate is missing / not below 2^32");
            acc_bound[dst] += (unsigned __int128)(imms[b] % glh::P) * 0xFFFFFFFFull;
            if (acc_bound[dst] >= ((unsigned __int128)1 << 63)) return bad(pc, "ACC: the accumulator could reach 2^63 before its ACCR");
            acc_used[dst] = true;
        } else if (op == SP_ACCR) {
            if (a >= 4) return bad(pc, "ACCR: accumulator out of range");
            if (!acc_used[a]) return bad(pc, "ACCR of an accumulator nothing was added to");
            acc_bound[a] = 0, acc_used[a] = false;
        }
        if (!is_emit && op != SP_ACC) {
            if (dst >= SP_MAX_REGS) return bad(pc, "register out of range");
            written[dst] = true;
        }
        emitted += is_emit;
    }
    if (!emitted) {
        *error = "STARK program: no EMIT, the STARK would have no constraints";
        return false;
    }
    return true;
}

uint32_t stark_num_zs(uint32_t num_pairs, uint32_t num_challenges, uint32_t qdf) { return (num_pairs * num_challenges + qdf - 1) / qdf; }

hipError_t stark_permutation_zs(const NttTables &tb, const uint64_t *trace, uint64_t trace_stride, const StarkPairsDev &pairs,
                                const uint64_t *h_challenges, uint32_t num_challenges, uint32_t qdf, uint32_t log_n, uint64_t *out,
                                hipStream_t stream) {
    PermChallenges ch = {};
    if (!load_challenges(&ch, h_challenges, num_challenges, qdf) || pairs.num_pairs == 0 || log_n > 24 || trace_stride < (1ull << log_n))
        return hipErrorInvalidValue;
    const uint64_t n = 1ull << log_n;
    const uint32_t num_zs = stark_num_zs(pairs.num_pairs, num_challenges, qdf);
    const uint64_t blocks = (n + SCAN_B - 1) / SCAN_B;
    if (!tb.scratch || tb.scratch_elems < blocks * num_zs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stark_perm_quotients_kernel, dim3(grid_for(n * num_zs, 256)), dim3(256), 0, stream, trace, trace_stride, pairs, ch,
                       num_challenges, qdf, num_zs, log_n, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // Z[0] = 1, Z[r] = prod_{s<r} q_s (permutation.rs:110-117): the exclusive prefix product of every Z slot
    uint64_t *totals = tb.scratch;
    hipLaunchKernelGGL(scan_blocks_kernel, dim3((unsigned)blocks, num_zs), dim3(SCAN_T), 0, stream, out, n, n, totals, blocks);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(num_zs), dim3(SCAN_T), 0, stream, totals, blocks, blocks);
    hipLaunchKernelGGL(stark_perm_finalize_kernel, dim3(grid_for(n * num_zs, 256)), dim3(256), 0, stream, out, totals, blocks, num_zs, log_n);
    return hipGetLastError();
}

hipError_t stark_ctl_zs(const NttTables &tb, const uint64_t *trace, uint64_t trace_stride, const StarkCtlDev &ctl, const uint64_t *h_challenges,
                        uint32_t num_challenges, uint32_t log_n, uint64_t *out, uint64_t *d_flag, hipStream_t stream) {
    CtlChallenges ch = {};
    if (!load_ctl_challenges(&ch, h_challenges, num_challenges) || ctl.num_zs == 0 || log_n > 24 || trace_stride < (1ull << log_n))
        return hipErrorInvalidValue;
    const uint64_t n = 1ull << log_n;
    const uint64_t blocks = (n + SCAN_B - 1) / SCAN_B;
    if (!tb.scratch || tb.scratch_elems < blocks * ctl.num_zs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stark_ctl_factors_kernel, dim3(grid_for(n * ctl.num_zs, 256)), dim3(256), 0, stream, trace, trace_stride, ctl, ch, log_n, out,
                       d_flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint64_t *totals = tb.scratch;
    hipLaunchKernelGGL(scan_blocks_kernel, dim3((unsigned)blocks, ctl.num_zs), dim3(SCAN_T), 0, stream, out, n, n, totals, blocks);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(ctl.num_zs), dim3(SCAN_T), 0, stream, totals, blocks, blocks);
    hipLaunchKernelGGL(stark_ctl_finalize_kernel, dim3(grid_for(n * ctl.num_zs, 256)), dim3(256), 0, stream, trace, trace_stride, ctl, ch, log_n, out,
                       totals, blocks);
    return hipGetLastError();
}

hipError_t stark_quotient_values(const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, hipStream_t stream) {
    const uint32_t qdb = glh::log2_ceil(a.qdf);
    if (a.num_challenges == 0 || a.num_challenges > STARK_MAX_CHALLENGES || a.qdf == 0 || a.qdf > STARK_MAX_QDF || qdb > a.rate_bits ||
        a.degree_bits + a.rate_bits > 24 || a.column_stride < (1ull << (a.degree_bits + a.rate_bits)) || !a.alphas)
        return hipErrorInvalidValue;
    StarkQuotientParams p = {};
    p.instrs = a.instrs, p.num_instrs = a.num_instrs, p.imms = a.imms, p.pis = a.public_inputs;
    p.trace = a.trace_lde, p.zs = a.zs_lde, p.twl = tb.twl, p.twh = tb.twh, p.out = out, p.stride = a.column_stride;
    p.num_challenges = a.num_challenges, p.qdf = a.qdf, p.degree_bits = a.degree_bits, p.qdb = qdb;
    if (a.pairs.num_pairs) {
        if (!a.zs_lde || !a.challenges || !load_challenges(&p.ch, a.challenges, a.num_challenges, a.qdf)) return hipErrorInvalidValue;
        p.pairs = a.pairs;
        p.num_zs = stark_num_zs(a.pairs.num_pairs, a.num_challenges, a.qdf);
    }
    if (a.ctl.num_zs) {
        if (!a.zs_lde || !load_ctl_challenges(&p.ctl_ch, a.ctl_challenges, a.num_challenges)) return hipErrorInvalidValue;
        p.ctl = a.ctl;
    }
    p.shift = 7;
    p.g_inv = glh::inv(glh::root_of_unity(a.degree_bits));
    for (uint32_t c = 0; c < a.num_challenges; c++) p.alpha[c] = a.alphas[c] % glh::P;
    const uint64_t g_pow_n = glh::pow(p.shift, 1ull << a.degree_bits), w = glh::root_of_unity(qdb);
    for (uint32_t e = 0; e < (1u << qdb); e++) {  // Z_H(x) = shift^n * w^(i mod 2^qdb) - 1 (zero_poly_coset.rs:20-41)
        p.zh[e] = glh::add(glh::mul(g_pow_n, glh::pow(w, e)), glh::P - 1);
        p.zh_inv[e] = glh::inv(p.zh[e]);
    }
    const uint64_t size = 1ull << (a.degree_bits + qdb);
    hipLaunchKernelGGL(stark_quotient_values_kernel, dim3(grid_for(size, 128)), dim3(128), 0, stream, p);
    return hipGetLastError();
}

}  // namespace plonky2_hip
