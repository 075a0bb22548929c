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
#include "plonk.h"
#include "plonk_device.h"
#include "program_isa.h"
#include "stark_jit_device.h"

namespace plonky2_hip {

namespace {

using Sets = uint64_t[STARK_MAX_QDF * STARK_MAX_CHALLENGES];  // [set][challenge] betas or gammas
using PerChallenge = uint64_t[STARK_MAX_CHALLENGES];
struct PermChallenges { Sets beta, gamma; };
struct CtlChallenges { PerChallenge beta, gamma; };
static_assert(sizeof(Sets) == sizeof(StarkJitArgs::perm_beta) && sizeof(PerChallenge) == sizeof(StarkJitArgs::ctl_beta) &&
              sizeof(PerChallenge) == sizeof(StarkJitArgs::alpha) && 8 * STARK_MAX_QDF == sizeof(StarkJitArgs::zh));  // sized by literals there

// The two products of batch b at one row (permutation.rs:97-103, 299-320): over the instances f = b * qdf + k of the batch,
// instance f = (pair f / num_challenges, challenge f % num_challenges) with the challenges of SET k, the reduced values
// gamma + sum_j beta^j row[col_j] of the pair's left and right columns. `row` points at the row's element of column 0.
__device__ __forceinline__ void batch_products(const StarkPairsDev &pairs, const Sets &betas, const Sets &gammas, uint32_t num_challenges, uint32_t qdf,
                                               uint32_t b, const uint64_t *row, uint64_t stride, uint64_t &lhs, uint64_t &rhs) {
    lhs = rhs = 1;
    const uint32_t instances = pairs.num_pairs * num_challenges;
    for (uint32_t k = 0; k < qdf; k++) {
        const uint32_t f = b * qdf + k;
        if (f >= instances) break;  // the last batch may be short
        const uint32_t pair = f / num_challenges, c = f % num_challenges;
        const uint64_t beta = betas[k * num_challenges + c], gamma = gammas[k * num_challenges + c];
        uint64_t l = 0, r = 0;
        for (uint32_t j = pairs.pair_bounds[pair + 1]; j-- > pairs.pair_bounds[pair];) {  // Horner from the last column pair
            l = gl::mac(row[pairs.column_pairs[2 * j] * stride], l, beta);
            r = gl::mac(row[pairs.column_pairs[2 * j + 1] * stride], r, beta);
        }
        lhs = gl::mul(lhs, gl::add(l, gamma));
        rhs = gl::mul(rhs, gl::add(r, gamma));
    }
}

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
__device__ __forceinline__ void ctl_challenge(const PerChallenge &betas, const PerChallenge &gammas, uint32_t c, uint64_t &beta, uint64_t &gamma) {
    beta = betas[0], gamma = gammas[0];
#pragma unroll
    for (uint32_t e = 1; e < STARK_MAX_CHALLENGES; e++) {
        beta = c == e ? betas[e] : beta;
        gamma = c == e ? gammas[e] : gamma;
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
    ctl_challenge(ch.beta, ch.gamma, d.zs[2 * z + 1], beta, gamma);
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
    batch_products(pairs, ch.beta, ch.gamma, num_challenges, qdf, b, trace + i, trace_stride, lhs, rhs);
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
    StarkJitArgs p;  // what the compiled kernels take as well (stark_point_args)
    const uint16_t *instrs;
    const uint64_t *imms;
    StarkPairsDev pairs;
    uint32_t num_instrs, num_zs, num_challenges, qdf, qdb;
    StarkCtlDev ctl;  // num_zs = 0 without cross-table lookups
};

__global__ __launch_bounds__(128) void stark_quotient_values_kernel(const StarkQuotientParams k) {
    const StarkJitArgs &p = k.p;
    sj::Point q;
    if (!sj::locate(p, k.qdb, q)) return;
    sj::head(p, k.qdb, q, true);
    uint64_t sums[STARK_MAX_CHALLENGES] = {0, 0, 0, 0};
    auto constraint = [&](uint64_t v) { sj::constraint(sums, p, v, k.num_challenges); };

    uint64_t regs[isa::MAX_REGS];
    uint64_t acc_lo[4] = {0, 0, 0, 0}, acc_hi[4] = {0, 0, 0, 0};  // ACC: plain (wrapping-free by contract) sums of the 32-bit halves
    for (uint32_t pc = 0; pc < k.num_instrs; pc++) {
        const uint16_t *in = k.instrs + 4 * pc;
        const uint16_t op = in[0], dst = in[1] & (isa::MAX_REGS - 1), a = in[2], b = in[3];
        switch (op) {
            case isa::LOAD_WIRE: regs[dst] = q.local[a * p.stride]; break;
            case isa::LOAD_NEXT: regs[dst] = q.next[a * p.stride]; break;
            case isa::LOAD_PI: regs[dst] = p.pis[a]; break;
            case isa::LOAD_IMM: regs[dst] = k.imms[a]; break;
            case isa::ADD: regs[dst] = gl::add(regs[a & (isa::MAX_REGS - 1)], regs[b & (isa::MAX_REGS - 1)]); break;
            case isa::SUB: regs[dst] = gl::sub(regs[a & (isa::MAX_REGS - 1)], regs[b & (isa::MAX_REGS - 1)]); break;
            case isa::MUL: regs[dst] = gl::mul(regs[a & (isa::MAX_REGS - 1)], regs[b & (isa::MAX_REGS - 1)]); break;
            case isa::MULK: regs[dst] = gl::mul(regs[a & (isa::MAX_REGS - 1)], 1ull << (b & 63)); break;
            case isa::ACC: {
                const uint64_t w = k.imms[b];
                acc_lo[dst & 3] += (regs[a & (isa::MAX_REGS - 1)] & 0xFFFFFFFFull) * w;
                acc_hi[dst & 3] += (regs[a & (isa::MAX_REGS - 1)] >> 32) * w;
                break;
            }
            case isa::ACCR:
                regs[dst] = gl::fold96(acc_lo[a & 3], acc_hi[a & 3]);
                acc_lo[a & 3] = acc_hi[a & 3] = 0;
                break;
            case isa::EMIT: constraint(regs[a & (isa::MAX_REGS - 1)]); break;
            case isa::EMIT_TRANSITION: constraint(gl::mul(regs[a & (isa::MAX_REGS - 1)], q.z_last)); break;
            case isa::EMIT_FIRST_ROW: constraint(gl::mul(regs[a & (isa::MAX_REGS - 1)], q.l_first)); break;
            case isa::EMIT_LAST_ROW: constraint(gl::mul(regs[a & (isa::MAX_REGS - 1)], q.l_last)); break;
            default: break;  // refused by stark_program_validate
        }
    }
    // eval_permutation_checks (permutation.rs:284-322): Z(1) = 1 for every Z, then per batch Z(g x) prod rhs = Z(x) prod lhs
    for (uint32_t z = 0; z < k.num_zs; z++) constraint(gl::mul(gl::sub(p.zs[z * p.stride + q.t], 1), q.l_first));
    for (uint32_t z = 0; z < k.num_zs; z++) {
        uint64_t lhs, rhs;
        batch_products(k.pairs, p.perm_beta, p.perm_gamma, k.num_challenges, k.qdf, z, q.local, p.stride, lhs, rhs);
        constraint(gl::sub(gl::mul(p.zs[z * p.stride + q.t_next], rhs), gl::mul(p.zs[z * p.stride + q.t], lhs)));
    }
    // eval_cross_table_lookup_checks (evm/src/cross_table_lookup.rs:421-450), the CTL Zs behind the permutation Zs: with
    // select(f, x) = f x + 1 - f, Z(1) = select(filter, combine) on the first row and Z(g x) = Z(x) select(filter', combine') on
    // every row but the last
    for (uint32_t z = 0; z < k.ctl.num_zs; z++) {
        const uint32_t tw = k.ctl.zs[2 * z], filter = k.ctl.twc_filter[tw];
        uint64_t beta, gamma;
        ctl_challenge(p.ctl_beta, p.ctl_gamma, k.ctl.zs[2 * z + 1], beta, gamma);
        uint64_t sel_local = ctl_combine(k.ctl, tw, beta, gamma, q.local, p.stride), sel_next = ctl_combine(k.ctl, tw, beta, gamma, q.next, p.stride);
        if (filter != STARK_CTL_NO_FILTER) {
            const uint64_t f_local = ctl_column(k.ctl, filter, q.local, p.stride), f_next = ctl_column(k.ctl, filter, q.next, p.stride);
            sel_local = gl::sub(gl::mac(1, f_local, sel_local), f_local);
            sel_next = gl::sub(gl::mac(1, f_next, sel_next), f_next);
        }
        const uint64_t z_local = p.zs[(k.num_zs + z) * p.stride + q.t], z_next = p.zs[(k.num_zs + z) * p.stride + q.t_next];
        constraint(gl::mul(gl::sub(z_local, sel_local), q.l_first));
        constraint(gl::mul(gl::sub(z_next, gl::mul(z_local, sel_next)), q.z_last));
    }
    sj::tail(sums, p, q, k.num_challenges);
}

unsigned grid_for(uint64_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

bool load_challenges(Sets &beta, Sets &gamma, const uint64_t *h_challenges, uint32_t num_challenges, uint32_t qdf) {
    if (num_challenges == 0 || num_challenges > STARK_MAX_CHALLENGES || qdf == 0 || qdf > STARK_MAX_QDF) return false;
    for (uint32_t k = 0; k < qdf * num_challenges; k++) {
        beta[k] = h_challenges[2 * k] % glh::P;
        gamma[k] = h_challenges[2 * k + 1] % glh::P;
    }
    return true;
}

bool load_ctl_challenges(PerChallenge &beta, PerChallenge &gamma, const uint64_t *h_challenges, uint32_t num_challenges) {
    if (!h_challenges || num_challenges == 0 || num_challenges > STARK_MAX_CHALLENGES) return false;
    for (uint32_t c = 0; c < num_challenges; c++) {
        beta[c] = h_challenges[2 * c] % glh::P;
        gamma[c] = h_challenges[2 * c + 1] % glh::P;
    }
    return true;
}

}  // namespace

bool stark_program_validate(const uint16_t *instrs, uint32_t num_instrs, const uint64_t *imms, uint32_t num_imms, uint32_t num_columns,
                            uint32_t num_public_inputs, std::string *error) {
    bool written[isa::MAX_REGS] = {};
    isa::AccBound acc_bound[isa::MAX_ACCS];
    bool acc_used[isa::MAX_ACCS] = {};
    uint32_t emitted = 0;
    auto bad = [&](uint32_t pc, const std::string &what) {
        *error = "STARK program, instruction " + std::to_string(pc) + ": " + what;
        return false;
    };
    for (uint32_t pc = 0; pc < num_instrs; pc++) {
        const isa::Instr in = isa::instr_at(instrs, pc);
        const uint16_t op = in.op, dst = in.dst, a = in.a, b = in.b;
        if (op == isa::LOAD_CONST) return bad(pc, "LOAD_CONST: a STARK has no constants columns");
        if (op > isa::EMIT_LAST_ROW) return bad(pc, "unknown opcode");
        const bool is_emit = isa::is_emit(op), reads_a = isa::reads_a(op), reads_b = isa::reads_b(op);
        if ((reads_a && a >= isa::MAX_REGS) || (reads_b && b >= isa::MAX_REGS)) return bad(pc, "register out of range");
        if ((reads_a && !written[a]) || (reads_b && !written[b])) return bad(pc, "register read before any write");
        if ((op == isa::LOAD_WIRE || op == isa::LOAD_NEXT) && a >= num_columns) return bad(pc, "column out of range");
        if (op == isa::LOAD_PI && a >= num_public_inputs) return bad(pc, "public input out of range");
        if (op == isa::LOAD_IMM && a >= num_imms) return bad(pc, "LOAD_IMM index out of range");
        if (op == isa::MULK && b >= 64) return bad(pc, "MULK shift out of range");
        if (op == isa::ACC) {
            if (dst >= isa::MAX_ACCS) return bad(pc, "ACC: accumulator out of range");
            if (b >= num_imms || imms[b] % glh::P >= (1ull << 32)) return bad(pc, "ACC: the immediate is missing / not below 2^32");
            if (!acc_bound[dst].add(imms[b] % glh::P)) return bad(pc, "ACC: the accumulator could reach 2^63 before its ACCR");
            acc_used[dst] = true;
        } else if (op == isa::ACCR) {
            if (a >= isa::MAX_ACCS) return bad(pc, "ACCR: accumulator out of range");
            if (!acc_used[a]) return bad(pc, "ACCR of an accumulator nothing was added to");
            acc_bound[a].reset(), acc_used[a] = false;
        }
        if (isa::writes_reg(op)) {
            if (dst >= isa::MAX_REGS) return bad(pc, "register out of range");
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
    if (!load_challenges(ch.beta, ch.gamma, h_challenges, num_challenges, qdf) || pairs.num_pairs == 0 || log_n > 24 || trace_stride < (1ull << log_n))
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
    if (!load_ctl_challenges(ch.beta, ch.gamma, h_challenges, num_challenges) || ctl.num_zs == 0 || log_n > 24 || trace_stride < (1ull << log_n))
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

hipError_t stark_point_args(const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, StarkJitArgs *args, uint32_t *qdb_out) {
    const uint32_t qdb = glh::log2_ceil(a.qdf);
    if (a.num_challenges == 0 || a.num_challenges > STARK_MAX_CHALLENGES || a.qdf == 0 || a.qdf > STARK_MAX_QDF || qdb > a.rate_bits ||
        a.degree_bits + a.rate_bits > 24 || a.column_stride < (1ull << (a.degree_bits + a.rate_bits)) || !a.alphas)
        return hipErrorInvalidValue;
    StarkJitArgs &p = *args;
    p = {};
    p.pis = a.public_inputs, p.trace = a.trace_lde, p.zs = a.zs_lde, p.twl = tb.twl, p.twh = tb.twh, p.out = out, p.stride = a.column_stride;
    p.degree_bits = a.degree_bits;
    if (a.pairs.num_pairs && (!a.zs_lde || !a.challenges || !load_challenges(p.perm_beta, p.perm_gamma, a.challenges, a.num_challenges, a.qdf)))
        return hipErrorInvalidValue;
    if (a.ctl.num_zs && (!a.zs_lde || !load_ctl_challenges(p.ctl_beta, p.ctl_gamma, a.ctl_challenges, a.num_challenges))) return hipErrorInvalidValue;
    p.shift = 7, p.g_inv = glh::inv(glh::root_of_unity(a.degree_bits));
    for (uint32_t c = 0; c < a.num_challenges; c++) p.alpha[c] = a.alphas[c] % glh::P;
    zh_on_coset(glh::pow(p.shift, 1ull << a.degree_bits), qdb, p.zh, p.zh_inv);
    *qdb_out = qdb;
    return hipSuccess;
}

hipError_t stark_quotient_values(const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, hipStream_t stream) {
    StarkQuotientParams k = {};
    if (hipError_t e = stark_point_args(tb, a, out, &k.p, &k.qdb); e != hipSuccess) return e;
    k.instrs = a.instrs, k.num_instrs = a.num_instrs, k.imms = a.imms;
    k.num_challenges = a.num_challenges, k.qdf = a.qdf;
    if (a.pairs.num_pairs) {
        k.pairs = a.pairs;
        k.num_zs = stark_num_zs(a.pairs.num_pairs, a.num_challenges, a.qdf);
    }
    if (a.ctl.num_zs) k.ctl = a.ctl;
    const uint64_t size = 1ull << (a.degree_bits + k.qdb);
    hipLaunchKernelGGL(stark_quotient_values_kernel, dim3(grid_for(size, 128)), dim3(128), 0, stream, k);
    return hipGetLastError();
}

}  // namespace plonky2_hip
