// stark.h — internal interface of the STARK kernels (stark.hip): starky's permutation Z polynomials and its constraint quotient,
// the constraints given as ONE register program for the whole STARK (the GlGateInstr encoding with the STARK opcodes of
// include/plonky2_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "ntt.h"

struct StarkJitArgs;  // stark_jit_device.h

namespace plonky2_hip {

constexpr uint32_t STARK_MAX_CHALLENGES = 4;  // num_challenges
constexpr uint32_t STARK_MAX_QDF = 16;        // quotient_degree_factor = the permutation batch size = the number of challenge sets

// What gl_stark_create checks once, on the host, before anything is allocated: opcodes of a STARK program only (no LOAD_CONST),
// columns / public inputs / immediates / registers in range, a register written before it is read, the ACC contract (weights
// below 2^32; between two ACCRs of an accumulator sum of weights * (2^32 - 1) < 2^63; no ACCR of an empty accumulator), and at
// least one EMIT. Returns false and fills `error`.
bool stark_program_validate(const uint16_t *instrs, uint32_t num_instrs, const uint64_t *imms, uint32_t num_imms, uint32_t num_columns,
                            uint32_t num_public_inputs, std::string *error);

// The permutation pairs of a STARK in device memory: pair p is column_pairs[pair_bounds[p] .. pair_bounds[p + 1]), a column pair
// the two words (lhs, rhs).
struct StarkPairsDev {
    const uint32_t *column_pairs = nullptr;  // device, 2 per column pair
    const uint32_t *pair_bounds = nullptr;   // device, num_pairs + 1
    uint32_t num_pairs = 0;
};

// challenge set s, challenge c: (beta, gamma) = h_challenges[2 * (s * num_challenges + c) + {0, 1}] — the order they are drawn in
// (get_n_permutation_challenge_sets, starky/src/permutation.rs:153-179); qdf sets.
uint32_t stark_num_zs(uint32_t num_pairs, uint32_t num_challenges, uint32_t qdf);

// out: [num_zs][n] value columns (compute_permutation_z_polys, permutation.rs:66-118)
hipError_t stark_permutation_zs(const NttTables &tb, const uint64_t *trace, uint64_t trace_stride, const StarkPairsDev &pairs,
                                const uint64_t *h_challenges, uint32_t num_challenges, uint32_t qdf, uint32_t log_n, uint64_t *out,
                                hipStream_t stream);

// The cross-table lookups seen from ONE table (evm/src/cross_table_lookup.rs), in device memory. A CTL column is
// constant + sum_j coeff_j row[col_j] (Column::eval, :100-119): column k is the terms column_bounds[k] .. column_bounds[k + 1];
// a table-with-columns (TWC) t is the CTL columns twc_column_bounds[t] .. twc_column_bounds[t + 1] with the filter column
// twc_filter[t] or STARK_CTL_NO_FILTER. CTL Z number z of the table belongs to TWC zs[2 z] under challenge zs[2 z + 1], in the
// order of cross_table_lookup_data (:237-312). Coefficients and constants are canonical.
constexpr uint32_t STARK_CTL_NO_FILTER = 0xFFFFFFFFu;
struct StarkCtlDev {
    const uint32_t *term_columns = nullptr, *column_bounds = nullptr, *twc_column_bounds = nullptr, *twc_filter = nullptr, *zs = nullptr;
    const uint64_t *term_coeffs = nullptr, *column_constants = nullptr;
    uint32_t num_zs = 0;
};

// out: [ctl.num_zs][n] value columns, Z[i] = prod_{r <= i} s_r with s_r = gamma + sum_j beta^j column_j(row r) where the filter is
// 1 and s_r = 1 where it is 0 (partial_products, cross_table_lookup.rs:314-341): the INCLUSIVE prefix product. h_challenges: (beta,
// gamma) of challenge c at [2 c]. A filter value that is neither 0 nor 1 stores 1 into *d_flag (which the caller zeroes and reads).
hipError_t stark_ctl_zs(const NttTables &tb, const uint64_t *trace, uint64_t trace_stride, const StarkCtlDev &ctl, const uint64_t *h_challenges,
                        uint32_t num_challenges, uint32_t log_n, uint64_t *out, uint64_t *d_flag, hipStream_t stream);

struct StarkQuotientArgs {
    const uint16_t *instrs;  // device, 4 x u16 per instruction
    uint32_t num_instrs;
    const uint64_t *imms;           // device, may be null without immediates
    const uint64_t *public_inputs;  // device, canonical; may be null without public inputs
    const uint64_t *trace_lde, *zs_lde;  // column-major LDEs in bit-reversed row order; zs_lde null without pairs
    uint64_t column_stride;              // >= n << rate_bits
    StarkPairsDev pairs;
    const uint64_t *alphas, *challenges;  // host
    uint32_t num_challenges, qdf, degree_bits, rate_bits;
    // the CTL checks behind the permutation checks (eval_cross_table_lookup_checks, cross_table_lookup.rs:410-451): zs_lde holds the
    // permutation Zs, then ctl.num_zs CTL Zs; ctl_challenges as for stark_ctl_zs (host). ctl.num_zs = 0: no CTL checks.
    StarkCtlDev ctl;
    const uint64_t *ctl_challenges;
};

// What the interpreter and a compiled quotient kernel both take per proof (stark_jit_device.h), from `a`: the checks the two routes
// share, the pointers, the coset shift, 1 / g, Z_H and its inverses, alphas and challenges mod p. `qdb`: log2_ceil(a.qdf).
hipError_t stark_point_args(const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, ::StarkJitArgs *args, uint32_t *qdb);

// out: [num_challenges][n << log2_ceil(qdf)] quotient VALUES on the coset 7 * <w>, natural order (compute_quotient_polys,
// starky/src/prover.rs:199-319 up to the coset_ifft)
hipError_t stark_quotient_values(const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, hipStream_t stream);

}  // namespace plonky2_hip
