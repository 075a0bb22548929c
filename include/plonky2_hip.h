/* plonky2_hip.h — C ABI of libplonky2_hip.so: the MI355X (gfx950) replacement for the reference's
 * `cuda/` crate (sideprotocol/plonky2-gpu), covering the prover's data-parallel hot path only:
 * Goldilocks NTT / inverse NTT / coset LDE, Poseidon Merkle-cap construction and the
 * PolynomialBatch commit; the permutation argument, the quotient polynomials for any circuit (gates as
 * register programs), openings and the FRI opening pipeline; and, on top of those, a whole prove() in one call.
 * No circuit building, witness generation or verification.
 *
 * Two groups of entry points:
 *   (A) the reference's own extern "C" symbols (cuda/src/lib.rs:58-145 <-> cuda/plonky2_gpu.cu),
 *       same names, argument order and memory-layout contract, so the Rust side links unchanged;
 *   (B) a generic-shape `gl_*` API with 64-bit sizes, explicit strides and real error returns,
 *       which (A) is implemented on and which new host code should prefer.
 *
 * Conventions
 *   - Field elements are plain-domain Goldilocks u64 (p = 2^64 - 2^32 + 1). Inputs may be any
 *     u64 representative (field/src/goldilocks_field.rs:26); every OUTPUT buffer holds canonical
 *     values (< p), i.e. exactly what the reference yields after `to_canonical_u64`. Except for
 *     gl_transpose, gl_ext2_interleave, gl_pack_leaf_ranges and the opened leaves of
 *     gl_merkle_open_batch / gl_merkle_open_batch_device: pure data movement, the output holds the
 *     input's words unchanged — canonical in, canonical out.
 *   - All `d_*` pointers are DEVICE pointers. The callee allocates nothing for data: the caller
 *     owns every buffer (as in the reference, plonky2/src/fri/oracle.rs:94-106). The library keeps,
 *     per device, a few hundred KiB of read-only twiddle tables, and per CONTEXT one workspace of
 *     gl_workspace_bytes() = 512 MiB (allocated by gl_ctx_create(), or on the first call that sees a
 *     caller-built context; gl_ctx_set_workspace() hands in the caller's own memory instead, for a
 *     host that sizes all device memory up front) that the natural-order transforms, the scans
 *     (partial products, divide_by_linear), the opening partial sums, gl_sponge_absorb,
 *     gl_merkle_open_batch and gl_fri_proof_of_work stage through, plus the commit's event pair and
 *     its low-priority hashing stream.
 *     Several contexts on one device run CONCURRENTLY (up to version 0.5 they took turns): nothing
 *     mutable is shared between them, so two host threads, each with its own context, keep two
 *     proofs in flight on one GPU and each fills the other's latency-bound phases (transcript,
 *     small tree layers, openings). One context is used by one host thread at a time; data shared
 *     by two contexts is the caller's to order, as with any two streams. Two things are still taken
 *     in turns, because their constant tables exist once: launches of ONE compiled gate kernel
 *     (gl_gate_kernel_build; proofs of one circuit handle on two contexts overlap everywhere
 *     except in the gate kernels) and the reference symbol compute_quotient_polys per device.
 *     A circuit handle (gl_circuit_create) may be proven with from several contexts at once; it
 *     keeps one buffer pool per context.
 *     Three entry points do allocate device memory themselves: gl_circuit_create (the preprocessed
 *     commitment, freed by gl_circuit_destroy) and gl_prove (every buffer of one proof), because their
 *     job is to own a whole computation, and the reference symbol compute_quotient_polys (a staging
 *     buffer, unless the caller provides it: gl_reference_quotient_set_staging).
 *   - Errors are returned BY VALUE as {code, message}; code 0 = success; `message` is
 *     malloc'ed (strdup) and owned by the caller, who frees it with free() — the convention of
 *     cuda/src/lib.rs:21-35 / cuda/plonky2_gpu.cu:19-31.
 *   - `ctx` points to {hipStream_t stream; hipStream_t stream2;} — the HIP twin of the reference's
 *     CudaInnerContext (plonky2/src/fri/oracle.rs:43-47, cuda/plonky2_gpu.cu:4-7). Create one with
 *     gl_ctx_create() or hand in your own pair of streams.
 *   - (B) calls are ASYNCHRONOUS on ctx->stream unless stated otherwise; (A) calls synchronise
 *     the stream before returning, like the reference (cuda/plonky2_gpu.cu:82).
 */
#ifndef PLONKY2_HIP_H
#define PLONKY2_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#pragma GCC visibility push(default)

/* == cuda::Error (cuda/src/lib.rs:21-25) / RustError (cuda/plonky2_gpu.cu:19-31) */
typedef struct GlError {
    int code;      /* 0 = ok; >0 = hipError_t; <0 = library error (GL_E_*) */
    char *message; /* NULL or strdup'ed, caller frees */
} GlError;

#define GL_E_INVALID (-1)     /* bad argument (sizes, alignment, NULL) */
#define GL_E_UNSUPPORTED (-2) /* entry point outside the hot path of this build */

/* == DataSlice (cuda/src/lib.rs:52-56): host struct holding a device pointer + i32 length */
typedef struct GlDataSlice {
    const void *ptr;
    int len;
} GlDataSlice;

/* ---------------------------------------------------------------------------------------------
 * (B) generic API
 * ------------------------------------------------------------------------------------------- */

/* Context = two HIP streams on one device (layout-compatible with CudaInnerContext). */
int gl_device_count(void);
void *gl_ctx_create(int device); /* NULL on failure; also makes `device` current */
void gl_ctx_destroy(void *ctx);
GlError gl_ctx_synchronize(void *ctx); /* waits for both streams */
/* A caller-built context ({stream, stream2} made with the host's own HIP binding, e.g. the reference's
 * CudaInnerContext through rustacuda_hip) gets its library-side state (workspace, events, hashing stream) on the
 * first call that sees it, keyed by ctx->stream; gl_ctx_release() waits for both streams and gives that state back
 * (before the caller destroys its streams). gl_ctx_destroy() = gl_ctx_release() + destroying the streams it created. */
void gl_ctx_release(void *ctx);
/* The workspace of a context: gl_workspace_bytes() bytes (constant for a build: 512 MiB). gl_ctx_set_workspace()
 * replaces the library's allocation by `d_workspace` (>= gl_workspace_bytes() bytes, 16-byte aligned, on the context's
 * device, the caller's to free after gl_ctx_release / gl_ctx_destroy) — the reference's memory contract, in which the
 * caller sizes every device buffer once up front (fri/oracle.rs:94-106) and the callee allocates nothing.
 * d_workspace = NULL goes back to a library-owned one. Waits for the context's stream. */
uint64_t gl_workspace_bytes(void);
GlError gl_ctx_set_workspace(void *ctx, void *d_workspace, uint64_t bytes);

/* Thin device-memory helpers for hosts without a HIP binding (synchronous). gl_malloc allocates on the calling
 * thread's CURRENT device; gl_ctx_malloc on the device of `ctx` (and makes it current) — what a host with several
 * contexts, or with threads that never called hipSetDevice, should use. Every entry point that takes a ctx runs on
 * the ctx's device in the same way, whatever the thread's current device was. */
GlError gl_malloc(void **d_ptr, uint64_t bytes);
GlError gl_ctx_malloc(void **d_ptr, uint64_t bytes, void *ctx);
GlError gl_free(void *d_ptr);
/* Page-locked host staging memory — the reference's MyAllocator (plonky2/src/fri/oracle.rs:49-73,
 * cudaHostAlloc): transfers from it run at link speed and do not stage through a bounce buffer. */
GlError gl_malloc_host(void **h_ptr, uint64_t bytes);
GlError gl_free_host(void *h_ptr);
GlError gl_memcpy_h2d(void *d_dst, const void *h_src, uint64_t bytes, void *ctx);
/* The same copy queued on ctx->stream2 WITHOUT waiting for it: with h_src page-locked (gl_malloc_host) it runs on
 * the DMA engines while ctx->stream computes — upload the next proof's witness during gl_prove of the current one
 * (gl_prove works on ctx->stream and waits for both streams only when it is done), then gl_ctx_synchronize()
 * before using d_dst. The witness upload (468 MiB, 8.5 ms at the ed25519 shape) disappears from the proof period. */
GlError gl_memcpy_h2d_async(void *d_dst, const void *h_src, uint64_t bytes, void *ctx);
GlError gl_memcpy_d2h(void *h_dst, const void *d_src, uint64_t bytes, void *ctx);
GlError gl_memcpy_d2d(void *d_dst, const void *d_src, uint64_t bytes, void *ctx);
GlError gl_memset_zero(void *d_dst, uint64_t bytes, void *ctx);

/* HIP-event timing on ctx->stream (what bench.py brackets kernels with). */
GlError gl_event_create(void **event);
GlError gl_event_record(void *event, void *ctx);
GlError gl_event_elapsed_ms(float *ms, void *start_event, void *stop_event); /* syncs on stop */
void gl_event_destroy(void *event);

/* Batched NTT, in place. Polynomial i occupies d_values[i*stride .. i*stride + 2^log_n).
 *   inverse = 0: fft_with_options(.., zero_factor None)  (field/src/fft.rs:58-66)
 *   inverse = 1: ifft_with_options                        (field/src/fft.rs:73-103)
 *   bit_reversed = 1 (forward only): output slot m holds the value of natural index bitrev(m),
 *     i.e. reverse_index_bits(fft(x)) (util/src/lib.rs:188) — the Merkle leaf order.
 * log_n <= 24. stride >= 2^log_n; for inverse, stride must be a multiple of 2^log_n. The passes move 16 bytes at a time:
 * d_values must be 16-byte aligned and, when poly_num > 1 and log_n > 0, stride even (one polynomial has no stride: any
 * value >= 2^log_n is accepted). Words between the polynomials (stride > 2^log_n) are not written. A violation is
 * GL_E_INVALID and nothing is touched. Here and in every call that takes a stride or a pitch, it has no upper bound: every
 * offset `column * stride` is formed in 64 bits, so columns may lie more than 2^32 words apart. */
GlError gl_ntt_batch(uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint64_t stride, int inverse,
                     int bit_reversed, void *ctx);

/* Coset low-degree extension of poly_num coefficient vectors (length 2^log_n) to
 * 2^(log_n+rate_bits) evaluations on shift*H, BIT-REVERSED order:
 *   d_out[i*dst_stride + m] = coset_fft_with_options(lde(coeffs_i, rate_bits), shift)[bitrev(m)]
 * (field/src/polynomial/mod.rs:205-207, 286-299; fri/oracle.rs:979-1004 then :942-952 per column).
 * d_out must not overlap d_coeffs. log_n <= 24, rate_bits <= 8. src_stride >= 2^log_n and dst_stride >= 2^(log_n+rate_bits), both
 * even when log_n > 0 (for any poly_num), both buffers 16-byte aligned; a violation is GL_E_INVALID. Any such dst_stride works at
 * every size (a padded column pitch for the LDE buffer); at log_n >= 22 (three passes) a dst_stride other than
 * 2^(log_n+rate_bits) runs the polynomials one launch sequence at a time. Words between the columns are not written. */
GlError gl_coset_lde_batch(const uint64_t *d_coeffs, uint64_t *d_out, uint64_t poly_num, uint32_t log_n,
                           uint32_t rate_bits, uint64_t shift, uint64_t src_stride, uint64_t dst_stride, void *ctx);

/* Natural-order coset transforms, in place:
 *   inverse = 0: PolynomialCoeffs::coset_fft(shift)   (field/src/polynomial/mod.rs:281-299)
 *   inverse = 1: PolynomialValues::coset_ifft(shift)  (field/src/polynomial/mod.rs:64-77) — the
 *               last step of compute_quotient_polys (plonk/prover.rs:1009-1021).
 * d_values, log_n and stride obey the rules of gl_ntt_batch (alignment, even stride, inverse: stride % 2^log_n == 0); they are
 * checked before anything is scaled: a refused call (GL_E_INVALID) leaves d_values as it was. */
GlError gl_coset_ntt_batch(uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint64_t stride, uint64_t shift, int inverse,
                           void *ctx);

/* Partial products and Z of the permutation argument for every challenge
 * (wires_permutation_partial_products_and_zs, plonky2/src/plonk/prover.rs:702-786;
 * quotient_chunk_products / partial_products_and_z_gx, plonky2/src/util/partial_products.rs:13-37).
 *   d_wires [>= num_routed][2^log_n] column-major, column stride wires_stride (the witness layout)
 *   d_sigmas [num_routed][2^log_n] column-major (prover_data.sigmas transposed), d_k_is [num_routed]
 *   h_betas / h_gammas: HOST arrays of num_challenges elements
 *   d_out [num_challenges * (1 + num_prods)][2^log_n], num_prods = ceil(num_routed / qdf) - 1, in the
 *   order the prover commits them: every Z first, then the partial products challenge-major
 *   (prover.rs:112-117) — ready for gl_commit_from_values. */
GlError gl_permutation_partial_products(const uint64_t *d_wires, uint64_t wires_stride, const uint64_t *d_sigmas,
                                        uint64_t sigmas_stride, const uint64_t *d_k_is, const uint64_t *h_betas,
                                        const uint64_t *h_gammas, uint32_t num_challenges, uint32_t num_routed,
                                        uint32_t quotient_degree_factor, uint32_t log_n, uint64_t *d_out, void *ctx);

/* compute_quotient_polys (plonky2/src/plonk/prover.rs:790-1034) for any circuit: the permutation
 * terms, L_0(x)(Z(x)-1), the alpha reduction and the division by Z_H are evaluated here
 * (plonk/vanishing_poly.rs:100-226, plonk_common.rs:97-114, field/src/zero_poly_coset.rs); the
 * circuit-specific gate-constraint terms are an INPUT, one row of num_gate_constraints values per
 * LDE point in natural point order (NULL = no gate constraints). The three *_leaves pointers are the
 * leaf-major LDE rows of the commitments (d_leaves of gl_commit_*), read at leaf
 * reverse_bits(i * step) like PolynomialBatch::get_lde_values (fri/oracle.rs:1007-1018).
 * d_quotient_polys [num_challenges][n << log2_ceil(qdf)] receives the COEFFICIENTS (after coset_ifft,
 * prover.rs:1009-1021); chunking into degree-n pieces is a reinterpretation (prover.rs:153-166). */
/* Table-driven gate constraints for gl_compute_quotient_polys: evaluate_gate_constraints_base_batch
 * (plonky2/src/plonk/vanishing_poly.rs:267-306) with compute_filter (gates/gate.rs:261-268) for ANY circuit.
 * Each gate is a register program of GlGateInstr {op, dst, a, b} (u16 each):
 *   0 LOAD_WIRE dst<-local_wires[a]      1 LOAD_CONST dst<-local_constants[num_selectors+a]
 *   2 LOAD_PI dst<-public_inputs_hash[a]  3 LOAD_IMM dst<-d_immediates[a]
 *   4 ADD  5 SUB  6 MUL  dst<-r[a] op r[b]       7 EMIT next constraint of the gate <- r[a]
 *   8 MULK dst<-r[a] * 2^b  (b < 64; a shift in the run-time compiled kernel)
 *   9 ACC  acc[dst] += r[a] * d_immediates[b]   (4 accumulators, dst = 0..3; the immediate must be < 2^32)
 *  10 ACCR dst<-acc[a] mod p; acc[a]<-0
 *     Sums with small constant weights without a modular step per term — limb recombinations sum limb_j * B^j,
 *     MDS rows — the way plonky2 computes its MDS layer on x86 (hash/poseidon.rs:34-47 uses the same split): an
 *     accumulator is a pair of plain u64 sums over the low and the high 32-bit halves of the operands, one
 *     32x32+64 multiply-add each per term, folded as lo + hi*2^32 mod p by ACCR. CONTRACT: between two ACCRs of an
 *     accumulator, sum of immediates * (2^32 - 1) < 2^63, so that neither half can wrap. gl_gate_kernel_build checks
 *     this and refuses the program otherwise; the interpreter cannot (its program is in device memory), the
 *     emitters in plonky2_gpu_amd/gate_program.py enforce it when they generate code. Accumulators start at 0 in
 *     every gate.
 * (64 registers). Indices are taken as written: a register index >= 64, an accumulator index >= 4 (ACC's dst, ACCR's a),
 * a MULK shift >= 64 and a LOAD_PI index >= 4 are GL_E_INVALID wherever the host sees the programs — gl_gate_kernel_build,
 * and gl_circuit_create for the compiled kernel and for the interpreter alike. (The device code masks them, & 63 and & 3,
 * so that a GlGateProgram handed over in device memory cannot index out of bounds; no valid program relies on that.)
 * A register is written before it is read. Gate g is described by GlGateDesc {row = its index in the circuit's gate list,
 * selector_index, group_start, group_end (selectors_info.groups[selector_index]), prog_start, prog_len}.
 * Constraint k of every gate accumulates into term k, multiplied by the gate's filter. */
typedef struct GlGateInstr {
    uint16_t op, dst, a, b;
} GlGateInstr;
typedef struct GlGateDesc {
    uint32_t row, selector_index, group_start, group_end, prog_start, prog_len;
} GlGateDesc;
typedef struct GlGateProgram {
    const GlGateInstr *d_instrs;  /* device */
    const GlGateDesc *d_gates;    /* device */
    const uint64_t *d_immediates; /* device, may be NULL */
    uint32_t num_gates, num_selectors;
    uint64_t public_inputs_hash[4];
} GlGateProgram;

/* Emitters of the register programs for the gate kinds of the ed25519 gate list, so that a compiled host needs no Python to
 * describe its circuit: what each gate's eval_unfiltered_base_one computes (plonky2/src/gates/{noop,constant,public_input,
 * arithmetic_base,base_sum,random_access,poseidon}.rs, u32/src/gates/{add_many_u32,arithmetic_u32,subtraction_u32,
 * range_check_u32,comparison}.rs), as a program in the encoding above — with the ACC / ACCR accumulators wherever a sum has
 * small constant weights, and their overflow contract enforced at emission. params by kind:
 *   NOOP, PUBLIC_INPUT, POSEIDON: none        CONSTANT {num_consts}         ARITHMETIC {num_ops}
 *   BASE_SUM {B, num_limbs}                   U32_ADD_MANY {num_addends, num_ops}
 *   U32_ARITHMETIC / U32_SUBTRACTION {num_ops}  U32_RANGE_CHECK {num_input_limbs}
 *   COMPARISON {num_bits, num_chunks} (chunks of at most 4 bits)   RANDOM_ACCESS {bits, num_copies, num_extra_constants}
 *   ARITHMETIC_EXTENSION / MUL_EXTENSION {num_ops}   REDUCING / REDUCING_EXTENSION {num_coeffs}   EXPONENTIATION {num_power_bits}
 *   POSEIDON_MDS: none   LOW_DEGREE_INTERPOLATION / HIGH_DEGREE_INTERPOLATION {subgroup_bits <= 4}
 *   (plonky2/src/gates/{arithmetic_extension,multiplication_extension,reducing,reducing_extension,exponentiation,poseidon_mds,
 *   low_degree_interpolation,high_degree_interpolation}.rs; pairs of wires are elements of F_p[X]/(X^2 - 7), plonk/vars.rs:122-129)
 * gl_gate_programs_emit builds the programs of a whole gate list in circuit order (gate i has selector index
 * gates[i].selector_index; group_bounds[2 s], group_bounds[2 s + 1] = selectors_info.groups[s], gates/selectors.rs): host arrays
 * in exactly the form GlCircuitDesc / gl_gate_kernel_build take, immediates deduplicated across the list, num_gate_constraints =
 * the largest number of constraints of any gate. The arrays are malloc'd by the library: release them with
 * gl_gate_programs_free. Pure host code: no device is needed. */
enum GlGateKind {
    GL_GATE_NOOP = 0, GL_GATE_CONSTANT = 1, GL_GATE_PUBLIC_INPUT = 2, GL_GATE_ARITHMETIC = 3, GL_GATE_BASE_SUM = 4,
    GL_GATE_U32_ADD_MANY = 5, GL_GATE_U32_ARITHMETIC = 6, GL_GATE_U32_SUBTRACTION = 7, GL_GATE_U32_RANGE_CHECK = 8,
    GL_GATE_COMPARISON = 9, GL_GATE_RANDOM_ACCESS = 10, GL_GATE_POSEIDON = 11,
    /* the other gates of upstream plonky2 (what standard_recursion_config circuits are made of), extension degree D = 2 */
    GL_GATE_ARITHMETIC_EXTENSION = 12, GL_GATE_MUL_EXTENSION = 13, GL_GATE_REDUCING = 14, GL_GATE_REDUCING_EXTENSION = 15,
    GL_GATE_EXPONENTIATION = 16, GL_GATE_POSEIDON_MDS = 17, GL_GATE_LOW_DEGREE_INTERPOLATION = 18, GL_GATE_HIGH_DEGREE_INTERPOLATION = 19
};
typedef struct GlGateSpec {
    uint32_t kind;      /* GlGateKind */
    uint32_t params[3];
    uint32_t selector_index;
} GlGateSpec;
typedef struct GlGatePrograms {
    GlGateInstr *instrs;
    GlGateDesc *gates;
    uint64_t *immediates;
    uint32_t num_instrs, num_gates, num_immediates, num_gate_constraints;
} GlGatePrograms;
GlError gl_gate_programs_emit(const GlGateSpec *gates, uint32_t num_gates, const uint32_t *group_bounds, uint32_t num_selectors,
                              GlGatePrograms *out);
void gl_gate_programs_free(GlGatePrograms *programs);

/* The same gate programs compiled at run time (hiprtc, gfx950) into a kernel specialised to the circuit:
 * gates that share wires and subexpressions are generated together (fused units: each value is loaded / computed once and goes to every
 * gate's accumulators), registers in VGPRs, immediates as literals or scalar operands. Built once per circuit
 * (under a second for a few small gates; the 25-gate ed25519 list: about a minute of CPU, in six units — 15 s when forked hiprtc workers
 * compile them side by side, PLONKY2_HIP_JIT_FORK=1), reused for every proof; h_* are HOST arrays in the GlGateInstr / GlGateDesc encoding.
 * On failure the GlError message carries the compiler log. */
GlError gl_gate_kernel_build(const GlGateInstr *h_instrs, uint32_t num_instrs, const GlGateDesc *h_gates, uint32_t num_gates,
                             const uint64_t *h_immediates, uint32_t num_immediates, uint32_t num_selectors,
                             uint32_t num_gate_constraints, uint32_t num_challenges, void **kernel);
void gl_gate_kernel_destroy(void *kernel);
/* the generated HIP source (owned by the kernel object) — for inspection and tests */
const char *gl_gate_kernel_source(const void *kernel);

typedef struct GlQuotientArgs {
    const uint64_t *d_wires_leaves;
    const uint64_t *d_constants_sigmas_leaves;
    const uint64_t *d_zs_partial_products_leaves;
    uint32_t wires_leaf_len, constants_sigmas_leaf_len, zs_partial_products_leaf_len;
    const uint64_t *d_k_is;
    const uint64_t *d_gate_constraint_terms; /* may be NULL */
    const uint64_t *h_betas, *h_gammas, *h_alphas; /* HOST, num_challenges each */
    uint32_t num_constants, num_routed_wires, num_challenges, num_gate_constraints;
    uint32_t degree_bits, rate_bits, quotient_degree_factor;
    uint64_t coset_shift; /* F::coset_shift() = 7 */
    const GlGateProgram *gate_program; /* HOST struct, may be NULL; exclusive with d_gate_constraint_terms */
    /* 0: the three d_*_leaves are leaf-major rows [n_ext][leaf_len] (d_leaves of gl_commit_*);
     * otherwise they are the column-major LDE [leaf_len][column_stride] in bit-reversed row order
     * (d_lde of gl_commit_*) — coalesced reads, and no leaf-major copy has to exist at all. Any value
     * >= 2^degree_bits << log2_ceil(quotient_degree_factor), the rows the kernel reads, is a legal column pitch (the padded
     * pitch of gl_coset_lde_batch's dst_stride); a smaller non-zero one is GL_E_INVALID. */
    uint64_t column_stride;
    /* Gates compiled by gl_gate_kernel_build (may be NULL; exclusive with the two other sources of gate
     * constraints). Needs h_public_inputs_hash (4, host) and d_gate_workspace
     * [num_challenges][n << log2_ceil(qdf)] (device scratch). */
    const void *gate_kernel;
    const uint64_t *h_public_inputs_hash;
    uint64_t *d_gate_workspace;
} GlQuotientArgs;
GlError gl_compute_quotient_polys(const GlQuotientArgs *args, uint64_t *d_quotient_polys, void *ctx);

/* Evaluate poly_num base-field polynomials (coefficients [poly_num][2^log_n], column stride `stride`)
 * at num_points (<= 4) points of the quadratic extension F_p[X]/(X^2 - 7): what OpeningSet::new does
 * with every commitment's `polynomials` at zeta and g*zeta (plonky2/src/plonk/proof.rs:305-334;
 * p.to_extension().eval(z), field/src/polynomial/mod.rs:161-166; extension/quadratic.rs:173-185).
 * h_points: HOST array of num_points pairs (c0, c1) meaning c0 + c1*X.
 * d_out[(q*poly_num + i)*2 + {0,1}] = polynomial i at point q, canonical. */
GlError gl_eval_polys_ext2(const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint64_t stride, const uint64_t *h_points,
                           uint32_t num_points, uint64_t *d_out, void *ctx);

/* ---- FRI opening pipeline primitives (PolynomialBatch::prove_openings, plonky2/src/fri/oracle.rs:1047-1112;
 * fri_proof, plonky2/src/fri/prover.rs). Extension-field vectors (F_p[X]/(X^2-7)) are PLANAR on the
 * device: v[0..len) first components, v[len..2len) second components, so that every transform of an
 * extension polynomial is two columns of gl_ntt_batch / gl_coset_lde_batch. Host-side scalars
 * (h_alpha, h_point, h_scale, h_beta) are pairs (c0, c1).
 *
 * gl_fri_reduce_polys_base: d_out = sum_j alpha^j * poly_j (ReducingFactor::reduce_polys_base,
 *   util/reducing.rs:83-95); d_poly_ptrs is a DEVICE array of num_polys device pointers to base
 *   polynomials of n coefficients each.
 * gl_fri_divide_by_linear: q = (p(X) - p(z))/(X - z) (polynomial/division.rs:75-88) of the composition
 *   polynomial (destroyed), written shifted by one: final[0] = 0, final[i+1] = (accumulate ?
 *   final[i+1]*scale : 0) + q_i  — the update `alpha.shift_poly(&mut final_poly); final_poly += quotient`
 *   plus the multiplication by X of oracle.rs:1069-1087.
 * gl_fri_fold: out[k] = sum_{i < 2^arity_bits} c[k*2^arity_bits + i] * beta^i (prover.rs:103-111).
 * gl_ext2_interleave: rows[2i + c] = plane_c[i] (flatten(), prover.rs:90-95): consecutive groups of
 *   `arity` extension values become the Merkle leaves of a commit-phase tree (gl_merkle_tree_from_leaves
 *   with leaf_len = 2*arity).
 * gl_fri_proof_of_work (SYNCHRONOUS): h_state = the challenger's sponge state with its buffered inputs
 *   already written, witness_pos = input_buffer.len(); returns the SMALLEST witness w such that
 *   permute(state with state[witness_pos] = w)[7] has >= min_leading_zeros leading zero bits
 *   (prover.rs:122-171; the reference's rayon find_any returns an arbitrary one). */
GlError gl_fri_reduce_polys_base(const uint64_t *const *d_poly_ptrs, uint32_t num_polys, uint64_t n, const uint64_t *h_alpha,
                                 uint64_t *d_out, void *ctx);
GlError gl_fri_divide_by_linear(uint64_t *d_composition, uint64_t n, const uint64_t *h_point, const uint64_t *h_scale, int accumulate,
                                uint64_t *d_final, void *ctx);
GlError gl_fri_fold(const uint64_t *d_coeffs, uint64_t len, uint32_t arity_bits, const uint64_t *h_beta, uint64_t *d_out, void *ctx);
/* The same with beta read from device memory (two canonical words, e.g. where gl_challenger_step wrote them): the FRI commit phase
 * (fri/prover.rs:77-120) runs without a host synchronisation per layer. */
GlError gl_fri_fold_device(const uint64_t *d_coeffs, uint64_t len, uint32_t arity_bits, const uint64_t *d_beta, uint64_t *d_out, void *ctx);
GlError gl_ext2_interleave(const uint64_t *d_planes, uint64_t len, uint64_t *d_rows, void *ctx);
GlError gl_fri_proof_of_work(const uint64_t *h_state, uint32_t witness_pos, uint32_t min_leading_zeros, uint64_t *h_witness, void *ctx);
/* The same against a device-resident Challenger: the duplex state is the challenger's (its input buffer written over the state's
 * first words, the candidate behind it, fri/prover.rs:137-147); the witness lands in *d_witness (from where gl_challenger_step can
 * observe it) and in *h_witness. Synchronous like gl_fri_proof_of_work. */
GlError gl_fri_proof_of_work_device(const uint64_t *d_challenger, uint32_t min_leading_zeros, uint64_t *d_witness, uint64_t *h_witness, void *ctx);

/* count Poseidon permutations in place, states[count][12] (plonky2/src/hash/poseidon.rs:602-616). */
GlError gl_poseidon_permute_batch(uint64_t *d_states, uint64_t count, void *ctx);

/* The transcript's sponge: h_state[12] (in/out, host) absorbs n_blocks full rate-8 blocks of h_inputs in
 * overwrite mode, one permutation per block — Challenger::duplexing (plonky2/src/iop/challenger.rs:131-149)
 * repeated, and hash_n_to_hash_no_pad (hash/hashing.rs:81-108) for whole blocks. SYNCHRONOUS. */
GlError gl_sponge_absorb(uint64_t *h_state, const uint64_t *h_inputs, uint32_t n_blocks, void *ctx);

/* The Challenger with its state in DEVICE memory (plonky2/src/iop/challenger.rs:19-149): d_challenger = 32 u64 the caller owns
 * (sponge state, input buffer, the two buffer lengths). One call = one launch, asynchronous on ctx->stream, no host round trip:
 * observe_elements over up to eight device sources in order — read where the producing kernels left them: a cap straight from
 * gl_commit_* / gl_merkle_tree_*, openings from gl_eval_polys_ext2, a planar extension vector (planar_len != 0: element i is
 * d_ptr[(i & 1) * planar_len + (i >> 1)], i.e. observe_extension_elements) — then get_n_challenges(n_challenges) into d_out
 * (canonical). GL_CHALLENGER_RESET starts from the empty transcript (Challenger::new) before observing. GL_CHALLENGER_HASH:
 * instead of challenges, d_out[0..4) = hash_n_to_hash_no_pad of everything observed since the reset (hash/hashing.rs:81-108; use it
 * with GL_CHALLENGER_RESET on a scratch challenger). Values a host holds (circuit digest, public inputs) are observed from a device
 * copy. The host fetches the challenges it needs itself with one gl_memcpy_d2h per step; kernels that can read a challenge from
 * device memory need no fetch at all (gl_fri_fold_device, gl_merkle_open_batch_device, gl_fri_proof_of_work_device). d_out, when
 * given, must not overlap the 32 words of d_challenger (GL_E_INVALID): the step writes its outputs before it stores the transcript. */
typedef struct GlObserveSrc {
    const uint64_t *d_ptr;
    uint64_t count;      /* field elements observed from this source */
    uint64_t planar_len; /* 0: d_ptr[i]; GL_OBSERVE_KECCAK_DIGESTS: see below; else the plane length of an extension vector kept
                          * as [2][planar_len] */
} GlObserveSrc;
/* Reserved value of planar_len: d_ptr holds Keccak digests in their 32-byte slots (a cap or a digest of the `_h` trees) and the
 * source is observed as Challenger::observe_hash::<KeccakHash<25>> / observe_cap do (BytesHash<25>::to_vec, hash/hash_types.rs:
 * 179-189): element i is chunk i & 3 of slot i >> 2 — bytes 7c .. 7c+6 for c < 3, bytes 21 .. 24 for c = 3, little endian, zero
 * extended. `count` stays "field elements observed", four per digest: one that is no multiple of 4 is GL_E_INVALID. Bytes 25..31
 * of a slot are never read into the transcript. */
#define GL_OBSERVE_KECCAK_DIGESTS UINT64_MAX
#define GL_CHALLENGER_RESET 1u
#define GL_CHALLENGER_HASH 2u
/* Challenger::compact() (challenger.rs:149-155) before observing, as GL_CHALLENGER_RESET acts before observing: a non-empty input
 * buffer is duplexed, then the output buffer is cleared. */
#define GL_CHALLENGER_COMPACT 4u
GlError gl_challenger_step(uint64_t *d_challenger, const GlObserveSrc *h_srcs, uint32_t n_srcs, uint32_t n_challenges, uint64_t *d_out,
                           uint32_t flags, void *ctx);

/* MerkleTree::prove (plonky2/src/hash/merkle_tree.rs:392-440) and the leaf itself for `count` leaf
 * indices in one launch and one copy — what fri_prover_query_round (fri/prover.rs:199-260) does per
 * query and tree. Element j of leaf i is read at d_leaves[i*row_stride + j*elem_stride] (leaf-major rows:
 * (leaf_len, 1); the LDE's columns: (1, col_stride), col_stride >= n_leaves the column pitch). Host outputs: h_out_leaves[count][leaf_len],
 * h_out_siblings[count][log2(n_leaves) - cap_height][4]. SYNCHRONOUS. */
GlError gl_merkle_open_batch(const uint64_t *d_leaves, uint64_t row_stride, uint64_t elem_stride, uint32_t leaf_len, uint64_t n_leaves,
                             uint32_t cap_height, const uint64_t *d_digests, const uint64_t *h_indices, uint32_t count,
                             uint64_t *h_out_leaves, uint64_t *h_out_siblings, void *ctx);
/* The same with everything in device memory and nothing synchronised: leaf of query q = (d_indices[q] mod (n_leaves << index_shift))
 * >> index_shift — d_indices may be raw challenges (fri/prover.rs:186-190: x_index = challenge mod lde size) and index_shift the
 * sum of the FRI arities before this layer's tree (:213-236). Outputs [count][leaf_len] and [count][layers][4] in device memory. */
GlError gl_merkle_open_batch_device(const uint64_t *d_leaves, uint64_t row_stride, uint64_t elem_stride, uint32_t leaf_len, uint64_t n_leaves,
                                    uint32_t cap_height, const uint64_t *d_digests, const uint64_t *d_indices, uint32_t count,
                                    uint32_t index_shift, uint64_t *d_out_leaves, uint64_t *d_out_siblings, void *ctx);

/* MerkleTree::new (plonky2/src/hash/merkle_tree.rs:283-319) over n_leaves (power of two) leaves of
 * leaf_len elements; leaf hash = hash_or_noop (plonk/config.rs:56-67).
 *   _columns: d_cols[j*col_stride + i] = element j of leaf i   (the NTT's output layout)
 *   _leaves : d_rows[i*leaf_len + j]                            (the reference's Vec<Vec<F>>)
 * d_digests: 4*2*(n_leaves - 2^cap_height) u64, reference layout (merkle_tree.rs:46-54);
 * d_cap: 4*2^cap_height u64. cap_height > log2(n_leaves) -> GL_E_INVALID (the reference panics).
 * col_stride >= n_leaves, odd or even (the columns are read word by word; d_cols 8-byte aligned); a smaller one would make the
 * columns overlap: GL_E_INVALID. The one exception is leaf_len <= 1, where col_stride is not used and may be anything. */
GlError gl_merkle_tree_from_columns(const uint64_t *d_cols, uint32_t leaf_len, uint64_t n_leaves, uint64_t col_stride,
                                    uint32_t cap_height, uint64_t *d_digests, uint64_t *d_cap, void *ctx);
GlError gl_merkle_tree_from_leaves(const uint64_t *d_rows, uint32_t leaf_len, uint64_t n_leaves, uint32_t cap_height,
                                   uint64_t *d_digests, uint64_t *d_cap, void *ctx);

/* d_cols[c*col_stride + r] -> d_rows[r*n_cols + c]  (plonky2/src/util/mod.rs:23-53). col_stride >= n_rows, odd or even;
 * a smaller one is GL_E_INVALID, except for n_cols <= 1, where it is not used. */
GlError gl_transpose(const uint64_t *d_cols, uint64_t *d_rows, uint32_t n_cols, uint64_t n_rows, uint64_t col_stride,
                     void *ctx);

/* The pack step of a commitment whose columns are sharded over `world` GPUs (one process per GPU; plonky2_gpu_amd/dist.py):
 * d_out[(q*n_cols + c)*leaves_per_rank + i] = d_lde[c*col_stride + q*leaves_per_rank + i] — for every rank q, the leaf
 * range it will hash of every one of this rank's n_cols LDE columns, contiguous per destination rank, in ONE launch
 * (d_out: world * n_cols * leaves_per_rank elements). The slices go out as they are with one send per peer.
 * leaves_per_rank and col_stride even, col_stride >= world * leaves_per_rank, both buffers 16-byte aligned (else GL_E_INVALID). */
GlError gl_pack_leaf_ranges(const uint64_t *d_lde, uint64_t col_stride, uint32_t n_cols, uint64_t leaves_per_rank, uint32_t world,
                            uint64_t *d_out, void *ctx);

/* PolynomialBatch::from_coeffs (plonky2/src/fri/oracle.rs:911-977) without the host-side struct:
 *   d_coeffs   [poly_num][2^log_n]            in
 *   d_lde      [(poly_num+salt_size)][n_ext]  out, column-major, bit-reversed (n_ext = 2^(log_n+rate_bits));
 *              the salt_size trailing columns are the caller's input (caller-provided randomness,
 *              oracle.rs:998-1002), any representative: they are reduced in place, so that d_lde and d_leaves
 *              hold canonical words, and take part in the leaf hash. They are read by kernels on a stream of the library's own
 *              that starts behind everything queued on ctx's stream at the time of the call: write them on ctx's stream
 *              (gl_memcpy_*, a kernel launched there) or complete the writes before calling.
 *   d_leaves   [n_ext][poly_num+salt_size]    out, leaf-major (= merkle_tree.leaves); may be NULL. MAY overlap d_coeffs (the
 *              reference's caller passes one region for both, fri/oracle.rs:409-422): the coefficients are then consumed --
 *              the leaves replace them. d_lde must not overlap d_coeffs or d_leaves.
 *   d_digests / d_cap as gl_merkle_tree_*.
 * shift is F::coset_shift() = 7 in the reference (field/src/types.rs:431-433). */
GlError gl_commit_from_coeffs(const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                              uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde,
                              uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap, void *ctx);
/* PolynomialBatch::from_values (oracle.rs:709-731): d_values is transformed IN PLACE into the
 * coefficients (= PolynomialBatch.polynomials), then as gl_commit_from_coeffs. The arguments are checked before the transform:
 * a call refused with GL_E_INVALID leaves d_values as it was (with either hasher of gl_commit_from_values_h). */
GlError gl_commit_from_values(uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                              uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde,
                              uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap, void *ctx);

/* ---- Keccak Merkle trees and commits: plonky2's KeccakGoldilocksConfig (plonk/config.rs:110-128) -----------------
 * The two GenericConfigs of plonky2 differ in the Hasher that builds Merkle trees only: PoseidonHash or KeccakHash<25>
 * (hash/keccak.rs:53-83); field, extension, challenger and the public-input hash are the same. The `_h` entry points below
 * are the un-suffixed ones with that hasher as their first argument; GL_HASHER_POSEIDON forwards to the un-suffixed call
 * (same bytes out), an unknown value is GL_E_INVALID. With GL_HASHER_KECCAK25:
 *   hash_no_pad(x)   = the first 25 bytes of Keccak-256 (original padding 0x01 .. 0x80, rate 136 bytes = 17 elements) of the
 *                      canonical words of x, little endian (util/serialization.rs:492-509); inputs may be any u64
 *                      representative, they are reduced before they are absorbed;
 *   two_to_one(l, r) = the first 25 bytes of Keccak-256 of the 50 bytes l || r;
 *   hash_or_noop(x)  = len <= 3: the canonical words, zero padded to 25 bytes; len >= 5: hash_no_pad; len == 4: the
 *                      reference panics (a 32-byte slice of a 25-byte vector, plonk/config.rs:58-63): GL_E_INVALID, nothing written.
 * DEVICE LAYOUT OF A DIGEST: a 32-byte slot (4 u64), bytes 0..24 the hash, bytes 25..31 zero. With that, every buffer size
 * (d_digests: 4*2*(n_leaves - 2^cap_height) u64, d_cap: 4*2^cap_height u64), every digest index, gl_merkle_open_batch /
 * gl_merkle_open_batch_device (siblings [count][layers][4], one slot each) and the region contract arithmetic are those of the
 * Poseidon trees, unchanged. A host reads a hash as the first 25 bytes of its slot.
 * The `_h` commits keep the whole contract of gl_commit_*: d_lde and d_leaves do not depend on the hasher, d_leaves may be NULL
 * or overlap d_coeffs, salt columns are reduced in place and hashed, the caller's stream continues only after the tree (and the
 * leaves), and a failing call leaves no work running on a stream other than the caller's own.
 * A whole proof with this hasher: gl_circuit_create_h below. Not covered: the reference's seven symbols are Poseidon-only. */
enum GlHasher { GL_HASHER_POSEIDON = 0, GL_HASHER_KECCAK25 = 1 };
/* count inputs of len elements at d_inputs[i*stride ..), stride >= len when count > 1; d_out[count][4] in the slot layout above.
 * d_out 16-byte aligned. Always hash_no_pad, whatever len (0 included: the hash of the empty message). */
GlError gl_keccak_hash_no_pad_batch(const uint64_t *d_inputs, uint32_t len, uint64_t stride, uint64_t count, uint64_t *d_out, void *ctx);
GlError gl_merkle_tree_from_columns_h(uint32_t hasher, const uint64_t *d_cols, uint32_t leaf_len, uint64_t n_leaves, uint64_t col_stride,
                                      uint32_t cap_height, uint64_t *d_digests, uint64_t *d_cap, void *ctx);
GlError gl_merkle_tree_from_leaves_h(uint32_t hasher, const uint64_t *d_rows, uint32_t leaf_len, uint64_t n_leaves, uint32_t cap_height,
                                     uint64_t *d_digests, uint64_t *d_cap, void *ctx);
GlError gl_commit_from_coeffs_h(uint32_t hasher, const uint64_t *d_coeffs, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                                uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde,
                                uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap, void *ctx);
GlError gl_commit_from_values_h(uint32_t hasher, uint64_t *d_values, uint64_t poly_num, uint32_t log_n, uint32_t rate_bits,
                                uint32_t cap_height, uint32_t salt_size, uint64_t shift, uint64_t *d_lde,
                                uint64_t *d_leaves, uint64_t *d_digests, uint64_t *d_cap, void *ctx);

/* ---- the whole prover in two calls ---------------------------------------------------------------
 * gl_circuit_create = the prover-side part of CircuitBuilder::build (plonky2/src/plonk/circuit_builder.rs:
 * 849-960): uploads sigmas / k_is, commits constants||sigmas (constants_sigmas_commitment), derives the
 * circuit digest (:915-927, empty domain separator) unless one is given, and compiles the gate programs.
 * gl_prove = prove() (plonky2/src/plonk/prover.rs:40-233) from the full witness on: d_wires is the flat
 * [num_wires][2^degree_bits] matrix of wire values in HBM (MatrixWitness::my_wire_values,
 * iop/witness.rs:351-362; left untouched). The proof comes back in the reference's wire format
 * (write_proof_with_public_inputs, util/serialization.rs:674-689) in a malloc'd buffer (gl_bytes_free).
 * h_stage_ms (optional, GL_PROVE_STAGES doubles) receives per-stage wall times with a device
 * synchronisation at each boundary: wires commit, partial products, Z/pp commit, quotient, quotient
 * commit, opening set, FRI combine, FRI commit phase, proof of work, query rounds, serialisation. */
typedef struct GlFriParams {
    uint32_t rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    uint32_t num_reductions;
    const uint32_t *reduction_arity_bits; /* host, num_reductions */
    uint32_t hiding; /* FriParams::hiding = CircuitConfig::zero_knowledge (fri/mod.rs:64-65, plonk/circuit_data.rs:74): the wires, Zs /
                      * partial products and quotient commitments carry SALT_SIZE = 4 random elements per leaf (fri/oracle.rs:41,
                      * 985-1002); such a circuit is proved with gl_prove_zk */
} GlFriParams;
typedef struct GlCircuitDesc {
    uint32_t struct_size; /* = sizeof(GlCircuitDesc) of the header the caller was compiled against. The struct embeds GlFriParams by
                           * value and has grown before (`hiding`, round 4): a caller built against another layout gets GL_E_INVALID
                           * from gl_circuit_create instead of shifted fields. (A caller of the 0.3 layout passes its degree_bits here,
                           * which no size equals.) */
    uint32_t degree_bits, num_wires, num_routed_wires, num_constants, num_challenges, quotient_degree_factor;
    uint32_t num_gate_constraints;
    GlFriParams fri;
    const uint64_t *h_k_is;      /* num_routed_wires */
    const uint64_t *h_constants; /* [num_constants][n] value columns, selectors first */
    const uint64_t *h_sigmas;    /* [num_routed_wires][n] value columns */
    const GlGateInstr *h_instrs;
    uint32_t num_instrs;
    const GlGateDesc *h_gates;
    uint32_t num_gates;
    const uint64_t *h_immediates;
    uint32_t num_immediates, num_selectors;
    int compile_gates;                /* 1: run-time compiled kernel, 0: interpreter */
    const uint64_t *h_circuit_digest; /* 4, or NULL to derive it */
} GlCircuitDesc;
#define GL_PROVE_STAGES 11
GlError gl_circuit_create(const GlCircuitDesc *desc, void **circuit, void *ctx);
/* The circuit of a GenericConfig whose Hasher is `hasher` (enum GlHasher): GL_HASHER_POSEIDON forwards to gl_circuit_create, an
 * unknown value is GL_E_INVALID and *circuit is not written. The handle carries its hasher: gl_prove, gl_prove_zk, gl_prove_many,
 * gl_circuit_trim and gl_circuit_info take it as they take a Poseidon one. With GL_HASHER_KECCAK25 (KeccakGoldilocksConfig,
 * plonk/config.rs:120-128: Hasher = KeccakHash<25>, InnerHasher = PoseidonHash) prove() differs from the Poseidon one in this:
 *   - every Merkle tree — constants / sigmas, wires, Zs / partial products, quotient chunks, the FRI commit phase — is a Keccak
 *     tree (the `_h` calls above); Merkle openings are the same, one 32-byte slot per sibling;
 *   - the Challenger, the public-inputs hash, the proof of work and the query indices stay Poseidon (prover.rs:96, fri/prover.rs:
 *     122-171), but observe_hash / observe_cap observe BytesHash<25>::to_vec(): four elements per hash, its bytes in chunks of
 *     7, 7, 7 and 4 (GL_OBSERVE_KECCAK_DIGESTS) — the circuit digest, the three caps and every FRI cap;
 *   - the circuit digest (circuit_builder.rs:915-927) is Keccak hash_no_pad(cap.flatten() || hash_pad([]).to_vec() || degree_bits);
 *     h_circuit_digest, if given, is one 32-byte slot, and gl_circuit_info returns slots (digest: 4 u64, cap: 4 << cap_height u64;
 *     VerifierOnlyCircuitData's hashes are the first 25 bytes of each);
 *   - write_hash writes 25 bytes (util/serialization.rs:537-543): a cap is 2^cap_height x 25 bytes, a Merkle proof its length byte
 *     and 25 bytes per sibling.
 * KeccakHash<25>::hash_or_noop panics on a leaf of exactly 4 elements (plonk/config.rs:56-63), so a circuit that would build one
 * is refused HERE with GL_E_INVALID, the message naming the cause, before anything is allocated: a commitment whose leaves have 4
 * elements, salt included (e.g. num_challenges * quotient_degree_factor = 4 without hiding), or a FRI reduction with arity_bits = 1
 * (leaves of 2 extension elements). */
GlError gl_circuit_create_h(uint32_t hasher, const GlCircuitDesc *desc, void **circuit, void *ctx);
void gl_circuit_destroy(void *circuit);
/* gl_prove recycles its working buffers from proof to proof of the same circuit (one proof's worth of
 * HBM stays attached to the circuit PER CONTEXT that proves with it: ~10 GB at n = 2^18 with 234 wires, plus a
 * page-locked staging buffer of a few hundred KiB for what travels between host and device). gl_circuit_trim
 * releases them without destroying the circuit; the next proof allocates again. Call it only between proofs.
 * Since 0.6 the proof's transcript lives in device memory (gl_challenger_step): gl_prove synchronises with the
 * device where the HOST computes with a challenge (betas / gammas, alphas, zeta, the FRI alpha), for the
 * proof-of-work witness, and once for everything that goes into the proof bytes. */
GlError gl_circuit_trim(void *circuit);
/* circuit digest (4) and constants_sigmas cap (4 << cap_height): what VerifierOnlyCircuitData holds (a Keccak circuit: digest slots) */
GlError gl_circuit_info(const void *circuit, uint64_t *h_digest, uint64_t *h_constants_sigmas_cap);
GlError gl_prove(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                 uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx);
/* prove() of a circuit built with zero_knowledge = true (fri.hiding != 0): the three blinded commitments — wires, Zs / partial
 * products, quotient chunks (plonk/prover.rs:84, 125, 174; PlonkOracle::*.blinding, plonk/plonk_common.rs:20-44) — get SALT_SIZE = 4
 * extra elements per leaf, which the proof's initial-tree openings carry and the verifier strips (fri/proof.rs:45-52).
 * The reference draws them from OsRng (F::rand_vec, fri/oracle.rs:998-1002); here the randomness is the CALLER's:
 *   d_salts  [3][4][n_ext] uniform field elements, any u64 representative (words >= p are reduced on their way into the commitment, so
 *            the proof carries canonical words like the reference's rand_vec output) (n_ext = 2^(degree_bits + rate_bits)): block 0 for the wires commitment, 1 for
 *            Zs / partial products, 2 for the quotient; column k of a block is element k of the salt of every leaf, in LEAF order
 *            (entry j belongs to leaf j, the leaf of the LDE point bitrev(j)).
 * gl_prove on a hiding circuit and gl_prove_zk on a non-hiding one return GL_E_INVALID. */
/* `count` independent proofs of ONE circuit with `in_flight` of them at a time — the per-GPU unit of a batch of proofs (a
 * throughput job: one proof alone leaves the chip idle or at one wavefront in its latency-bound phases — transcript, small tree
 * layers, openings; a second one in flight fills them: 1.15 x the proofs per second at the ed25519 shape). Worker w, a host thread
 * the call starts, proves witnesses w, w + in_flight, .. on ctxs[w] (in_flight distinct contexts of the circuit's device, each
 * with its own 512 MiB workspace); d_wires[i] / h_public_inputs[i] / proofs[i] / proof_lens[i] belong to proof i, every proof is
 * what gl_prove gives for that witness alone; all or nothing on error. Not for hiding circuits (use gl_prove_zk per proof). */
GlError gl_prove_many(const void *circuit, const uint64_t *const *d_wires, const uint64_t *const *h_public_inputs, uint32_t num_public_inputs,
                      uint32_t count, uint8_t **proofs, uint64_t *proof_lens, void *const *ctxs, uint32_t in_flight);
GlError gl_prove_zk(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                    const uint64_t *d_salts, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx);
void gl_bytes_free(uint8_t *p);

/* ---- STARKs: starky's prove() in two calls --------------------------------------------------------
 * gl_stark_create describes a STARK (starky/src/stark.rs), gl_stark_prove = prove() (starky/src/prover.rs:32-195) of one trace:
 * trace commit, the permutation Z polynomials (permutation.rs) and their commit if the STARK has permutation pairs, the constraint
 * quotient, its commit, the openings at zeta and g * zeta and PolynomialBatch::prove_openings over the instance of stark.rs:88-137 —
 * the commit, tree, transcript and FRI code of gl_prove. This version of starky observes only the caps and the openings: neither a
 * digest of the STARK nor the public inputs enter the transcript.
 *
 * The constraints (Stark::eval_packed_generic) are ONE register program for the whole STARK in the GlGateInstr encoding above — its
 * 64 registers, its 4 ACC accumulators and their overflow contract — without GlGateDescs, selectors or filters. In a STARK program:
 *   0 LOAD_WIRE dst<-local_values[a]      2 LOAD_PI dst<-public_inputs[a] (the public inputs themselves, any number of them)
 *   3 LOAD_IMM  4 ADD  5 SUB  6 MUL  8 MULK  9 ACC  10 ACCR   as above         1 LOAD_CONST   invalid
 *   7 EMIT            consumer.constraint(r[a])                11 LOAD_NEXT dst<-next_values[a]
 *  12 EMIT_TRANSITION constraint(r[a] * z_last)                13 EMIT_FIRST_ROW constraint(r[a] * lagrange_first)
 *  14 EMIT_LAST_ROW   constraint(r[a] * lagrange_last)
 * Opcodes 11..14 exist in STARK programs only: gate programs refuse them as they refuse any unknown opcode. The consumer is starky's
 * (constraint_consumer.rs:53-76), not plonk's reduce_with_powers: for every challenge acc <- acc * alpha + constraint in emission
 * order. gl_stark_create validates the program once, on the host: no LOAD_CONST or unknown opcode, columns / public inputs /
 * immediates / registers in range, every register written before it is read, the ACC contract, at least one EMIT. The ACC contract
 * as enforced: per accumulator, the sum of weight * (2^32 - 1) over the ACCs since its last ACCR stays below 2^63 (weights are the
 * immediates reduced mod p, each below 2^32); the sum is kept in 128 bits, so that two weights near 2^32 are refused and do not
 * wrap to a small bound. A single weight 2^31 is the largest sum that passes; the four accumulators are bounded separately.
 *
 * Permutation pairs (PermutationPair::column_pairs): pair p is the column pairs h_pair_bounds[p] .. h_pair_bounds[p + 1] of
 * h_column_pairs, two words (lhs, rhs) each. The instances cartesian_product(pairs, 0..num_challenges) are batched by
 * quotient_degree_factor = max(1, constraint_degree - 1) into num_z = ceil(num_pairs * num_challenges / qdf) Z polynomials.
 *
 * fri.hiding must be 0 (starky: fri_params(degree_bits, false)); log2_ceil(qdf) <= fri.rate_bits; num_challenges <= 4; qdf <= 16.
 * With GL_HASHER_KECCAK25 a commitment with 4-element leaves (num_columns = 4, num_z = 4, num_challenges * qdf = 4) or a FRI
 * reduction with arity_bits = 1 is refused here, as by gl_circuit_create_h. Every refusal is GL_E_INVALID with a message, before
 * anything is allocated. */
typedef struct GlStarkDesc {
    uint32_t struct_size; /* = sizeof(GlStarkDesc) of the header the caller was compiled against, as in GlCircuitDesc */
    uint32_t degree_bits, num_columns, num_public_inputs, constraint_degree, num_challenges;
    GlFriParams fri;
    const GlGateInstr *h_instrs;
    uint32_t num_instrs;
    const uint64_t *h_immediates;
    uint32_t num_immediates;
    const uint32_t *h_column_pairs; /* 2 * h_pair_bounds[num_pairs] words; NULL without pairs */
    const uint32_t *h_pair_bounds;  /* num_pairs + 1, starting at 0, non-decreasing; NULL without pairs */
    uint32_t num_pairs;
} GlStarkDesc;
/* h_stage_ms of gl_stark_prove: trace commit, permutation Zs, Z commit, quotient, quotient commit, openings, FRI combine, FRI commit
 * phase, proof of work, query rounds, serialisation */
#define GL_STARK_STAGES 11
GlError gl_stark_create(uint32_t hasher, const GlStarkDesc *desc, void **stark, void *ctx);
void gl_stark_destroy(void *stark);
/* releases the recycled working buffers of the handle's proofs (one pool per context, as gl_circuit_trim); only between proofs */
GlError gl_stark_trim(void *stark);
/* d_trace: [num_columns][2^degree_bits] value columns, left untouched; h_public_inputs: num_public_inputs words. The proof comes
 * back in a malloc'd buffer (gl_bytes_free). WIRE FORMAT of StarkProofWithPublicInputs (the reference has no serializer for it):
 * the fields in struct order (starky/src/proof.rs:23-35, 129-135) with the primitives of plonky2/src/util/serialization.rs —
 *   trace_cap; permutation_zs_cap only if the STARK has pairs (no flag byte: the description decides); quotient_polys_cap —
 *     2^cap_height hashes each (write_hash: 4 field elements, or 25 bytes with GL_HASHER_KECCAK25);
 *   the openings, extension elements as two field elements: local_values, next_values, [permutation_zs, permutation_zs_next,]
 *     quotient_polys;
 *   the FRI proof exactly as write_fri_proof writes it (the bytes gl_prove emits for that part);
 *   the public inputs.
 * A trace that violates the constraints gives GL_E_INVALID "Quotient has failed..." where the reference's trim_to_len can fail
 * (qdf no power of two); otherwise, as in the reference, a proof that no verifier accepts. */
GlError gl_stark_prove(const void *stark, const uint64_t *d_trace, const uint64_t *h_public_inputs, uint8_t **proof, uint64_t *proof_len,
                       double *h_stage_ms, void *ctx);
/* The two kernels of gl_stark_prove alone, with host challenges. h_challenges: the qdf challenge sets in the order they are drawn
 * (permutation.rs:153-179): (beta, gamma) of set s, challenge c at h_challenges[2 * (s * num_challenges + c)].
 * gl_stark_permutation_zs: d_trace value columns at pitch trace_stride >= n -> d_zs [num_z][n] value columns
 * (compute_permutation_z_polys). GL_E_INVALID for a STARK without pairs. The trace need not satisfy anything. A ZERO DENOMINATOR —
 * a row on which the product of a batch's right-hand sides gamma + sum_j beta^j row[rhs_j] vanishes — gives that row the quotient 0
 * (0^(p-2) = 0; the reference's batch inversion panics instead): Z[r + 1 ..] of that batch are all 0, no error is reported, and the
 * proof built on such Zs fails the permutation check at the verifier. */
GlError gl_stark_permutation_zs(const void *stark, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_challenges, uint64_t *d_zs,
                                void *ctx);
/* gl_stark_quotient_polys: compute_quotient_polys (prover.rs:199-319). d_trace_lde / d_zs_lde: the d_lde of gl_commit_from_values of
 * the trace and of the Zs (NULL without pairs), column-major at pitch column_stride >= n << rate_bits, rows in bit-reversed order;
 * h_alphas: num_challenges; h_challenges: as above (NULL without pairs); h_public_inputs: num_public_inputs.
 * d_quotient_polys [num_challenges][n << log2_ceil(qdf)] receives the COEFFICIENTS (after the coset_ifft). */
GlError gl_stark_quotient_polys(const void *stark, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde, uint64_t column_stride,
                                const uint64_t *h_alphas, const uint64_t *h_challenges, const uint64_t *h_public_inputs,
                                uint64_t *d_quotient_polys, void *ctx);

/* ---- Multi-table STARKs with cross-table lookups ---------------------------------------------------
 * gl_stark_tables_create describes num_tables STARKs (each a GlStarkDesc with its own degree_bits, columns, program, permutation
 * pairs and fri.reduction_arity_bits) tied together by cross-table lookups (CTLs); gl_stark_tables_prove is prove_with_traces
 * (evm/src/prover.rs:66-421) over cross_table_lookup_data / eval_cross_table_lookup_checks (evm/src/cross_table_lookup.rs) and the
 * three-batch FRI instance of evm/src/stark.rs:83-142. Nothing EVM-specific: the tables and the lookups are what the caller describes.
 *
 * A CTL COLUMN is constant + sum_j coeff_j * row[col_j] (Column::eval): CTL column k is the terms h_column_bounds[k] ..
 * h_column_bounds[k + 1] of (h_term_columns, h_term_coeffs) plus h_column_constants[k]; no terms = a constant column. Coefficients
 * and constants are any u64, reduced mod p. A TABLE-WITH-COLUMNS (TWC) t names table h_twc_table[t], the CTL columns
 * h_twc_column_bounds[t] .. h_twc_column_bounds[t + 1] and the filter h_twc_filter[t]: the index of a CTL column, or
 * GL_CTL_NO_FILTER. Term columns are columns of the TWC's table. LOOKUP l is the TWCs h_lookup_bounds[l] .. h_lookup_bounds[l + 1]:
 * the LAST one is the looked table, the others are looking. (A verifier's `default` row is not part of the description.)
 *
 * THE CTL Zs of a table, in order: for every lookup, for every challenge c in 0..num_challenges, the looking TWCs in order and then
 * the looked TWC each append one Z to the table they name. Z[i] = prod_{r <= i} s_r, s_r = gamma_c + sum_j beta_c^j column_j(row r)
 * where the filter evaluates to 1 (as a field element: a word p + 1 is 1) and s_r = 1 where it evaluates to 0 — the INCLUSIVE
 * prefix product (partial_products, :314-341). Any other filter value is GL_E_INVALID "Non-binary filter?". The Zs oracle of a
 * table holds its permutation Zs, then its CTL Zs; the quotient's constraints are the program's, then the permutation checks, then
 * per CTL Z, with select(f, x) = f x + 1 - f (f = 1 without a filter),
 *   constraint_first_row(z - select(filter(local), combine(local))), constraint_transition(z' - z select(filter(next), combine(next))).
 *
 * TRANSCRIPT: every trace is committed; a fresh Challenger observes all trace caps in table order and yields num_challenges (beta,
 * gamma) CTL challenges shared by all tables; then per table in order: compact(), the permutation challenge sets (with pairs), the
 * Zs cap, alphas, the quotient cap, zeta, the openings (zeta batch, zeta g batch, then ctl_zs_last lifted to (x, 0)), prove_openings.
 * The one Challenger runs on from table to table.
 *
 * gl_stark_tables_create refuses, with GL_E_INVALID and a message, before anything is allocated: whatever gl_stark_create refuses
 * for a table; tables that differ in num_challenges, rate_bits, cap_height, proof_of_work_bits, num_query_rounds or hiding
 * (reduction_arity_bits may differ); a table with public inputs; a table no lookup names ("No CTL?"); indices out of range; a
 * lookup without a looking TWC, with unequal column counts or with filters on some of its TWCs only; constraint_degree < 3 for a
 * table with a filtered CTL Z, < 2 with an unfiltered one; with GL_HASHER_KECCAK25 a Zs oracle of exactly 4 polynomials. */
#define GL_CTL_NO_FILTER 4294967295u
typedef struct GlStarkTablesDesc {
    uint32_t struct_size; /* = sizeof(GlStarkTablesDesc) */
    uint32_t num_tables;
    const GlStarkDesc *tables;
    const uint32_t *h_term_columns;
    const uint64_t *h_term_coeffs;
    const uint32_t *h_column_bounds; /* num_ctl_columns + 1, starting at 0, non-decreasing */
    const uint64_t *h_column_constants;
    uint32_t num_ctl_columns;
    const uint32_t *h_twc_table, *h_twc_column_bounds /* num_twcs + 1 */, *h_twc_filter;
    uint32_t num_twcs;
    const uint32_t *h_lookup_bounds; /* num_lookups + 1 */
    uint32_t num_lookups;
} GlStarkTablesDesc;
GlError gl_stark_tables_create(uint32_t hasher, const GlStarkTablesDesc *desc, void **tables, void *ctx);
void gl_stark_tables_destroy(void *tables);
GlError gl_stark_tables_trim(void *tables);
/* d_traces[k]: the trace of table k, [num_columns][2^degree_bits] value columns, left untouched. h_stage_ms: NULL or
 * [num_tables][GL_STARK_STAGES], the stages of gl_stark_prove per table; stage 1 of a table is its permutation Zs plus its CTL Zs.
 * All trace commitments stay alive until their table is proved: HBM use is the sum of the tables' trace LDEs plus one table's
 * working set. WIRE FORMAT: the tables' StarkProofs (evm/src/proof.rs:103-257) in table order, each
 *   trace_cap, permutation_ctl_zs_cap (always present), quotient_polys_cap;
 *   the openings: local_values, next_values, permutation_ctl_zs, permutation_ctl_zs_next as extension elements; ctl_zs_last (the
 *     CTL Zs only, at 1 / g), ONE field element each; quotient_polys as extension elements;
 *   the FRI proof as write_fri_proof writes it.
 * There are no public inputs. The non-binary filter is reported at the proof's next host synchronisation. */
GlError gl_stark_tables_prove(const void *tables, const uint64_t *const *d_traces, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms,
                              void *ctx);
/* The two kernels alone, synchronous, with host challenges. h_ctl_challenges: (beta, gamma) of challenge c at [2 c].
 * gl_stark_tables_ctl_zs: d_trace value columns of table `table` at pitch trace_stride >= n -> d_zs [num CTL Zs of the table][n]
 * value columns; GL_E_INVALID "Non-binary filter?" as above. gl_stark_tables_quotient_polys: gl_stark_quotient_polys of that table
 * with the CTL checks; d_zs_lde holds the permutation Zs, then the CTL Zs; h_perm_challenges NULL without pairs. A filter's LDE
 * is not binary off the subgroup: the quotient evaluates select() as written and reports nothing. */
GlError gl_stark_tables_ctl_zs(const void *tables, uint32_t table, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_ctl_challenges,
                               uint64_t *d_zs, void *ctx);
GlError gl_stark_tables_quotient_polys(const void *tables, uint32_t table, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde,
                                       uint64_t column_stride, const uint64_t *h_alphas, const uint64_t *h_perm_challenges,
                                       const uint64_t *h_ctl_challenges, uint64_t *d_quotient_polys, void *ctx);

/* ---- A STARK's constraints compiled into a kernel of their own (opt-in) ----------------------------
 * By default the quotient INTERPRETS the register program per LDE point. gl_stark_compile turns the handle's description — the
 * program, the permutation checks and, for a table, its CTL checks — into straight-line HIP source for one kernel specialised to
 * that STARK (registers in VGPRs, immediates, ACC weights, column indices, CTL terms and coefficients as literals), compiles it
 * with hiprtc for gfx950 and uses it from then on wherever the handle computes a quotient. The values are the interpreter's bit
 * for bit. Code objects are kept where the gate kernels' are: $PLONKY2_HIP_KERNEL_CACHE (empty = no cache), else the directory
 * kernel_cache next to the library if it exists; files stark_<hash of source, hiprtc version, target>.hsaco with the source in
 * .hip next to it; $PLONKY2_HIP_KERNEL_CACHE_LIST receives their paths. A compiled handle is used by several host threads on
 * several contexts at once, as an interpreted one.
 *
 * Compile the handle's quotient kernel(s) and use them from now on in gl_stark_prove / gl_stark_quotient_polys
 * (gl_stark_tables_prove / gl_stark_tables_quotient_polys). Only between proofs, like gl_stark_trim. A second call is a no-op.
 * On failure (hiprtc / module load) the message carries the compiler's log and the handle stays interpreted and usable. */
GlError gl_stark_compile(void *stark, void *ctx);
GlError gl_stark_tables_compile(void *tables, void *ctx); /* one kernel per table; compile side by side, at most 8 threads */
int gl_stark_is_compiled(const void *stark);
int gl_stark_tables_is_compiled(const void *tables);
const char *gl_stark_kernel_source(const void *stark); /* NULL unless compiled */
const char *gl_stark_tables_kernel_source(const void *tables, uint32_t table);
/* Device-free: validate exactly as gl_stark_create / gl_stark_tables_create do, generate, compile into the kernel cache.
 * No context, no allocation, no module load — what a build machine without a GPU runs so that *_compile finds its kernels.
 * GL_E_INVALID also where there is no kernel cache to compile into. */
GlError gl_stark_precompile(uint32_t hasher, const GlStarkDesc *desc);
GlError gl_stark_tables_precompile(uint32_t hasher, const GlStarkTablesDesc *desc);

/* ---- ... as several kernel units (for long programs) ------------------------------------------------
 * hiprtc's compile time is superlinear in the length of one kernel's straight-line body, so a program of tens of thousands of
 * instructions (the Keccak-f table's 47 227) cannot be compiled as one kernel in reasonable time. The *_units calls cut the
 * description into UNITS of at most max_unit_instrs instructions each and compile one kernel per unit; the kernels run in order
 * on the call's stream and hand the constraint consumer's running sums on through the call's own output buffer, so the quotient
 * is still the interpreter's bit for bit. max_unit_instrs = 0: the library's default cap (1000; DESIGN.md 3.7.3 has the
 * measurements behind it).
 *   * The program is cut by gl_stark_split_program's rule (below). The permutation checks and a table's CTL checks follow the
 *     program in the consumer's order; a check counts the field operations it generates; they go into the last program unit
 *     while they fit under the cap and into further units otherwise. One CTL Z's pair of constraints is never cut.
 *   * One stark_<hash>.hsaco + .hip per distinct unit source in the kernel cache; all units (of all tables) compile side by
 *     side on at most 8 threads. Failure is all or nothing: the handle stays interpreted and usable.
 *   * A handle compiled in units is used by several host threads on several contexts at once like any other.
 * gl_stark_compile / gl_stark_tables_compile / gl_stark_precompile / gl_stark_tables_precompile keep producing ONE unit with the
 * sources and cache names they always had. On a handle that is already compiled every compile call is a no-op.
 * gl_stark_kernel_units: 0 while interpreted. gl_stark_kernel_unit_source: NULL unless compiled or beyond the units;
 * gl_stark_kernel_source is unit 0's. */
GlError gl_stark_compile_units(void *stark, uint32_t max_unit_instrs, void *ctx);
GlError gl_stark_tables_compile_units(void *tables, uint32_t max_unit_instrs, void *ctx);
GlError gl_stark_precompile_units(uint32_t hasher, const GlStarkDesc *desc, uint32_t max_unit_instrs);
GlError gl_stark_tables_precompile_units(uint32_t hasher, const GlStarkTablesDesc *desc, uint32_t max_unit_instrs);
int gl_stark_kernel_units(const void *stark);
int gl_stark_tables_kernel_units(const void *tables, uint32_t table);
const char *gl_stark_kernel_unit_source(const void *stark, uint32_t unit);
const char *gl_stark_tables_kernel_unit_source(const void *tables, uint32_t table, uint32_t unit);
/* The device-free splitter of desc's program (only the program, its immediates, num_columns and num_public_inputs are read and
 * validated as gl_stark_create validates them; max_unit_instrs = 0: the default cap). Unit k holds a contiguous run of the
 * program's EMIT* instructions, the runs partition all EMITs in order, and its body is the backward slice of its EMITs: every
 * instruction an EMIT transitively reads through "the latest write of that register", every ACC since the previous ACCR of an
 * accumulator whose ACCR is kept, in the original order with the original register numbers. A value live across a cut is
 * computed again in every unit that reads it. A unit grows constraint by constraint while its slice has at most max_unit_instrs
 * instructions; one constraint whose slice alone is longer is a unit of its own. max_unit_instrs >= num_instrs: one unit, the
 * input word for word. Every unit is a program gl_stark_create accepts with desc's immediates, columns and public inputs.
 * ONE result for all units, laid out and released as gl_keccak_table_program's (gl_gate_programs_free), with a descriptor per
 * unit: instrs = the units' programs one behind the other, immediates = desc's (shared, indices unchanged), num_gates = the
 * number of units, gates[k] = {row = k, selector_index = 0, group_start / group_end = the unit's EMITs are numbers group_start
 * .. group_end - 1 of the program's, prog_start, prog_len = the unit's instructions in instrs}, num_gate_constraints = the
 * program's EMITs. */
GlError gl_stark_split_program(const GlStarkDesc *desc, uint32_t max_unit_instrs, GlGatePrograms *out);

/* ---------------------------------------------------------------------------------------------
 * The lookup columns of a trace: the Halo2-style lookup argument of the reference's STARKs (evm/src/lookup.rs, used by its memory
 * table, memory_stark.rs:147, and by system_zero/src/lookup.rs). A lookup is four trace columns: the inputs, the table, and the
 * two columns that permuted_cols(inputs, table) (lookup.rs:67-131) fills. The constraints are eval_lookups (lookup.rs:13-34: a
 * program of LOAD_WIRE / LOAD_NEXT / SUB / MUL / EMIT / EMIT_LAST_ROW) and the two permutation pairs (input, permuted input) and
 * (table, permuted table) (memory_stark.rs:452-456). CONTRACT: inputs may be any u64 representatives, n is any length with
 * 1 <= n <= 2^30 (no power of two needed); every output is canonical; permuted_inputs is the inputs' canonical values in ascending
 * order; permuted_table is EXACTLY the reference's column, bit for bit: beside the first input of a run of equal values that the
 * table holds stands that value, and an input the table does not hold gets the table value the reference's serial merge gives it
 * — the unused table value pushed LAST before it (its stack is LIFO), or, where that stack is empty or the merge has ended, the
 * values left on the stack from the bottom, in order.
 * Everything runs on ctx->stream in call order and returns without waiting; nothing is allocated: the caller provides d_scratch
 * of gl_lookup_scratch_bytes(n) bytes (about 8.7 n words), 16-byte aligned, which holds nothing between calls. Refused with
 * GL_E_INVALID before anything is launched: n out of range, NULL pointers, an output that overlaps an input or the other output
 * (gl_sort_canonical: d_out == d_in is allowed, a partial overlap is not), and for gl_stark_fill_lookups a column index
 * >= num_columns, trace_stride < n, and a permuted column that is also an input, table or permuted column of a lookup of the call.
 * ------------------------------------------------------------------------------------------- */
uint64_t gl_lookup_scratch_bytes(uint64_t n);
/* canonical values of d_in[0..n) in ascending order -> d_out (d_out == d_in allowed) */
GlError gl_sort_canonical(const uint64_t *d_in, uint64_t *d_out, uint64_t n, void *d_scratch, void *ctx);
/* permuted_cols (evm/src/lookup.rs:67-131), bit for bit */
GlError gl_lookup_permuted_cols(const uint64_t *d_inputs, const uint64_t *d_table, uint64_t n, uint64_t *d_permuted_inputs,
                                uint64_t *d_permuted_table, void *d_scratch, void *ctx);
/* h_lookups: 4 words per lookup (input, table, permuted input, permuted table): columns of d_trace [num_columns][pitch trace_stride
 * >= n]; the two permuted columns are written, everything else is left untouched */
GlError gl_stark_fill_lookups(uint64_t *d_trace, uint64_t trace_stride, uint64_t n, uint32_t num_columns, const uint32_t *h_lookups,
                              uint32_t num_lookups, void *d_scratch, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * The Keccak-f table: the reference's KeccakStark (evm/src/keccak/: keccak_stark.rs, columns.rs, round_flags.rs, logic.rs,
 * constants.rs), the widest table of its multi-table prover — 2430 columns, 24 rows per permutation — with its trace built in
 * HBM and its constraints emitted natively, so that gl_stark_prove / gl_stark_tables_prove prove it without the trace ever
 * visiting the host.
 * gl_keccak_table_trace = generate_trace_rows (keccak_stark.rs:53-72). d_inputs: [num_inputs][25] words of 64 bits in device
 * memory, the Keccak-f[1600] states in the reference's order input[y * 5 + x]. d_trace receives [2430][pitch trace_stride] value
 * columns with n = 2^degree_bits rows, the layout gl_stark_prove takes. CONTRACT: rows 24 k .. 24 k + 23 are permutation k exactly
 * as generate_trace_rows_for_perm fills them; the rows from 24 num_inputs up to n are the permutation of the all-zero state,
 * repeated and cut off at n (pad_rows, then drain: a power of two is never a multiple of 24, so the last padding permutation is
 * always cut). Every word written is canonical — a bit, a 32-bit limb or a round flag —, and every one of the 2430 columns is
 * written on every row: the buffer need not be zeroed; the words between n and trace_stride are left untouched. Column indices
 * are those of columns.rs (reg_b is an alias into A' and has no columns of its own). The call runs on ctx->stream, returns
 * without waiting and allocates nothing. Refused with GL_E_INVALID and a message before anything is launched: degree_bits 0 or
 * above 24, 24 * num_inputs > n, trace_stride < n, a NULL pointer (num_inputs == 0 is allowed and gives an all-padding trace;
 * d_inputs may then be NULL), d_trace overlapping d_inputs.
 * gl_keccak_table_program = eval_packed_generic (keccak_stark.rs:230-375) with eval_round_flags as ONE STARK program in the
 * encoding of GlStarkDesc.h_instrs: 842 constraints of degree 3 in the reference's order (the order decides the powers of alpha
 * and so the proof's bytes), the bit recompositions through ACC in blocks that keep its overflow contract, rc_value_bit folded in
 * at emission. Device-free. It fills instrs, immediates and their counts; gates is NULL and num_gates 0; num_gate_constraints is
 * the number of emitted constraints; release the result with gl_gate_programs_free. The table has no public inputs and no
 * permutation pairs; its cross-table lookup (keccak_stark.rs:34-43) has the 50 input limbs then the 50 output limbs as columns —
 * single columns 24 + 2 (5 x + y) + limb for input[5 y + x], and 2314 + 2 (5 x + y) + limb for output[5 y + x] except lane (0, 0),
 * whose output limbs are columns 2428 and 2429 — and column 23 (the flag of the last round) as filter.
 * ------------------------------------------------------------------------------------------- */
#define GL_KECCAK_TABLE_COLUMNS 2430
GlError gl_keccak_table_trace(const uint64_t *d_inputs, uint64_t num_inputs, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                              void *ctx);
GlError gl_keccak_table_program(GlGatePrograms *out);

/* ---------------------------------------------------------------------------------------------
 * The memory table: the reference's MemoryStark (evm/src/memory/: memory_stark.rs, columns.rs), the table whose height follows
 * the length of the execution — 26 columns, one row per memory operation, dummy read or padding row — with its trace built in
 * HBM from the UNSORTED operation list and its constraints emitted natively, so that gl_stark_prove / gl_stark_tables_prove
 * prove it without the trace ever visiting the host.
 * gl_memory_table_trace = generate_trace (memory_stark.rs:122-236), bit for bit. d_ops: [num_ops][14] words of 64 bits in device
 * memory, one record per operation, exactly MemoryOp::into_row()[0..14]: FILTER, TIMESTAMP, IS_READ, ADDR_CONTEXT, ADDR_SEGMENT,
 * ADDR_VIRTUAL, then the eight 32-bit limbs of the value, least significant first. Any order; the order of the list breaks the
 * ties of equal (context, segment, virtual address, timestamp), as the reference's stable sorts do. LIMITS, checked on the
 * device: FILTER and IS_READ are 0 or 1, every other word is below 2^32, 2 <= num_ops <= 2^30.
 * d_trace receives [26][pitch trace_stride] value columns with n = 2^degree_bits rows, the layout gl_stark_prove takes. CONTRACT:
 * the rows are the reference's, quirks included — fill_gaps takes max_rc = next_power_of_two(num_ops) - 1 before any dummy is
 * added, never looks at context or segment gaps, and pushes dummy reads of value 0 and filter 0 at virt + k (max_rc + 1) with
 * timestamp 0 where the virtual address jumps and at timestamp + k max_rc where only the timestamp does; pad_memory_ops repeats
 * the LAST ELEMENT OF THE VECTOR after fill_gaps (the last dummy pushed, else the largest operation) as a read with filter 0, so
 * the padding rows can lie in the middle of the trace; then the first-change flags and RANGE_CHECK, COUNTER = 0 .. n, and
 * RANGE_CHECK_PERMUTED / COUNTER_PERMUTED as permuted_cols gives them. Every word of the 26 columns is written on every row
 * (columns 17 .. 21, between VIRTUAL_FIRST_CHANGE and RANGE_CHECK, as zeros; the last row's three flags and RANGE_CHECK are
 * zero) and is canonical: the buffer need not be zeroed; the words between n and trace_stride are left untouched.
 * The number of rows depends on the data: rows = num_ops + dummies, returned in *h_rows. With n = next_power_of_two(rows) the
 * trace is the reference's; a larger degree_bits is allowed and gives more padding rows under the same max_rc. d_trace == NULL
 * asks for the count alone (trace_stride is not read; degree_bits still sizes the scratch). PROTOCOL: the sort, the gaps, their
 * prefix sums and every data refusal are decided on ctx->stream first; the host then reads rows and a status word — the call's
 * ONE host wait —; the rows, the flags and the lookup columns are enqueued behind it and the call returns without waiting for
 * them. Nothing is allocated: d_scratch is gl_memory_table_scratch_bytes(num_ops, degree_bits) bytes, 16-byte aligned (it
 * includes what permuted_cols needs, about 8.7 max(n, num_ops) words) and holds nothing between calls; 0 is returned for
 * arguments out of range.
 * Refused with GL_E_INVALID and a message that names the reason, the trace untouched — for the data: rows > n (*h_rows still
 * says what is needed); a word outside the limits above (*h_rows is 0); a context or segment gap whose range check would be >= n
 * (the reference asserts there; not checked on a count-only call) — and before anything is launched: degree_bits outside 1 ..= 23
 * (what gl_stark_create takes for constraints of degree 3), num_ops out of range, trace_stride < n, a NULL pointer other than
 * d_trace, d_scratch not 16-byte aligned, d_ops, d_trace and d_scratch overlapping one another.
 * gl_memory_table_program = eval_packed_generic (memory_stark.rs:242-319) as ONE STARK program in the encoding of
 * GlStarkDesc.h_instrs, 23 constraints of degree 3 in the reference's order: the filter is boolean; a dummy row is a read; the
 * four flags are boolean; the six transition constraints "no change before the flagged column"; the range check's transition
 * constraint; the eight value constraints (plain constraints: they also bind the last row to row 0); eval_lookups of
 * (RANGE_CHECK_PERMUTED, COUNTER_PERMUTED). Device-free; the result is laid out and released as gl_keccak_table_program's. The
 * table has no public inputs; its permutation pairs are (RANGE_CHECK 22, RANGE_CHECK_PERMUTED 24) and (COUNTER 23,
 * COUNTER_PERMUTED 25); its cross-table lookup (memory_stark.rs:29-39) has the 13 columns IS_READ 2, ADDR_CONTEXT 3,
 * ADDR_SEGMENT 4, ADDR_VIRTUAL 5, the value limbs 6 .. 13, TIMESTAMP 1 and FILTER 0 as filter.
 * ------------------------------------------------------------------------------------------- */
#define GL_MEMORY_TABLE_COLUMNS 26
#define GL_MEMORY_TABLE_OP_WORDS 14
uint64_t gl_memory_table_scratch_bytes(uint64_t num_ops, uint32_t degree_bits);
GlError gl_memory_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                              void *d_scratch, uint64_t *h_rows, void *ctx);
GlError gl_memory_table_program(GlGatePrograms *out);
/* Measurement hook: gl_memory_table_trace with an event between its stages. h_ms[5] receives the milliseconds of the sort, the
 * gaps (dummy counts, their prefix sums, the decision), the rows, the flags and the lookup columns; the host's wait for the count
 * lies between the second and the third and belongs to none. d_trace is required. Creates and destroys its events and waits for
 * ctx->stream before it returns: not for use next to a proof in flight on the same context. */
GlError gl_debug_memory_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                       void *d_scratch, float *h_ms, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * The logic table: the reference's LogicStark (evm/src/logic.rs), the looked table of ctl_logic — what the CPU table's AND / OR /
 * XOR and the Keccak sponge's byte XORs look into — 523 columns, one row per operation on two 256-bit words — with its trace
 * built in HBM from a compact operation list and its constraints emitted natively, so that gl_stark_prove /
 * gl_stark_tables_prove prove it without the trace ever visiting the host.
 * gl_logic_table_trace = generate_trace_rows (logic.rs:157-176). d_ops: [num_ops][17] words of 64 bits in device memory, one
 * record per operation: word 0 the operator, given as the index of its flag column (0 = AND, 1 = OR, 2 = XOR); words 1 .. 8 the
 * eight 32-bit limbs of input0, least significant first; words 9 .. 16 the eight 32-bit limbs of input1. The result is not part
 * of the record: the device computes it. LIMITS, checked on the device: the operator is 0, 1 or 2, every limb is below 2^32.
 * d_trace receives [523][pitch trace_stride] value columns with n = 2^degree_bits rows, the layout gl_stark_prove takes. Columns
 * (logic.rs:28-52): IS_AND 0, IS_OR 1, IS_XOR 2, the bits of INPUT0 3 .. 258, least significant first, the bits of INPUT1
 * 259 .. 514, the eight 32-bit limbs of RESULT 515 .. 522. CONTRACT: row k < num_ops is Operation::into_row of record k (the
 * list order is the row order); rows num_ops .. n are all zero. With degree_bits = log2(next_power_of_two(max(num_ops, 1))),
 * at least 1, the trace is the reference's; a larger degree_bits is allowed and plays generate_trace_rows' min_rows. Every word
 * of the 523 columns is written on every row and is canonical — a flag, a bit or a 32-bit limb —: the buffer need not be
 * zeroed; the words between n and trace_stride are left untouched. num_ops == 0 is allowed (d_ops may then be NULL) and gives
 * an all-padding trace. PROTOCOL: a validation kernel runs first on ctx->stream; the host then reads one status word from
 * d_scratch — the call's ONE host wait —; the rows are enqueued behind it and the call returns without waiting for them. With
 * num_ops == 0 nothing is validated and the call does not wait. Nothing is allocated: d_scratch is
 * GL_LOGIC_TABLE_SCRATCH_BYTES bytes in device memory, 16-byte aligned, and holds nothing between calls.
 * Refused with GL_E_INVALID and a message, the trace untouched — for the data: an operator word that is not 0, 1 or 2, a limb
 * of 2^32 or more (the message names the lowest record index at fault and which of the two it was; the operator where that
 * record has both) — and before anything is launched: degree_bits outside 1 ..= 23 (what gl_stark_create takes for constraints
 * of degree 3), num_ops > n, trace_stride < n, a NULL pointer (other than d_ops with num_ops == 0), d_scratch not 16-byte
 * aligned, d_ops, d_trace and d_scratch overlapping one another.
 * gl_logic_table_program = eval_packed_generic (logic.rs:182-231) as ONE STARK program in the encoding of GlStarkDesc.h_instrs,
 * 520 constraints of degree 3 in the reference's order (the order decides the powers of alpha and so the proof's bytes): the 256
 * bit checks bit (bit - 1) of INPUT0, the 256 of INPUT1, then per result limb i = 0 .. 7
 * RESULT[i] - (sum_coeff (x + y) + and_coeff x_land_y) with sum_coeff = IS_OR + IS_XOR, and_coeff = IS_AND - IS_OR - 2 IS_XOR,
 * x and y the limb's 32 bits of the two inputs recomposed and x_land_y the weighted sum of their 32 products. The
 * recompositions and the weighted sum go through ACC in blocks of 16 weights that keep its overflow contract; the program stays
 * within 64 registers and 4 accumulators. Device-free; the result is laid out and released as gl_keccak_table_program's. The
 * table has no public inputs and no permutation pairs; its cross-table lookup (logic.rs:54-68) has 27 columns — the three flags
 * as single columns, eight combinations sum_j 2^j column(3 + 32 i + j) over j < 32 for INPUT0, eight such over
 * column(259 + 32 i + j) for INPUT1, the eight RESULT columns 515 .. 522 — and the combination IS_AND + IS_OR + IS_XOR as filter.
 * ------------------------------------------------------------------------------------------- */
#define GL_LOGIC_TABLE_COLUMNS 523
#define GL_LOGIC_TABLE_OP_WORDS 17
#define GL_LOGIC_TABLE_SCRATCH_BYTES 16
GlError gl_logic_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                             void *d_scratch, void *ctx);
GlError gl_logic_table_program(GlGatePrograms *out);
/* Measurement hook: the rows of gl_logic_table_trace alone, without the validation and its wait, at a chosen store width —
 * rows_per_thread 1: one row per thread, 8 bytes per lane and column store; 2: two adjacent rows per thread, 16 bytes per lane,
 * which needs d_trace 16-byte aligned and an even trace_stride. The records must be within the limits above: an operator
 * outside them gives a row without flag and result, a limb is cut to 32 bits. Same argument refusals as gl_logic_table_trace. */
GlError gl_debug_logic_table_fill(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                  uint32_t rows_per_thread, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * The Keccak sponge table: the reference's KeccakSpongeStark (evm/src/keccak_sponge/), the table that ties the three above
 * together — the only looker of ctl_keccak, five of the lookers of ctl_logic, 136 of the lookers of ctl_memory and the looked
 * table of ctl_keccak_sponge — 414 columns, len / 136 + 1 rows per hashed byte string. A list of byte strings goes in once; the
 * sponge's trace and the records the other three trace calls take come out in HBM.
 * gl_keccak_sponge_table_trace = generate_trace_rows (keccak_sponge_stark.rs:190-347), bit for bit. d_ops: [num_ops][5] words
 * of 64 bits in device memory, one record per KeccakSpongeOp: context, segment, virt (the base address), timestamp, len.
 * d_bytes: the inputs concatenated in list order, one uint8_t each, no alignment promised; may be NULL when every len is 0.
 * d_ops may be NULL when num_ops == 0, which gives an all-padding trace. LIMITS, checked on the device: every record word is
 * below 2^32, virt + len <= 2^32, the sum of all len is below 2^32; num_ops <= 2^30.
 * d_trace receives [414][pitch trace_stride] value columns with n = 2^degree_bits rows, the layout gl_stark_prove takes. Columns
 * (columns.rs:15-60): is_full_input_block 0, is_final_block 1, context 2, segment 3, virt 4, timestamp 5, len 6,
 * already_absorbed_bytes 7, is_final_input_len 8 .. 143, original_rate_u32s 144 .. 177, original_capacity_u32s 178 .. 193,
 * block_bytes 194 .. 329, xored_rate_u32s 330 .. 363, updated_state_u32s 364 .. 413. ROWS: operation k takes len_k / 136 + 1
 * consecutive rows, in list order: its full-block rows, then the final row, padded by pad10*1 (0x01 behind the input, 0x80 in
 * byte 135; a remainder of 135 bytes puts 0x81 in one byte). State limb 2 j / 2 j + 1 is the low / high half of Keccak lane j
 * (keccak_util.rs:6-18). The rows behind the operations are all zero. Every word of the 414 columns is written on every row and
 * is canonical: the buffer need not be zeroed; the words between n and trace_stride are left untouched.
 * ROW COUNT: rows = sum_k (len_k / 136 + 1) depends on the data and is returned in *h_rows; d_trace == NULL asks for the count
 * alone (trace_stride and d_bytes are not read; degree_bits still sizes the scratch). The reference sizes its trace as
 * next_power_of_two(max(num_ops, min_rows)) and silently drops whatever does not fit (.take(num_rows)), which cuts an operation in
 * the middle; this call REFUSES rows > n and names the count needed. CONTRACT: with n >= rows the trace is the reference's for
 * that n (for a min_rows with next_power_of_two(max(num_ops, min_rows)) == n).
 * PROTOCOL, as gl_memory_table_trace's: validation, the per-operation row and byte counts and their exclusive prefix sums run on
 * ctx->stream; the host then reads the row count and the status words — the call's ONE host wait —; the fill is enqueued
 * behind it and the call returns without waiting for it. With num_ops == 0 nothing is counted and the call does not wait. The
 * fill is two kernels: one lane per operation walks the operation's blocks (absorb, Keccak-f, next block; the only serial part)
 * and writes the 100 state columns; one lane per row writes the other 314. Nothing is allocated: d_scratch is
 * gl_keccak_sponge_table_scratch_bytes(num_ops, degree_bits) bytes in device memory, 16-byte aligned (32 + 8 (n + 2 num_ops)
 * bytes and a little), and holds nothing between calls; 0 is returned for arguments out of range.
 * Refused with GL_E_INVALID and a message that names the reason, the trace untouched — for the data: a record outside the
 * limits (the message names the LOWEST record at fault and its fault; *h_rows is 0); rows > n (*h_rows says what is needed);
 * d_bytes NULL although a len is not 0; d_trace overlapping the bytes the operations name — and before anything is launched:
 * degree_bits outside 1 ..= 23 (what gl_stark_create takes for constraints of degree 3), num_ops > 2^30, trace_stride < n, a NULL
 * pointer other than d_trace, d_bytes and (with num_ops == 0) d_ops, d_scratch not 16-byte aligned, d_ops, d_trace and d_scratch
 * overlapping one another. Keeping d_bytes apart from d_scratch is the caller's: its extent is known on the device alone.
 * gl_keccak_sponge_table_ops reads rows 0 .. rows of a finished trace (rows as *h_rows gave it) and writes what
 * keccak_sponge_log (witness/util.rs:196-250) pushes for the other tables; any output may be NULL:
 *   d_keccak_inputs [rows][25]: the state behind the XOR — lane j is limbs 2 j, 2 j + 1 of xored_rate_u32s ++
 *     original_capacity_u32s —, what push_keccak_bytes receives: the input of gl_keccak_table_trace;
 *   d_logic_ops [5 rows][17]: record 5 r + i is XOR (2), limbs 8 i .. of original_rate_u32s, the little-endian u32s of
 *     block_bytes[32 i ..], both zero-padded to eight limbs (record 4 carries two): xor_into_sponge's order, the input of
 *     gl_logic_table_trace;
 *   d_memory_ops [sum of len][14]: one read per input byte (padding bytes get none), by operation, then by address: FILTER 1,
 *     TIMESTAMP = timestamp, IS_READ 1, context, segment, virt + offset, the byte, seven zeros: the input of
 *     gl_memory_table_trace. A row's first record stands at the exclusive prefix sum of the rows' byte counts (136 for a full
 *     row, len - already_absorbed_bytes for a final one), computed on the device.
 * Runs on ctx->stream, waits for nothing, allocates nothing; d_scratch is gl_keccak_sponge_table_scratch_bytes(k, degree_bits)
 * bytes for any k (the trace call's scratch serves). Refused before anything is launched: NULL d_trace or d_scratch, degree_bits,
 * rows > n, trace_stride < n, alignment, an output overlapping the trace, the scratch or (the two of known size) each other.
 * gl_keccak_sponge_table_program: the table's constraints as ONE STARK program in the encoding of GlStarkDesc.h_instrs. The
 * reference's eval_packed_generic for this table is a list of TODOs (keccak_sponge_stark.rs:363-377); gl_stark_create refuses a
 * program without an EMIT, so the program is THAT LIST WRITTEN OUT — the reference's to-do list, NOT a soundness claim (nothing
 * here ties xored_rate_u32s to the block, for example: that is the logic lookup's job). 435 constraints of degree <= 3, in this
 * order, with F = is_full_input_block, L = is_final_block, d = is_final_input_len: F (F - 1), L (L - 1), F L; d[i] (d[i] - 1),
 * i < 136; sum_i d[i] - L; on the first row original_rate_u32s[j], original_capacity_u32s[j], already_absorbed_bytes (51); as
 * transitions L next.original_rate_u32s[j], L next.original_capacity_u32s[j], L next.already_absorbed_bytes (51); F (next.x - x)
 * for x = context, segment, virt, timestamp, len; F (next.original_rate_u32s[j] - updated_state_u32s[j]), j < 34, and
 * F (next.original_capacity_u32s[j] - updated_state_u32s[34 + j]), j < 16; F (next.already_absorbed_bytes -
 * already_absorbed_bytes - 136); (1 - F - L) (next.F + next.L); and plain again d[i] (len - already_absorbed_bytes - i), i < 136.
 * The TODO's "before_rate_bits, block_bits" name columns this layout does not have: nothing is emitted for them. Device-free;
 * the result is laid out and released as gl_keccak_table_program's. constraint_degree 3, no public inputs, no permutation pairs.
 * ------------------------------------------------------------------------------------------- */
#define GL_KECCAK_SPONGE_TABLE_COLUMNS 414
#define GL_KECCAK_SPONGE_TABLE_OP_WORDS 5
uint64_t gl_keccak_sponge_table_scratch_bytes(uint64_t num_ops, uint32_t degree_bits);
GlError gl_keccak_sponge_table_trace(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint32_t degree_bits, uint64_t *d_trace,
                                     uint64_t trace_stride, void *d_scratch, uint64_t *h_rows, void *ctx);
GlError gl_keccak_sponge_table_ops(const uint64_t *d_trace, uint64_t trace_stride, uint32_t degree_bits, uint64_t rows, uint64_t *d_keccak_inputs,
                                   uint64_t *d_logic_ops, uint64_t *d_memory_ops, void *d_scratch, void *ctx);
GlError gl_keccak_sponge_table_program(GlGatePrograms *out);
/* Measurement hook: gl_keccak_sponge_table_trace with an event between its stages. h_ms[4] receives the milliseconds of the
 * counting pass, the row-to-operation map, the chain kernel and the rows kernel; the host's wait for the count lies between the
 * first and the second and belongs to none. d_trace and num_ops >= 1 are required. Creates and destroys its events and waits for
 * ctx->stream before it returns: not for use next to a proof in flight on the same context. */
GlError gl_debug_keccak_sponge_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, const uint8_t *d_bytes, uint32_t degree_bits,
                                              uint64_t *d_trace, uint64_t trace_stride, void *d_scratch, float *h_ms, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * The arithmetic table: the reference's ArithmeticStark (evm/src/arithmetic/), 92 columns — the table of the EVM's 256-bit ADD, MUL,
 * SUB, LT, GT (one row each) and DIV, MOD, ADDMOD, SUBMOD, MULMOD (two rows each) — with its trace built in HBM from a compact
 * operation list and its constraints emitted natively, so that gl_stark_prove / gl_stark_tables_prove prove it without the trace
 * ever visiting the host. The reference's snapshot has the columns, ArithmeticStark::generate(lv, nv) for ONE operation's derived
 * cells and eval_packed_generic; it has no generate_trace, no range check and no cross-table lookup, the table is not in AllStark,
 * and generate panics on SHL and SHR. The TABLE is therefore defined here; the cells of an operation are bit for bit what
 * add / sub / mul / compare / modular::generate write.
 * d_ops: [num_ops][25] words of 64 bits in device memory, one record per operation: word 0 the operator, given as the index of its
 * flag column (ADD 0, MUL 1, SUB 2, DIV 3, MOD 4, ADDMOD 5, SUBMOD 6, MULMOD 7, LT 8, GT 9); words 1 .. 8, 9 .. 16 and 17 .. 24 the
 * eight 32-bit limbs of in0, in1 and in2, least significant first. ADD, MUL, SUB, LT, GT take (in0, in1) and in2 must be zero;
 * ADDMOD, SUBMOD, MULMOD take in2 as the modulus; MOD and DIV take in0 as numerator and in2 as denominator, and in1 must be zero.
 * The results are not part of the record: the device computes them. LIMITS, checked on the device: the operator is 0 .. 9 (SHL 10
 * and SHR 11 have flag columns that are always zero here), every limb is below 2^32, the must-be-zero input is zero;
 * num_ops <= 2^22.
 * d_trace receives [92][pitch trace_stride] value columns with n = 2^degree_bits rows, the layout gl_stark_prove takes. Columns
 * (columns.rs:25-117): the flags IS_ADD .. IS_SHR 0 .. 11, then five ranges of sixteen 16-bit limbs, least significant first:
 * GENERAL_INPUT_0 12 .. 27 (in0), GENERAL_INPUT_1 28 .. 43 (in1), GENERAL_INPUT_2 44 .. 59, GENERAL_INPUT_3 60 .. 75,
 * AUX_INPUT_0_LO 76 .. 91. ADD, SUB: the result in 44 .. 59. MUL: the result in 44 .. 59, mul.rs' aux carries in 60 .. 75. LT, GT:
 * the result in column 44 (45 .. 59 zero), the difference in 60 .. 75. Modular operations, first row: the modulus AS GIVEN in
 * 44 .. 59 (zero stays zero; the substitution by 1, or by 2^256 for DIV, is local to the witness, as in generate_modular_op), the
 * output (the remainder) in 60 .. 75, the low sixteen quotient limbs in 76 .. 91 — DIV's result; second row: all twelve flags
 * zero, MODULAR_QUO_INPUT_HI 12 .. 27 (the high sixteen quotient limbs), MODULAR_AUX_INPUT 28 .. 58 (31 values),
 * MODULAR_MOD_IS_ZERO 59, MODULAR_OUT_AUX_RED 60 .. 75, 76 .. 91 zero. Every shared cell of a one-row operation that the
 * reference does not write is zero. Signed values (the quotient limbs of a SUBMOD with in0 < in1, the aux values) are stored
 * canonically, p - |v|. A zero modulus or denominator gives the result 0.
 * ROWS: the operations stand in list order; operation k starts at the exclusive prefix sum of the row counts; the rows behind the
 * operations are all zero. Every flag constraint is filtered, so second rows and padding satisfy the program. rows = the sum of
 * the row counts depends on the data and is returned in *h_rows; d_trace == NULL asks for the count alone (trace_stride is not
 * read). rows > n is REFUSED and the message names the count needed; a modular operation whose second row is row n - 1 is allowed.
 * Every word of the 92 columns is written on all n rows and is canonical: the buffer need not be zeroed; the words between n and
 * trace_stride are left untouched. num_ops == 0 is allowed (d_ops may then be NULL) and gives an all-padding trace.
 * PROTOCOL, as gl_keccak_sponge_table_trace's: validation, the per-operation row counts and their exclusive prefix sums run on
 * ctx->stream; the host then reads the row count and the status words — the call's ONE host wait —; the fill is enqueued behind
 * it and the call returns without waiting for it. With num_ops == 0 nothing is counted and the call does not wait. The fill is
 * one lane per operation (a 512-by-256-bit division with fixed trip counts for the modular operators; nothing goes to scratch
 * memory) and one lane per zero row. Nothing is allocated: d_scratch is gl_arithmetic_table_scratch_bytes(num_ops, degree_bits)
 * bytes in device memory, 16-byte aligned (32 + 8 num_ops bytes and a little), and holds nothing between calls; 0 is returned for
 * arguments out of range.
 * Refused with GL_E_INVALID and a message that names the reason, the trace untouched — for the data: a record outside the limits
 * (the message names the LOWEST record at fault and its fault — the operator, else a limb, else the must-be-zero input —;
 * *h_rows is 0); rows > n (*h_rows says what is needed) — and before anything is launched: a NULL pointer other than d_trace and
 * (with num_ops == 0) d_ops, num_ops > 2^22, degree_bits outside 1 ..= 22 (what gl_stark_create takes for constraints of degree
 * 5), d_scratch not 16-byte aligned, trace_stride < n, d_ops, d_trace and d_scratch overlapping one another.
 * gl_arithmetic_table_program = arithmetic_stark.rs:72-87 as ONE STARK program in the encoding of GlStarkDesc.h_instrs, 246
 * constraints in the reference's order (the order decides the powers of alpha and so the proof's bytes): add 16, sub 16, mul 16,
 * compare 35 (the bit check, then 17 for LT and 17 for GT), modular 163 — constraint_last_row of the five modular flags' sum, the
 * two mod_is_zero checks, 16 + 1 of the less-than that shows the output reduced, the 15 high coefficients of quot * modulus, and
 * 4 x 32 coefficients of c + q m + (x - 2^16) s against the inputs of ADDMOD, SUBMOD, MULMOD and MOD / DIV —; everything in
 * modular behind the last-row check is a transition constraint. Product coefficients are formed on demand from LOAD_WIRE /
 * LOAD_NEXT; 2^16 and 2^-16 are immediates; the program stays within 64 registers and uses no accumulator. Device-free; the
 * result is laid out and released as gl_keccak_table_program's. No public inputs, no permutation pairs.
 * CONSTRAINT DEGREE: the reference's constraint_degree() says 3, but modular.rs:350 adds mod_is_zero * lv[IS_DIV] to limb 0 of
 * the output and the less-than then yields filter * t * (2^16 - t) with that quadratic t: sixteen constraints of degree 5
 * wherever the IS_DIV column and column 59 are not zero polynomials. A proof at declared degree 3 of such a trace is refused by
 * the verifier at zeta (tests/test_arithmetic_table_ref.py). Declare constraint_degree 5 (quotient_degree_factor 4, rate_bits >=
 * 2) for any trace that may hold a DIV row; 3 is sound only for a trace without one.
 * CROSS-TABLE LOOKUPS: the reference has none for this table. The result sits in a different range per operator family, so three
 * looked entries are offered, each over an operation's first row, values as eight 32-bit limbs lo + 2^16 hi of adjacent 16-bit
 * columns: "binary" — the flags 0, 1, 2, 8, 9, in0, in1, columns 44 .. 59, filter the sum of those flags; "modular" — the flags
 * 4, 5, 6, 7, in0, in1, in2, columns 60 .. 75, filter their sum; "div" — in0, in2, columns 76 .. 91, filter IS_DIV.
 * ------------------------------------------------------------------------------------------- */
#define GL_ARITHMETIC_TABLE_COLUMNS 92
#define GL_ARITHMETIC_TABLE_OP_WORDS 25
uint64_t gl_arithmetic_table_scratch_bytes(uint64_t num_ops, uint32_t degree_bits);
GlError gl_arithmetic_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                  void *d_scratch, uint64_t *h_rows, void *ctx);
GlError gl_arithmetic_table_program(GlGatePrograms *out);
/* Measurement hook: gl_arithmetic_table_trace with an event between its stages. h_ms[2] receives the milliseconds of the counting
 * pass and of the fill; the host's wait for the count lies between them and belongs to neither. d_trace and num_ops >= 1 are
 * required. Creates and destroys its events and waits for ctx->stream before it returns: not for use next to a proof in flight on
 * the same context. */
GlError gl_debug_arithmetic_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                           uint64_t trace_stride, void *d_scratch, float *h_ms, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * The Poseidon table: the permutation unit of the reference's system_zero crate (system_zero/src/permutation_unit.rs,
 * system_zero/src/registers/permutation.rs with START_PERMUTATION = 0) as a table of its own — every cell a degree-3 constraint
 * system needs for one width-12 Poseidon permutation over Goldilocks lies in one row — built on the device from a record list.
 * gl_poseidon_table_trace = generate_permutation_unit (permutation_unit.rs:56-105) on every row.
 * d_ops: [num_ops][13] words of 64 bits in device memory, one record per row. Word 0 is the kind:
 *   0, START: words 1 .. 12 are the whole input state;
 *   k = 1 .. 8, ABSORB: the row continues the sponge of the row before it — its input is that row's OUTPUT with elements
 *   0 .. k - 1 overwritten by words 1 .. k (the overwrite mode of plonky2's hash_n_to_m_no_pad); words k + 1 .. 12 are ignored.
 * Element words are any u64 and are reduced mod p; a kind word is compared as it stands. LIMITS, checked on the device: a kind is
 * 0 .. 8, and record 0 is a START.
 * d_trace receives [249][pitch trace_stride] value columns with n = 2^degree_bits rows, the layout gl_stark_prove takes. Columns:
 * INPUT 0 .. 11, the state before round 0; first full rounds r = 0 .. 3: mid_sbox 12 + 24 r + i, after_mds 24 + 24 r + i;
 * partial rounds r = 0 .. 21: mid_sbox 108 + 2 r, after_sbox 109 + 2 r; second full rounds r = 0 .. 3: mid_sbox 152 + 24 r + i,
 * after_mds 164 + 24 r + i; OUTPUT 236 .. 247 is the second full rounds' last after_mds; IS_REAL 248. mid_sbox is the CUBE of
 * the state behind the constant layer, after_mds the state behind the MDS layer and BEFORE the next round's constants,
 * after_sbox element 0 to the seventh power. IS_REAL is not the reference's: its unit has no filter because nothing looks into
 * it yet; it is 1 on a row a record made and 0 on padding.
 * ROWS: the record order is the row order; the rows num_ops .. n - 1 are padding rows. A padding row is NOT a zero row — the
 * constraints hold on every row —: it is the permutation of the all-zero state with IS_REAL = 0, the row the reference's
 * generate_trace_rows writes everywhere. Every word of the 249 columns is written on all n rows and is canonical: the buffer need
 * not be zeroed; the words between n and trace_stride are left untouched. num_ops == 0 is allowed (d_ops may then be NULL).
 * PROTOCOL: the validation (one thread per record) runs on ctx->stream; the host reads its 16 bytes — the call's ONE host wait
 * —; behind it, where the list holds an ABSORB, a serial pass (one lane per record: the lane of a START that an ABSORB follows
 * walks its run and writes the INPUT words of the continuation rows; a run as long as the list runs on one lane), then the rows
 * (one lane per row, all thirty rounds in registers) are enqueued and the call returns without waiting for them. With
 * num_ops == 0 nothing is validated and the call does not wait. Nothing is allocated: d_scratch is
 * GL_POSEIDON_TABLE_SCRATCH_BYTES bytes in device memory, 16-byte aligned, and holds nothing between calls.
 * Refused with GL_E_INVALID and a message that names the reason, the trace untouched — for the data, with the LOWEST record at
 * fault named: a kind above 8; record 0 being an ABSORB ("continues a sponge that no record starts") — and before anything is
 * launched: a NULL pointer (d_ops only with num_ops > 0), degree_bits outside 1 ..= GL_POSEIDON_TABLE_MAX_DEGREE_BITS (what
 * gl_stark_create takes for constraints of degree 3), num_ops > n, trace_stride < n, d_scratch not 16-byte aligned, d_ops,
 * d_trace and d_scratch overlapping one another.
 * gl_poseidon_table_program = eval_permutation_unit (permutation_unit.rs:108-172) as ONE STARK program in the encoding of
 * GlStarkDesc.h_instrs, 236 constraints in the reference's order (the order decides the powers of alpha and so the proof's
 * bytes), then IS_REAL (IS_REAL - 1): 237. The constant layers are LOAD_IMM + ADD, the MDS layers ACC / ACCR (a row's weights
 * sum to 264); the program stays within 64 registers. Device-free; the result is laid out and released as
 * gl_keccak_table_program's. Declare constraint_degree 3, no public inputs, no permutation pairs.
 * CROSS-TABLE LOOKUPS: one looked entry, "permutation": the 12 INPUT and the 12 OUTPUT columns, filter IS_REAL.
 * ------------------------------------------------------------------------------------------- */
#define GL_POSEIDON_TABLE_COLUMNS 249
#define GL_POSEIDON_TABLE_OP_WORDS 13
#define GL_POSEIDON_TABLE_SCRATCH_BYTES 16
#define GL_POSEIDON_TABLE_MAX_DEGREE_BITS 23
GlError gl_poseidon_table_trace(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace, uint64_t trace_stride,
                                void *d_scratch, void *ctx);
GlError gl_poseidon_table_program(GlGatePrograms *out);
/* Measurement hook: gl_poseidon_table_trace with an event between its stages and a choice of the rows kernel's MDS layer — mds 0:
 * the product's, 1: on the matrix cores, 2: on the vector ALU; the three write the same trace. h_ms[3] receives the milliseconds
 * of the validation, of the serial pass (negative: it did not run, the list holds no ABSORB) and of the rows; the host's wait for
 * the status words lies behind the validation and belongs to no stage. num_ops >= 1 is required. Creates and destroys its events
 * and waits for ctx->stream before it returns: not for use next to a proof in flight on the same context. */
GlError gl_debug_poseidon_table_stage_ms(const uint64_t *d_ops, uint64_t num_ops, uint32_t degree_bits, uint64_t *d_trace,
                                         uint64_t trace_stride, void *d_scratch, uint32_t mds, float *h_ms, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * (A) the reference's extern "C" surface (cuda/src/lib.rs:58-145). Synchronous.
 * ------------------------------------------------------------------------------------------- */

/* lib.rs:59 — declared by the reference, its definition is commented out there
 * (cuda/plonky2_gpu.cu:59-67). Here: makes device 0 current and builds the twiddle tables. */
void init(void);

/* lib.rs:61-69 / plonky2_gpu.cu:70-86. In-place inverse NTT of poly_num polynomials of
 * values_num_per_poly = 2^log_len elements each, contiguous. root_table is accepted and ignored
 * (twiddles are internal); n_inv is a HOST pointer and is checked against 2^-log_len. */
GlError ifft(uint64_t *d_values_flatten, int poly_num, int values_num_per_poly, int log_len,
             const uint64_t *d_root_table, const uint64_t *n_inv, void *ctx);

/* lib.rs:100-114 / plonky2_gpu.cu:435-606. Region contract (element offsets from
 * d_ext_values_flatten, P = poly_num, S = salt_size, n_ext = values_num_per_poly << rate_bits):
 *   [pad .. pad + (P+S)*n_ext)          column-major bit-reversed LDE         (plonky2_gpu.cu:461)
 *   [pad + (P+S)*n_ext .. + 4*num_digests + 4*2^cap_height)  digests || cap   (plonky2_gpu.cu:552)
 *   [0 .. (P+S)*n_ext)                  leaf-major LDE, written last after ctx->stream2 has been
 *                                       synchronised (plonky2_gpu.cu:586-591)
 * with pad = pad_extvalues_len. d_values_flatten holds the coefficients [P][n] and may alias
 * d_ext_values_flatten (plonky2/src/fri/oracle.rs:409-422 passes the same pointer).
 * d_shift_powers / root tables are accepted and ignored; the coset shift is 7. */
GlError merkle_tree_from_coeffs(uint64_t *d_values_flatten, uint64_t *d_ext_values_flatten, int poly_num,
                                int values_num_per_poly, int log_len, const uint64_t *d_root_table,
                                const uint64_t *d_root_table2, const uint64_t *d_shift_powers, int rate_bits,
                                int salt_size, int cap_height, int pad_extvalues_len, void *ctx);

/* lib.rs:83-98. The reference's definition is `assert(0)` (plonky2_gpu.cu:228); here it is the
 * working composition ifft + merkle_tree_from_coeffs. */
GlError merkle_tree_from_values(uint64_t *d_values_flatten, uint64_t *d_ext_values_flatten, int poly_num,
                                int values_num_per_poly, int log_len, const uint64_t *d_root_table,
                                const uint64_t *d_root_table2, const uint64_t *d_shift_powers, const uint64_t *n_inv,
                                int rate_bits, int salt_size, int cap_height, int pad_extvalues_len, void *ctx);

/* lib.rs:71-81 / plonky2_gpu.cu:138-189: Merkle tree over an LDE already resident at
 * d_ext_values_flatten + pad (column-major, NATURAL order as in the reference, which bit-reverses
 * it first): bit-reverses each column in place, then hashes and reduces as above. */
GlError build_merkle_tree(uint64_t *d_ext_values_flatten, int poly_num, int values_num_per_poly, int log_len,
                          int rate_bits, int salt_size, int cap_height, int pad_extvalues_len, void *ctx);

/* lib.rs:117-143 / plonky2_gpu.cu:609-783: the quotient polynomials of the ONE circuit the reference kernel is
 * hard-wired to — plonky2-ed25519: 234 wires / 80 routed, 8 constants, 2 challenges, quotient degree factor 8 =
 * 2^rate_bits, 25 gates in 6 selector groups, 231 gate constraints (plonky2_gpu.cu:666-675,
 * plonky2_gpu_impl.cuh:597-685). Same contract as the reference:
 *   - d_ext_values_flatten (wires), zs_partial_products_commitment_leaves->ptr and
 *     constants_sigmas_commitment_leaves->ptr are DEVICE buffers of LEAF-MAJOR rows [n_ext][leaf_len] with leaf t
 *     holding the point bitrev(t) (leaf_len 234 + salt_size, 20, 88; n_ext = values_num_per_poly << rate_bits) —
 *     region A of merkle_tree_from_values/coeffs; the DataSlice lengths are checked as the reference asserts them;
 *   - k_is (>= 80), alphas, betas, gammas (2 each) are DEVICE slices;
 *   - d_outs [2][n_ext] is scratch, d_quotient_polys [2][n_ext] receives the COEFFICIENTS of the two quotient
 *     polynomials (values on the coset -> ifft -> x shift^-i, plonky2_gpu.cu:737-765); the call synchronises ctx->stream.
 * Not read: d_root_table2, d_shift_inv_powers, points, z_h_on_coset_evals, z_h_on_coset_inverses (may be NULL) —
 * the kernels derive these from the library's own tables. Other shapes return GL_E_INVALID: every other circuit goes
 * through gl_compute_quotient_polys, of which this is one instance with the gate programs compiled in
 * (csrc/ed25519_gate_program.inc). The first call on a device builds its kernels with hiprtc: about a minute
 * of compilation when nothing is cached (six units; 15 s on the 8-core build container when forked workers compile them side by
 * side), about 2 s when ROCm's own compilation cache (~/.cache/comgr, on by default) has seen the
 * sources, immediate from
 * $PLONKY2_HIP_KERNEL_CACHE or, when that is unset, from the directory kernel_cache/ next to this library, where the
 * build (__graft_entry__.build()) puts the precompiled code objects. gl_reference_quotient_prepare() does it ahead of
 * the first proof.
 * The reference also compiles in the hash of one proof's public inputs (plonky2_gpu.cu:686-689); the same value is
 * the default here; gl_reference_set_public_inputs_hash_ctx() sets the value for the calls of ONE context (two circuits in one
 * process, each proving on its own context, do not race), gl_reference_set_public_inputs_hash() the process-wide value that
 * contexts without their own use (NULL restores the default in both).
 * Device memory: the kernels read column-major data 2.5x faster than leaf-major rows (a 1872-byte stride between
 * the lanes of a wave), so the call first transposes the three inputs into a staging buffer of
 * gl_reference_quotient_staging_bytes(log_len) = (234 + 88 + 20) * n_ext * 8 bytes per device (5.7 GB at log_len 18; salt
 * columns add salt_size * n_ext * 8). Either the CALLER provides it — gl_reference_quotient_set_staging(d_ptr, bytes) on the
 * current device, the reference's contract of a callee that allocates nothing; a buffer too small for a call is not used —
 * or the library allocates it on first use, keeps it for the next proof and frees it in gl_reference_quotient_release().
 * Without a staging buffer (allocation failed, too small, or PLONKY2_HIP_REFERENCE_IN_PLACE=1 in the environment) the
 * rows are read in place (same result, slower). Calls of compute_quotient_polys on one device take turns. */
GlError gl_reference_quotient_prepare(void *ctx);
GlError gl_reference_quotient_release(void);
uint64_t gl_reference_quotient_staging_bytes(int log_len);
GlError gl_reference_quotient_set_staging(void *d_staging /* NULL: library-owned again */, uint64_t bytes);
GlError gl_reference_set_public_inputs_hash(const uint64_t *h_hash /* 4, host */);
GlError gl_reference_set_public_inputs_hash_ctx(const uint64_t *h_hash /* 4, host */, void *ctx);
GlError compute_quotient_polys(const uint64_t *d_ext_values_flatten, int poly_num, int values_num_per_poly,
                               int log_len, const uint64_t *d_root_table2, const uint64_t *d_shift_inv_powers,
                               int rate_bits, int salt_size, const GlDataSlice *zs_partial_products_commitment_leaves,
                               const GlDataSlice *constants_sigmas_commitment_leaves, void *d_outs,
                               void *d_quotient_polys, const GlDataSlice *points, const GlDataSlice *z_h_on_coset_evals,
                               const GlDataSlice *z_h_on_coset_inverses, const GlDataSlice *k_is,
                               const GlDataSlice *alphas, const GlDataSlice *betas, const GlDataSlice *gammas, void *ctx);

/* The Rust wrapper falls back to this symbol when an Error carries no message
 * (cuda/src/lib.rs:42-45). Forwards to hipGetErrorString. */
const char *cudaGetErrorString(int code);

/* Test hook: element-wise field op on device arrays (op: 0 add, 1 sub, 2 mul, 3 neg, 4 x^7,
 * 5 a + b*b, 6 a * 2^(b mod 192), 7 a + canon(b), 8-16 internal variants, 17 a + (b mod 2^63) * 2^32, 18-27 the grouped
 * forms with deferred corrections, 28-30 the canonical form of a, b, a ^ b as a group with the subtraction deferred: stored as the
 * group left it); output canonical. d_b may be NULL for unary ops. Ops 100-109: the register-level radix
 * routines of the NTT passes on vectors of sixteen elements (n = 16 x vectors; d_b unused), see csrc/probes.hip. */
GlError gl_debug_field_op(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, uint64_t n, void *ctx);
/* Measurement hook: a plain streaming copy kernel (16 B per lane, asynchronous on ctx->stream) — the bandwidth a
 * kernel can actually reach on this device, which bench.py reports next to the 8 TB/s specification. */
GlError gl_debug_copy(void *d_dst, const void *d_src, uint64_t bytes, void *ctx);

/* Library identification: "plonky2_hip <version> gfx950". */
const char *gl_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PLONKY2_HIP_H */
