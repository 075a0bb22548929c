// prove.hip — the provers' HOST logic in native code: gl_circuit_create / gl_prove here, and gl_stark_create / gl_stark_prove (starky's
// prove(), stark_prove.hip) over the same commitments, transcript and FRI half (prove_common.h).
//
// prove() (plonky2/src/plonk/prover.rs:40-233) from the full witness on, with PolynomialBatch::prove_openings
// (plonky2/src/fri/oracle.rs:1047-1112), fri_proof (plonky2/src/fri/prover.rs:24-260), the Challenger
// (plonky2/src/iop/challenger.rs) and the proof wire format (plonky2/src/util/serialization.rs:466-700).
// Everything data-parallel is a kernel behind the gl_* entry points of this library; what lives here is
// the serial glue a Rust host would otherwise write against those entry points — the transcript's
// buffers, challenge arithmetic on single field elements, buffer management, serialisation — so that a
// host in any language needs exactly two calls. No polynomial, LDE, tree or witness column is touched
// by the CPU; the transcript lives on the device (gl_challenger_step): its sponge state, input buffer and challenges.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "prove_common.h"

using namespace plonky2_hip;

namespace {

// ---- the circuit object ---------------------------------------------------------------------------
struct Circuit : ProverShape {
    uint32_t num_wires, num_routed, num_constants, num_challenges, qdf, num_gate_constraints;
    uint64_t digest[4];  // HashOut, or one Keccak digest slot
    DevBuf k_is, sigmas;
    Batch cs;  // constants_sigmas_commitment
    // gates
    DevBuf d_instrs, d_gates, d_imms;
    uint32_t num_gates = 0, num_selectors = 0;
    void *gate_kernel = nullptr;
    ~Circuit() {
        if (gate_kernel) gl_gate_kernel_destroy(gate_kernel);
    }
};

uint32_t num_partial_products(uint32_t routed, uint32_t qdf) { return (routed + qdf - 1) / qdf - 1; }

}  // namespace

extern "C" {

static GlError circuit_create(uint32_t hasher, const GlCircuitDesc *d, void **circuit, void *ctx) {
    if (!d || !circuit || !ctx || !d->h_k_is || !d->h_constants || !d->h_sigmas || (d->fri.num_reductions && !d->fri.reduction_arity_bits))
        return fail(GL_E_INVALID, "null pointer");
    if (d->struct_size != sizeof(GlCircuitDesc)) return struct_size_error("GlCircuitDesc");
    if (d->degree_bits > 24 || d->num_challenges == 0 || d->num_challenges > 4 || d->num_routed_wires > d->num_wires ||
        d->quotient_degree_factor < 2 || d->quotient_degree_factor >= d->num_routed_wires)
        return fail(GL_E_INVALID, "bad circuit shape (the prover needs quotient_degree_factor < num_routed_wires, prover.rs:99-102)");
    // a Keccak circuit with a leaf of exactly four elements is refused here, before anything is allocated, not in the middle of a proof
    const uint32_t salt = d->fri.hiding ? SALT_SIZE : 0, nch = d->num_challenges, qdf = d->quotient_degree_factor;
    TRY(keccak_leaf_error(hasher, {{"constants / sigmas", d->num_constants + d->num_routed_wires}, {"wires", d->num_wires + salt},
                                   {"Zs / partial products", nch * (1 + num_partial_products(d->num_routed_wires, qdf)) + salt}, {"quotient", nch * qdf + salt}},
                          d->fri));
    std::unique_ptr<Circuit> c(new Circuit());  // deleted on every early return
    c->hasher = hasher;
    c->degree_bits = d->degree_bits, c->num_wires = d->num_wires, c->num_routed = d->num_routed_wires;
    c->num_constants = d->num_constants, c->num_challenges = d->num_challenges, c->qdf = d->quotient_degree_factor;
    c->num_gate_constraints = d->num_gate_constraints;
    c->set_fri(d->fri);
    const uint64_t n = 1ull << c->degree_bits;
    TRY(c->k_is.alloc(c->num_routed));
    TRY(gl_memcpy_h2d(c->k_is.p, d->h_k_is, 8ull * c->num_routed, ctx));
    TRY(c->sigmas.alloc((uint64_t)c->num_routed * n));
    TRY(gl_memcpy_h2d(c->sigmas.p, d->h_sigmas, 8ull * c->num_routed * n, ctx));
    // constants_sigmas_commitment (circuit_builder.rs:861-873): constants then sigmas, from values
    DevBuf csv;
    TRY(csv.alloc((uint64_t)(c->num_constants + c->num_routed) * n));
    TRY(gl_memcpy_h2d(csv.p, d->h_constants, 8ull * c->num_constants * n, ctx));
    TRY(gl_memcpy_h2d(csv.p + (uint64_t)c->num_constants * n, d->h_sigmas, 8ull * c->num_routed * n, ctx));
    TRY(commit(&c->cs, std::move(csv), true, c->num_constants + c->num_routed, *c, ctx));
    if (d->h_circuit_digest) {
        memcpy(c->digest, d->h_circuit_digest, 32);
    } else if (c->keccak()) {
        // the same with C::Hasher = KeccakHash<25>: cap.flatten() and the separator's hash enter as to_vec(), four elements per hash
        const std::vector<uint64_t> pad = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
        uint64_t dsd[4];
        TRY(keccak_hash_no_pad(pad, dsd, ctx));
        std::vector<uint64_t> parts(c->cs.cap.size() + 5);
        for (size_t h = 0; h < c->cs.cap.size() / 4; h++) keccak_to_vec(c->cs.cap.data() + 4 * h, parts.data() + 4 * h);
        keccak_to_vec(dsd, parts.data() + c->cs.cap.size());
        parts.back() = c->degree_bits;
        TRY(keccak_hash_no_pad(parts, c->digest, ctx));
    } else {
        // circuit_builder.rs:915-927: hash_no_pad(cap || hash_pad(domain separator = []) || degree_bits)
        uint64_t pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, dsd[4];
        TRY(hash_no_pad(pad, 12, dsd, ctx));
        std::vector<uint64_t> parts(c->cs.cap);
        parts.insert(parts.end(), dsd, dsd + 4);
        parts.push_back(c->degree_bits);
        TRY(hash_no_pad(parts.data(), parts.size(), c->digest, ctx));
    }
    if (d->num_gates) {
        if (!d->h_instrs || !d->h_gates) return fail(GL_E_INVALID, "null gate program");
        c->num_gates = d->num_gates, c->num_selectors = d->num_selectors;
        {
            std::string verr;
            uint32_t wires_needed = 0, constants_needed = 0;
            if (!plonky2_hip::gate_programs_validate(reinterpret_cast<const uint16_t *>(d->h_instrs), d->num_instrs, reinterpret_cast<const uint32_t *>(d->h_gates),
                                        d->num_gates, d->num_immediates, d->num_selectors, d->num_gate_constraints, &wires_needed,
                                        &constants_needed, &verr))
                return fail(GL_E_INVALID, "gate programs: " + verr);
            if (wires_needed > c->num_wires || constants_needed > c->num_constants)
                return fail(GL_E_INVALID, "gate programs load wire " + std::to_string(wires_needed ? wires_needed - 1 : 0) + " / constant column " +
                                 std::to_string(constants_needed ? constants_needed - 1 : 0) + " but the circuit has " + std::to_string(c->num_wires) +
                                 " wires and " + std::to_string(c->num_constants) + " constants");
        }
        if (d->compile_gates) {
            TRY(gl_gate_kernel_build(d->h_instrs, d->num_instrs, d->h_gates, d->num_gates, d->h_immediates, d->num_immediates,
                                      d->num_selectors, d->num_gate_constraints, d->num_challenges, &c->gate_kernel));
        } else {
            TRY(c->d_instrs.alloc(d->num_instrs ? d->num_instrs : 1));  // 8 bytes per GlGateInstr
            TRY(gl_memcpy_h2d(c->d_instrs.p, d->h_instrs, 8ull * d->num_instrs, ctx));
            TRY(c->d_gates.alloc(3ull * d->num_gates));  // 24 bytes per GlGateDesc
            TRY(gl_memcpy_h2d(c->d_gates.p, d->h_gates, 24ull * d->num_gates, ctx));
            if (d->num_immediates) {
                TRY(c->d_imms.alloc(d->num_immediates));
                TRY(gl_memcpy_h2d(c->d_imms.p, d->h_immediates, 8ull * d->num_immediates, ctx));
            }
        }
    }
    TRY(gl_ctx_synchronize(ctx));
    *circuit = c.release();
    return ok();
}

GlError gl_circuit_create(const GlCircuitDesc *d, void **circuit, void *ctx) { return circuit_create(GL_HASHER_POSEIDON, d, circuit, ctx); }

GlError gl_circuit_create_h(uint32_t hasher, const GlCircuitDesc *d, void **circuit, void *ctx) {
    if (hasher == GL_HASHER_POSEIDON) return gl_circuit_create(d, circuit, ctx);
    if (hasher != GL_HASHER_KECCAK25) return fail(GL_E_INVALID, "unknown hasher");
    return circuit_create(hasher, d, circuit, ctx);
}

void gl_circuit_destroy(void *circuit) { delete static_cast<Circuit *>(circuit); }

GlError gl_circuit_trim(void *circuit) {
    if (!circuit) return fail(GL_E_INVALID, "null pointer");
    return static_cast<Circuit *>(circuit)->trim();
}

GlError gl_circuit_info(const void *circuit, uint64_t h_digest[4], uint64_t *h_constants_sigmas_cap) {
    if (!circuit) return fail(GL_E_INVALID, "null pointer");
    const Circuit *c = static_cast<const Circuit *>(circuit);
    if (h_digest) memcpy(h_digest, c->digest, 32);
    if (h_constants_sigmas_cap) memcpy(h_constants_sigmas_cap, c->cs.cap.data(), c->cs.cap.size() * 8);
    return ok();
}

void gl_bytes_free(uint8_t *p) { free(p); }

// The transcript of a proof lives on the device (gl_challenger_step): every observation reads its source where the producing kernel
// left it (caps, openings, the final polynomial, the proof-of-work witness), the FRI betas, the query indices and the proof-of-work
// state are consumed there, and the host fetches exactly the challenges it computes with — betas / gammas (with the public-inputs
// hash), alphas, zeta, the FRI alpha — one small copy and one stream synchronisation each, then the proof-of-work witness, then
// everything that goes into the proof bytes in one go. Round 5 paid a host round trip per Challenger call (sixteen per proof, each
// an upload, a launch, a download and a synchronisation) and one per cap, opening batch and query batch.
static GlError prove_impl(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                          const uint64_t *d_salts, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx) {
    if (!circuit || !d_wires || !proof || !proof_len || !ctx || (num_public_inputs && !h_public_inputs)) return fail(GL_E_INVALID, "null pointer");
    const Circuit &c = *static_cast<const Circuit *>(circuit);
    if (c.hiding && !d_salts) return fail(GL_E_INVALID, "the circuit's FRI parameters are hiding (zero_knowledge): prove it with gl_prove_zk and salt columns");
    if (!c.hiding && d_salts) return fail(GL_E_INVALID, "gl_prove_zk on a circuit whose FRI parameters are not hiding");
    if (h_stage_ms) memset(h_stage_ms, 0, sizeof(double) * GL_PROVE_STAGES);
    ProofSession s(c, h_stage_ms, ctx);  // the context's device is current; every DevBuf below comes from / returns to the circuit's pool of this context
    const uint32_t db = c.degree_bits, nch = c.num_challenges, qdf = c.qdf, npi = num_public_inputs;
    const uint64_t n = 1ull << db, n_ext = n << c.rate_bits, cap_words = 4ull << c.cap_height;
    const uint32_t npp = num_partial_products(c.num_routed, qdf);

    // ---- the small-data side of the proof: one device buffer, one page-locked mirror -------------------------------------------
    const uint32_t n_polys[4] = {c.num_constants + c.num_routed, c.num_wires, nch * (1 + npp), nch * qdf};
    const uint32_t salt = d_salts ? SALT_SIZE : 0;
    const std::vector<uint32_t> leaf_len = {n_polys[0], n_polys[1] + salt, n_polys[2] + salt, n_polys[3] + salt};
    FriLayout L;
    TRY(fri_shapes(c, &L));
    const Span T = s.take(32), HP = s.take(32), hostin = s.take(4 + (uint64_t)npi);
    const Span fetch0 = s.take(0);  // from here on: what the host fetches
    const Span pih_s = s.take(4), bg = s.take(2ull * nch), alphas_s = s.take(nch), zeta_s = s.take(2);
    Span opens[4], caps[3];
    for (int o = 0; o < 4; o++) opens[o] = s.take(2ull * (o == 2 ? 2 : 1) * n_polys[o]);
    for (int o = 0; o < 3; o++) caps[o] = s.take(cap_words);
    fri_layout(c, leaf_len, &s.sd, &L);
    TRY(s.begin());
    uint64_t *const D = s.D, *const H = s.H;

    // circuit digest and public inputs go up once; hash_no_pad(public inputs) (prover.rs:52) on a scratch challenger
    memcpy(H + hostin.off, c.digest, 32);
    for (uint32_t i = 0; i < npi; i++) H[hostin.off + 4 + i] = h_public_inputs[i];
    TRY(s.upload(hostin));
    TRY(s.step(HP, {GlObserveSrc{D + hostin.off + 4, npi, 0}}, 0, pih_s, GL_CHALLENGER_RESET | GL_CHALLENGER_HASH));
    // wires commitment (prover.rs:66-90); the caller's witness stays intact for the partial products
    Batch wires;
    TRY(commit_copy(&wires, d_wires, c.num_wires, c, ctx, d_salts));
    TRY(s.st.mark(0));
    // challenger.observe_hash(circuit digest), observe_hash(public inputs hash), observe_cap(wires cap); betas, gammas (prover.rs:92-97)
    TRY(s.step(T, {c.hashes(D + hostin.off, 4), GlObserveSrc{D + pih_s.off, 4, 0}, c.hashes(wires.cap_d.p, cap_words)}, 2 * nch, bg, GL_CHALLENGER_RESET));
    TRY(s.fetch(Span{pih_s.off, bg.off + bg.words - pih_s.off}));
    TRY(s.sync());
    uint64_t pih[4];
    memcpy(pih, H + pih_s.off, 32);
    const std::vector<uint64_t> betas(H + bg.off, H + bg.off + nch), gammas(H + bg.off + nch, H + bg.off + 2 * nch);
    std::vector<uint64_t> alphas;
    // partial products and Z (prover.rs:99-117), committed in place
    Batch zs;
    {
        DevBuf z;
        TRY(z.alloc((uint64_t)nch * (1 + npp) * n));
        TRY(gl_permutation_partial_products(d_wires, n, c.sigmas.p, n, c.k_is.p, betas.data(), gammas.data(), nch, c.num_routed, qdf, db, z.p,
                                            ctx));
        TRY(s.st.mark(1));
        TRY(commit(&zs, std::move(z), true, nch * (1 + npp), c, ctx, d_salts ? d_salts + (uint64_t)SALT_SIZE * n_ext : nullptr, false));
    }
    TRY(s.st.mark(2));
    TRY(s.step(T, {c.hashes(zs.cap_d.p, cap_words)}, nch, alphas_s));
    TRY(s.fetch(alphas_s));
    TRY(s.sync());
    alphas.assign(H + alphas_s.off, H + alphas_s.off + nch);
    // quotient polynomials (prover.rs:137-151)
    const uint32_t qdb = glh::log2_ceil(qdf);
    DevBuf quotient, work;
    TRY(quotient.alloc((uint64_t)nch << (db + qdb)));
    {
        GlQuotientArgs a;
        memset(&a, 0, sizeof a);
        a.d_wires_leaves = wires.lde.p, a.d_constants_sigmas_leaves = c.cs.lde.p, a.d_zs_partial_products_leaves = zs.lde.p;
        a.wires_leaf_len = c.num_wires, a.constants_sigmas_leaf_len = c.num_constants + c.num_routed;
        a.zs_partial_products_leaf_len = nch * (1 + npp);
        a.d_k_is = c.k_is.p;
        a.h_betas = betas.data(), a.h_gammas = gammas.data(), a.h_alphas = alphas.data();
        a.num_constants = c.num_constants, a.num_routed_wires = c.num_routed, a.num_challenges = nch;
        a.num_gate_constraints = c.num_gates ? c.num_gate_constraints : 0;
        a.degree_bits = db, a.rate_bits = c.rate_bits, a.quotient_degree_factor = qdf, a.coset_shift = 7;
        a.column_stride = n_ext;
        GlGateProgram gp;
        memset(&gp, 0, sizeof gp);
        if (c.gate_kernel) {
            TRY(work.alloc((uint64_t)nch << (db + qdb)));
            a.gate_kernel = c.gate_kernel, a.h_public_inputs_hash = pih, a.d_gate_workspace = work.p;
        } else if (c.num_gates) {
            gp.d_instrs = reinterpret_cast<const GlGateInstr *>(c.d_instrs.p);
            gp.d_gates = reinterpret_cast<const GlGateDesc *>(c.d_gates.p);
            gp.d_immediates = c.d_imms.p;
            gp.num_gates = c.num_gates, gp.num_selectors = c.num_selectors;
            memcpy(gp.public_inputs_hash, pih, 32);
            a.gate_program = &gp;
        }
        TRY(gl_compute_quotient_polys(&a, quotient.p, ctx));
    }
    TRY(s.st.mark(3));
    // split into degree-n chunks (prover.rs:153-166) and commit from coefficients
    Batch quot;
    TRY(commit_quotient_chunks(&quot, std::move(quotient), nch, qdf, qdb, c, ctx, d_salts ? d_salts + 2ull * SALT_SIZE * n_ext : nullptr));
    TRY(s.st.mark(4));
    TRY(s.step(T, {c.hashes(quot.cap_d.p, cap_words)}, 2, zeta_s));
    TRY(s.fetch(zeta_s));
    TRY(s.sync());
    const E2 zeta{H[zeta_s.off], H[zeta_s.off + 1]};
    if (E2 zn = e2_pow(zeta, n); zn.a == 1 && zn.b == 0) return fail(GL_E_INVALID, "Opening point is in the subgroup.");
    const uint64_t g = glh::root_of_unity(db);
    const E2 g_zeta = e2_mul(E2{g, 0}, zeta);
    // OpeningSet::new (plonk/proof.rs:305-334): every oracle's polynomials at zeta, the Zs also at g * zeta, left in device memory
    const std::vector<const Batch *> oracles = {&c.cs, &wires, &zs, &quot};
    {
        const uint64_t pts[4] = {zeta.a, zeta.b, g_zeta.a, g_zeta.b};
        for (int o = 0; o < 4; o++)
            TRY(gl_eval_polys_ext2(oracles[o]->coeffs.p, oracles[o]->n_polys, db, n, pts, o == 2 ? 2 : 1, D + opens[o].off, ctx));
    }
    TRY(s.st.mark(5));
    // to_fri_openings (proof.rs:336-356): [constants, sigmas, wires, zs, partial products, quotient], then zs_next; then
    // PolynomialBatch::prove_openings: batch 0 is every polynomial of the four oracles at zeta, batch 1 the Zs at g*zeta
    // (circuit_data.rs:351-371)
    uint64_t pow_witness = 0;
    {
        std::vector<FriBatch> batches(2);
        batches[0].point = zeta, batches[1].point = g_zeta;
        for (int o = 0; o < 4; o++)
            for (uint32_t k = 0; k < oracles[o]->n_polys; k++) batches[0].polys.push_back(oracles[o]->coeffs.p + (uint64_t)k * n);
        for (uint32_t k = 0; k < nch; k++) batches[1].polys.push_back(zs.coeffs.p + (uint64_t)k * n);
        const std::vector<GlObserveSrc> opening_srcs = {
            GlObserveSrc{D + opens[0].off, 2ull * n_polys[0], 0}, GlObserveSrc{D + opens[1].off, 2ull * n_polys[1], 0},
            GlObserveSrc{D + opens[2].off, 2ull * n_polys[2], 0}, GlObserveSrc{D + opens[3].off, 2ull * n_polys[3], 0},
            GlObserveSrc{D + opens[2].off + 2ull * n_polys[2], 2ull * nch, 0}};
        TRY(fri_prove(c, L, s, T, oracles, opening_srcs, batches, &pow_witness));
    }
    // everything the proof consists of, in one go
    TRY(gl_memcpy_d2d(D + caps[0].off, wires.cap_d.p, cap_words * 8, ctx));
    TRY(gl_memcpy_d2d(D + caps[1].off, zs.cap_d.p, cap_words * 8, ctx));
    TRY(gl_memcpy_d2d(D + caps[2].off, quot.cap_d.p, cap_words * 8, ctx));
    TRY(s.fetch(Span{fetch0.off, s.sd.top - fetch0.off}));
    TRY(gl_ctx_synchronize(ctx));
    TRY(s.st.mark(9));
    TRY(fri_check_pow(c, L, H, pow_witness));
    // ---- write_proof_with_public_inputs (util/serialization.rs:641-689) ----
    Bytes out;
    out.keccak = c.keccak();
    for (int o = 0; o < 3; o++) out.hashes(H + caps[o].off, cap_words / 4);  // wires, zs / partial products, quotient
    // write_opening_set (:557-571): constants, sigmas, wires, zs, zs_next, partial products, quotient
    const uint64_t *ev[4] = {H + opens[0].off, H + opens[1].off, H + opens[2].off, H + opens[3].off};
    out.fields(ev[0], 2ull * n_polys[0]);                                   // constants then sigmas: contiguous
    out.fields(ev[1], 2ull * n_polys[1]);                                   // wires
    out.fields(ev[2], 2ull * nch);                                          // plonk_zs
    out.fields(ev[2] + 2ull * n_polys[2], 2ull * nch);                      // plonk_zs_next
    out.fields(ev[2] + 2ull * nch, 2ull * n_polys[2] - 2ull * nch);         // partial_products
    out.fields(ev[3], 2ull * n_polys[3]);                                   // quotient_polys
    fri_write(out, c, L, H, oracles, pow_witness);
    out.fields(h_public_inputs, num_public_inputs);
    TRY(bytes_out(out, proof, proof_len));
    return s.st.mark(10);
}

GlError gl_prove(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                 uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx) {
    return prove_impl(circuit, d_wires, h_public_inputs, num_public_inputs, nullptr, proof, proof_len, h_stage_ms, ctx);
}

// A batch of independent proofs of one circuit with several in flight (configs[4]'s unit of work per GPU): worker w — a host thread
// this call starts — proves witnesses w, w + in_flight, w + 2 in_flight, .. on ctxs[w]. The workers share the circuit handle (a buffer
// pool per context; the launches of its gate kernel take turns) and run at the same time: each fills the other's latency-bound phases.
GlError gl_prove_many(const void *circuit, const uint64_t *const *d_wires, const uint64_t *const *h_public_inputs, uint32_t num_public_inputs,
                      uint32_t count, uint8_t **proofs, uint64_t *proof_lens, void *const *ctxs, uint32_t in_flight) {
    if (!circuit || !proofs || !proof_lens || !ctxs || (count && (!d_wires || (num_public_inputs && !h_public_inputs)))) return fail(GL_E_INVALID, "null pointer");
    if (in_flight == 0 || in_flight > 16) return fail(GL_E_INVALID, "in_flight must be 1..16");
    for (uint32_t w = 0; w < in_flight; w++) {
        if (!ctxs[w]) return fail(GL_E_INVALID, "null context");
        for (uint32_t v = 0; v < w; v++)
            if (ctxs[v] == ctxs[w]) return fail(GL_E_INVALID, "every worker needs a context of its own");
    }
    for (uint32_t i = 0; i < count; i++) proofs[i] = nullptr, proof_lens[i] = 0;
    std::vector<GlError> errs(in_flight, GlError{0, nullptr});
    auto work = [&](uint32_t w) {
        for (uint32_t i = w; i < count; i += in_flight) {
            GlError e = prove_impl(circuit, d_wires[i], num_public_inputs ? h_public_inputs[i] : nullptr, num_public_inputs, nullptr, &proofs[i], &proof_lens[i],
                                   nullptr, ctxs[w]);
            if (e.code != 0) {
                errs[w] = e;
                return;
            }
        }
    };
    std::vector<std::thread> threads;
    for (uint32_t w = 1; w < in_flight && w < count; w++) threads.emplace_back(work, w);
    work(0);
    for (auto &t : threads) t.join();
    GlError first{0, nullptr};
    for (uint32_t w = 0; w < in_flight; w++)
        if (errs[w].code != 0) {
            if (first.code == 0) first = errs[w];
            else free(errs[w].message);
        }
    if (first.code != 0)
        for (uint32_t i = 0; i < count; i++) {  // all or nothing
            free(proofs[i]);
            proofs[i] = nullptr, proof_lens[i] = 0;
        }
    return first;
}

GlError gl_prove_zk(const void *circuit, const uint64_t *d_wires, const uint64_t *h_public_inputs, uint32_t num_public_inputs,
                    const uint64_t *d_salts, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms, void *ctx) {
    if (!d_salts) return fail(GL_E_INVALID, "gl_prove_zk: null salt columns");
    return prove_impl(circuit, d_wires, h_public_inputs, num_public_inputs, d_salts, proof, proof_len, h_stage_ms, ctx);
}

}  // extern "C"
