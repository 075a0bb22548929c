// ---- STARKs: gl_stark_create / gl_stark_prove = starky's prove() (starky/src/prover.rs:32-195); gl_stark_tables_create /
// gl_stark_tables_prove = prove_with_traces (evm/src/prover.rs:66-421) over the same per-table flow ------------------------------------
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "stark_prove.h"

using namespace plonky2_hip;

namespace plonky2_hip {

static GlError tables_of(void *ctx, const NttTables **tb) {
    if (hipError_t e = ctx_tables(ctx, tb); e != hipSuccess) return hip_fail(e, "context tables");
    return ok();
}

// the quotient values of one trace, then their coset_ifft (prover.rs:314-318); ctl / h_ctl_challenges: the table's CTL checks, or null
static GlError stark_quotient(const Stark &s, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde, uint64_t column_stride, const uint64_t *h_alphas,
                              const uint64_t *h_challenges, const uint64_t *d_public_inputs, uint64_t *d_out, void *ctx,
                              const plonky2_hip::StarkCtlDev *ctl = nullptr, const uint64_t *h_ctl_challenges = nullptr) {
    const plonky2_hip::NttTables *tb;
    TRY(tables_of(ctx, &tb));
    plonky2_hip::StarkQuotientArgs a = {};
    a.instrs = reinterpret_cast<const uint16_t *>(s.d_instrs.p), a.num_instrs = s.num_instrs, a.imms = s.d_imms.p, a.public_inputs = d_public_inputs;
    a.trace_lde = d_trace_lde, a.zs_lde = d_zs_lde, a.column_stride = column_stride, a.pairs = s.pairs();
    a.alphas = h_alphas, a.challenges = h_challenges;
    a.num_challenges = s.num_challenges, a.qdf = s.qdf, a.degree_bits = s.degree_bits, a.rate_bits = s.rate_bits;
    if (ctl) a.ctl = *ctl, a.ctl_challenges = h_ctl_challenges;
    const hipError_t e = s.jit ? plonky2_hip::stark_jit_launch(s.jit, *tb, a, d_out, ctx_stream(ctx))
                               : plonky2_hip::stark_quotient_values(*tb, a, d_out, ctx_stream(ctx));
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "inconsistent arguments of the STARK quotient (column_stride / challenges / sizes)");
    if (e != hipSuccess) return hip_fail(e, "stark_quotient_values");
    const uint32_t log_size = s.degree_bits + s.qdb;
    return gl_coset_ntt_batch(d_out, s.num_challenges, log_size, 1ull << log_size, 7, 1, ctx);
}

GlError stark_check(uint32_t hasher, const GlStarkDesc *d, uint32_t num_ctl_zs) {
    if (!d || !d->h_instrs || (d->num_immediates && !d->h_immediates) || (d->fri.num_reductions && !d->fri.reduction_arity_bits) ||
        (d->num_pairs && (!d->h_column_pairs || !d->h_pair_bounds)))
        return fail(GL_E_INVALID, "null pointer");
    if (d->struct_size != sizeof(GlStarkDesc)) return struct_size_error("GlStarkDesc");
    if (hasher != GL_HASHER_POSEIDON && hasher != GL_HASHER_KECCAK25) return fail(GL_E_INVALID, "unknown hasher");
    if (d->fri.hiding) return fail(GL_E_INVALID, "a STARK's FRI parameters are not hiding (starky: fri_params(degree_bits, false))");
    if (d->degree_bits == 0 || d->degree_bits + d->fri.rate_bits > 24 || d->num_columns == 0 || d->num_columns > 65535 || d->num_public_inputs > 65535 ||
        d->num_challenges == 0 || d->num_challenges > plonky2_hip::STARK_MAX_CHALLENGES || d->constraint_degree == 0)
        return fail(GL_E_INVALID, "bad STARK shape (1 <= degree_bits, degree_bits + rate_bits <= 24, 1 <= num_columns, 1 <= num_challenges <= 4, 1 <= constraint_degree)");
    const uint32_t qdf = d->constraint_degree > 2 ? d->constraint_degree - 1 : 1;  // stark.rs:79-81
    const uint32_t qdb = glh::log2_ceil(qdf);
    if (qdf > plonky2_hip::STARK_MAX_QDF) return fail(GL_E_INVALID, "quotient_degree_factor > 16");
    if (qdb > d->fri.rate_bits) return fail(GL_E_INVALID, "Having constraints of degree higher than the rate is not supported yet. (log2_ceil(quotient_degree_factor) > rate_bits, prover.rs:223-226)");
    uint32_t total_arity = 0;
    for (uint32_t li = 0; li < d->fri.num_reductions; li++) total_arity += d->fri.reduction_arity_bits[li];
    if (d->fri.cap_height > d->degree_bits + d->fri.rate_bits || total_arity > d->degree_bits + d->fri.rate_bits - d->fri.cap_height || total_arity > d->degree_bits)
        return fail(GL_E_INVALID, "FRI total reduction arity is too large.");
    if (d->num_pairs) {
        if (d->h_pair_bounds[0] != 0) return fail(GL_E_INVALID, "h_pair_bounds must start at 0");
        for (uint32_t p = 0; p < d->num_pairs; p++)
            if (d->h_pair_bounds[p + 1] < d->h_pair_bounds[p]) return fail(GL_E_INVALID, "h_pair_bounds must not decrease");
        for (uint32_t k = 0; k < 2 * d->h_pair_bounds[d->num_pairs]; k++)
            if (d->h_column_pairs[k] >= d->num_columns) return fail(GL_E_INVALID, "permutation pair: column out of range");
    }
    const uint32_t num_zs = d->num_pairs ? plonky2_hip::stark_num_zs(d->num_pairs, d->num_challenges, qdf) : 0;
    {
        std::string verr;
        if (!plonky2_hip::stark_program_validate(reinterpret_cast<const uint16_t *>(d->h_instrs), d->num_instrs, d->h_immediates, d->num_immediates,
                                                 d->num_columns, d->num_public_inputs, &verr))
            return fail(GL_E_INVALID, verr);
    }
    TRY(keccak_leaf_error(hasher, {{"trace", d->num_columns}, {num_ctl_zs ? "permutation / CTL Zs" : "permutation Zs", num_zs + num_ctl_zs}, {"quotient", d->num_challenges * qdf}},
                          d->fri));  // as gl_circuit_create_h
    return ok();
}

plonky2_hip::StarkJitDesc stark_host_desc(const GlStarkDesc *d) {
    plonky2_hip::StarkJitDesc h;
    const uint16_t *instrs = reinterpret_cast<const uint16_t *>(d->h_instrs);
    h.instrs.assign(instrs, instrs + 4ull * d->num_instrs);
    for (uint32_t i = 0; i < d->num_immediates; i++) h.imms.push_back(d->h_immediates[i] % P);
    h.num_challenges = d->num_challenges, h.qdf = d->constraint_degree > 2 ? d->constraint_degree - 1 : 1;
    if (d->num_pairs) {
        h.pair_bounds.assign(d->h_pair_bounds, d->h_pair_bounds + d->num_pairs + 1);
        h.column_pairs.assign(d->h_column_pairs, d->h_column_pairs + 2ull * d->h_pair_bounds[d->num_pairs]);
    }
    return h;
}

void stark_host_ctl(plonky2_hip::StarkJitDesc *h, const GlStarkTablesDesc *d, const std::vector<uint32_t> &zs) {
    const uint32_t ncol = d->num_ctl_columns, ntw = d->num_twcs, nterms = d->h_column_bounds[ncol];
    h->term_columns.assign(d->h_term_columns, d->h_term_columns + nterms);
    for (uint32_t j = 0; j < nterms; j++) h->term_coeffs.push_back(d->h_term_coeffs[j] % P);
    h->column_bounds.assign(d->h_column_bounds, d->h_column_bounds + ncol + 1);
    for (uint32_t k = 0; k < ncol; k++) h->column_constants.push_back(d->h_column_constants[k] % P);
    h->twc_column_bounds.assign(d->h_twc_column_bounds, d->h_twc_column_bounds + ntw + 1);
    h->twc_filter.assign(d->h_twc_filter, d->h_twc_filter + ntw);
    h->ctl_zs = zs;
}

GlError stark_tables_check(uint32_t hasher, const GlStarkTablesDesc *d, std::vector<std::vector<uint32_t>> *zs_out) {
    if (d->struct_size != sizeof(GlStarkTablesDesc)) return struct_size_error("GlStarkTablesDesc");
    if (!d->num_tables || !d->tables) return fail(GL_E_INVALID, "no tables");
    if (!d->num_lookups || !d->num_twcs || !d->h_lookup_bounds || !d->h_twc_table || !d->h_twc_column_bounds || !d->h_twc_filter || !d->h_column_bounds ||
        (d->num_ctl_columns && !d->h_column_constants))
        return fail(GL_E_INVALID, "No CTL? (null or empty cross-table lookup arrays)");
    const uint32_t nt = d->num_tables, ncol = d->num_ctl_columns, ntw = d->num_twcs, nl = d->num_lookups;
    auto bounds_ok = [](const uint32_t *b, uint32_t count, uint32_t limit) {
        if (b[0] != 0) return false;
        for (uint32_t i = 0; i < count; i++)
            if (b[i + 1] < b[i]) return false;
        return b[count] <= limit;
    };
    if (!bounds_ok(d->h_column_bounds, ncol, 0xFFFFFFFFu)) return fail(GL_E_INVALID, "h_column_bounds must start at 0 and not decrease");
    const uint32_t nterms = d->h_column_bounds[ncol];
    if (nterms && (!d->h_term_columns || !d->h_term_coeffs)) return fail(GL_E_INVALID, "null pointer");
    if (!bounds_ok(d->h_twc_column_bounds, ntw, ncol)) return fail(GL_E_INVALID, "h_twc_column_bounds must start at 0, not decrease and stay within the CTL columns");
    if (!bounds_ok(d->h_lookup_bounds, nl, ntw)) return fail(GL_E_INVALID, "h_lookup_bounds must start at 0, not decrease and stay within the TWCs");
    const uint32_t nch = d->tables[0].num_challenges;
    for (uint32_t k = 0; k < nt; k++) {
        const GlStarkDesc &t = d->tables[k], &t0 = d->tables[0];
        if (t.struct_size != sizeof(GlStarkDesc)) return struct_size_error("GlStarkDesc");
        if (t.num_challenges != t0.num_challenges || t.fri.rate_bits != t0.fri.rate_bits || t.fri.cap_height != t0.fri.cap_height ||
            t.fri.proof_of_work_bits != t0.fri.proof_of_work_bits || t.fri.num_query_rounds != t0.fri.num_query_rounds || (t.fri.hiding != 0) != (t0.fri.hiding != 0))
            return fail(GL_E_INVALID, "table " + std::to_string(k) + ": the tables share one StarkConfig (num_challenges, rate_bits, cap_height, proof_of_work_bits, num_query_rounds, hiding); only reduction_arity_bits may differ");
        if (t.num_public_inputs) return fail(GL_E_INVALID, "table " + std::to_string(k) + ": a table of a multi-table STARK has no public inputs");
    }
    // a CTL column as used by a TWC of table `table`: its terms name columns of that table
    auto column_ok = [&](uint32_t col, uint32_t table) {
        for (uint32_t j = d->h_column_bounds[col]; j < d->h_column_bounds[col + 1]; j++)
            if (d->h_term_columns[j] >= d->tables[table].num_columns) return false;
        return true;
    };
    for (uint32_t t = 0; t < ntw; t++) {
        if (d->h_twc_table[t] >= nt) return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": table out of range");
        if (d->h_twc_filter[t] != GL_CTL_NO_FILTER && d->h_twc_filter[t] >= ncol) return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": filter column out of range");
        for (uint32_t k = d->h_twc_column_bounds[t]; k < d->h_twc_column_bounds[t + 1]; k++)
            if (!column_ok(k, d->h_twc_table[t])) return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": a term's column is out of range for its table");
        if (d->h_twc_filter[t] != GL_CTL_NO_FILTER && !column_ok(d->h_twc_filter[t], d->h_twc_table[t]))
            return fail(GL_E_INVALID, "TWC " + std::to_string(t) + ": a term's column of the filter is out of range for its table");
    }
    std::vector<std::vector<uint32_t>> &zs = *zs_out;
    zs.assign(nt, {});
    std::vector<bool> filtered(nt, false), unfiltered(nt, false);
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t lo = d->h_lookup_bounds[l], hi = d->h_lookup_bounds[l + 1];
        if (hi - lo < 2) return fail(GL_E_INVALID, "lookup " + std::to_string(l) + ": a lookup has at least one looking table and the looked table");
        const uint32_t width = d->h_twc_column_bounds[lo + 1] - d->h_twc_column_bounds[lo];
        const bool has_filter = d->h_twc_filter[lo] != GL_CTL_NO_FILTER;
        for (uint32_t t = lo; t < hi; t++) {
            if (d->h_twc_column_bounds[t + 1] - d->h_twc_column_bounds[t] != width) return fail(GL_E_INVALID, "lookup " + std::to_string(l) + ": its tables have unequal numbers of columns");
            if ((d->h_twc_filter[t] != GL_CTL_NO_FILTER) != has_filter)
                return fail(GL_E_INVALID, "lookup " + std::to_string(l) + ": either every table of a lookup has a filter column or none has (CrossTableLookup::new)");
            (has_filter ? filtered : unfiltered)[d->h_twc_table[t]] = true;
        }
        for (uint32_t c = 0; c < nch; c++)
            for (uint32_t t = lo; t < hi; t++) zs[d->h_twc_table[t]].push_back(t), zs[d->h_twc_table[t]].push_back(c);
    }
    for (uint32_t k = 0; k < nt; k++) {
        if (zs[k].empty()) return fail(GL_E_INVALID, "No CTL? (no lookup names table " + std::to_string(k) + ")");
        if (filtered[k] && d->tables[k].constraint_degree < 3) return fail(GL_E_INVALID, "table " + std::to_string(k) + ": the checks of a filtered CTL Z have degree 3: constraint_degree must be at least 3");
        if (d->tables[k].constraint_degree < 2) return fail(GL_E_INVALID, "table " + std::to_string(k) + ": the checks of a CTL Z have degree 2: constraint_degree must be at least 2");
        TRY(stark_check(hasher, &d->tables[k], (uint32_t)zs[k].size() / 2));
    }
    return ok();
}

// after stark_check
static GlError stark_build(uint32_t hasher, const GlStarkDesc *d, Stark **stark, void *ctx) {
    const uint32_t qdf = d->constraint_degree > 2 ? d->constraint_degree - 1 : 1;
    const uint32_t qdb = glh::log2_ceil(qdf);
    const uint32_t num_column_pairs = d->num_pairs ? d->h_pair_bounds[d->num_pairs] : 0;
    DeviceCall device_call(ctx);  // makes the context's device current before the first allocation
    std::unique_ptr<Stark> s(new Stark());  // deleted on every early return
    s->hasher = hasher;
    s->degree_bits = d->degree_bits, s->num_columns = d->num_columns, s->num_public_inputs = d->num_public_inputs;
    s->num_challenges = d->num_challenges, s->qdf = qdf, s->qdb = qdb, s->num_instrs = d->num_instrs, s->num_pairs = d->num_pairs;
    s->num_zs = d->num_pairs ? plonky2_hip::stark_num_zs(d->num_pairs, d->num_challenges, qdf) : 0;
    s->set_fri(d->fri);
    s->host = stark_host_desc(d);
    TRY(s->d_instrs.alloc(d->num_instrs));  // 8 bytes per GlGateInstr
    TRY(gl_memcpy_h2d(s->d_instrs.p, d->h_instrs, 8ull * d->num_instrs, ctx));
    if (d->num_immediates) {
        std::vector<uint64_t> imms(d->h_immediates, d->h_immediates + d->num_immediates);
        for (uint64_t &v : imms) v %= P;
        TRY(s->d_imms.alloc(imms.size()));
        TRY(gl_memcpy_h2d(s->d_imms.p, imms.data(), 8ull * imms.size(), ctx));
    }
    if (d->num_pairs) {
        TRY(s->d_column_pairs.alloc(num_column_pairs ? num_column_pairs : 1));  // two u32 per column pair
        TRY(gl_memcpy_h2d(s->d_column_pairs.p, d->h_column_pairs, 8ull * num_column_pairs, ctx));
        TRY(s->d_pair_bounds.alloc((d->num_pairs + 2) / 2));
        TRY(gl_memcpy_h2d(s->d_pair_bounds.p, d->h_pair_bounds, 4ull * (d->num_pairs + 1), ctx));
    }
    TRY(gl_ctx_synchronize(ctx));
    *stark = s.release();
    return ok();
}

// What a table of gl_stark_tables_prove brings to the flow of gl_stark_prove
struct CtlPart {
    Batch *trace;                     // committed before the transcript began
    plonky2_hip::StarkCtlDev ctl;     // ctl.num_zs CTL Zs behind the permutation Zs
    const uint64_t *d_ctl_zs;         // their values [ctl.num_zs][n]
    const uint64_t *h_ctl_challenges;
    uint64_t *d_transcript;           // the Challenger all tables share: compacted, never reset
    const uint64_t *h_filter_flag;    // page-locked; its copy is queued: valid after the next host synchronisation
};

// One STARK proof from the trace (commitment) to its bytes, appended to `out`: prove() of starky/src/prover.rs:32-195 with a fresh
// transcript and public inputs (ctl = null), or prove_single_table of evm/src/prover.rs:245-421 on the compacted shared transcript
// with the table's CTL Zs in the Zs oracle, their checks in the quotient and the third opening batch.
static GlError stark_prove_one(const Stark &c, const uint64_t *d_trace, const uint64_t *h_public_inputs, const CtlPart *ctl, Bytes &out, double *h_stage_ms,
                               void *ctx) {
    ProofSession s(c, h_stage_ms, ctx);  // the context's device is current; every DevBuf below comes from / returns to the handle's pool of this context
    const uint32_t db = c.degree_bits, nch = c.num_challenges, qdf = c.qdf, qdb = c.qdb, npi = c.num_public_inputs;
    const uint32_t nperm = c.num_zs, nctl = ctl ? ctl->ctl.num_zs : 0, nz = nperm + nctl;
    const uint64_t n = 1ull << db, n_ext = n << c.rate_bits, cap_words = 4ull << c.cap_height;
    const bool perm = c.num_pairs != 0, has_zs = nz != 0;

    // ---- the small-data side of the proof: one device buffer, one page-locked mirror ----
    // oracles: trace, [Zs], quotient (stark.rs:94-119)
    const uint32_t n_quot = nch * qdf;
    std::vector<uint32_t> leaf_len = {c.num_columns};
    if (has_zs) leaf_len.push_back(nz);
    leaf_len.push_back(n_quot);
    FriLayout L;
    TRY(fri_shapes(c, &L));
    const Span T = s.take(32), hostin = s.take(npi);
    const Span fetch0 = s.take(0);  // from here on: what the host fetches
    const Span perm_s = s.take(perm ? 2ull * qdf * nch : 0), alphas_s = s.take(nch), zeta_s = s.take(2);
    // openings at zeta and g * zeta: [2][n_polys] extension elements for the trace and the Zs, [1][n_polys] for the quotient; the CTL
    // Zs at 1 / g as extension elements (x, 0)
    const Span open_trace = s.take(4ull * c.num_columns), open_zs = s.take(4ull * nz), open_quot = s.take(2ull * n_quot), open_last = s.take(2ull * nctl);
    const Span cap_trace = s.take(cap_words), cap_zs = s.take(has_zs ? cap_words : 0), cap_quot = s.take(cap_words);
    fri_layout(c, leaf_len, &s.sd, &L);
    TRY(s.begin());
    uint64_t *const D = s.D, *const H = s.H;
    for (uint32_t i = 0; i < npi; i++) H[hostin.off + i] = h_public_inputs[i] % P;
    TRY(s.upload(hostin));

    // trace commitment (prover.rs:57-70); the caller's trace stays intact
    Batch own_trace;
    if (!ctl)
        TRY(commit_copy(&own_trace, d_trace, c.num_columns, c, ctx, nullptr));
    else
        TRY(gl_memcpy_d2d(D + T.off, ctl->d_transcript, 32 * 8, ctx));  // the shared transcript runs on in this proof's buffer
    Batch &trace = ctl ? *ctl->trace : own_trace;
    TRY(s.st.mark(0));
    // On its own: a fresh Challenger observes the trace cap (prover.rs:72-74), nothing else. As a table: the shared Challenger has
    // observed every trace cap already and is compacted (evm/src/prover.rs:271).
    const uint32_t begin = ctl ? GL_CHALLENGER_COMPACT : GL_CHALLENGER_RESET;
    auto filter_check = [&]() { return ctl && *ctl->h_filter_flag ? fail(GL_E_INVALID, "Non-binary filter?") : ok(); };
    Batch zs;
    std::vector<uint64_t> perm_challenges;
    if (has_zs) {
        DevBuf z;
        TRY(z.alloc((uint64_t)nz * n));
        if (perm) {
            // get_n_permutation_challenge_sets (permutation.rs:153-179): qdf sets of num_challenges (beta, gamma) draws
            if (ctl)
                TRY(s.step(T, {}, 2 * qdf * nch, perm_s, begin));
            else
                TRY(s.step(T, {c.hashes(trace.cap_d.p, cap_words)}, 2 * qdf * nch, perm_s, begin));
            TRY(s.fetch(perm_s));
            TRY(s.sync());
            TRY(filter_check());
            perm_challenges.assign(H + perm_s.off, H + perm_s.off + 2ull * qdf * nch);
            TRY(gl_stark_permutation_zs(&c, d_trace, n, perm_challenges.data(), z.p, ctx));
        }
        // the Zs oracle: permutation Zs, then CTL Zs (evm/src/prover.rs:290-311)
        if (nctl) TRY(gl_memcpy_d2d(z.p + (uint64_t)nperm * n, ctl->d_ctl_zs, 8ull * nctl * n, ctx));
        TRY(s.st.mark(1));
        TRY(commit(&zs, std::move(z), true, nz, c, ctx, nullptr, false));
        TRY(s.st.mark(2));
        TRY(s.step(T, {c.hashes(zs.cap_d.p, cap_words)}, nch, alphas_s, perm ? 0 : begin));
    } else {
        TRY(s.step(T, {c.hashes(trace.cap_d.p, cap_words)}, nch, alphas_s, begin));
    }
    TRY(s.fetch(alphas_s));
    TRY(s.sync());
    TRY(filter_check());
    const std::vector<uint64_t> alphas(H + alphas_s.off, H + alphas_s.off + nch);
    // quotient polynomials (prover.rs:115-123)
    DevBuf quotient;
    TRY(quotient.alloc((uint64_t)nch << (db + qdb)));
    TRY(stark_quotient(c, trace.lde.p, has_zs ? zs.lde.p : nullptr, n_ext, alphas.data(), perm ? perm_challenges.data() : nullptr, D + hostin.off,
                       quotient.p, ctx, ctl ? &ctl->ctl : nullptr, ctl ? ctl->h_ctl_challenges : nullptr));
    TRY(s.st.mark(3));
    // trim_to_len(degree * qdf) and the split into degree-n chunks (prover.rs:124-133), committed from coefficients
    Batch quot;
    TRY(commit_quotient_chunks(&quot, std::move(quotient), nch, qdf, qdb, c, ctx, nullptr));
    TRY(s.st.mark(4));
    TRY(s.step(T, {c.hashes(quot.cap_d.p, cap_words)}, 2, zeta_s));
    TRY(s.fetch(zeta_s));
    TRY(s.sync());
    const E2 zeta{H[zeta_s.off], H[zeta_s.off + 1]};
    if (E2 zn = e2_pow(zeta, n); zn.a == 1 && zn.b == 0) return fail(GL_E_INVALID, "Opening point is in the subgroup.");
    const uint64_t g = glh::root_of_unity(db);
    const E2 g_zeta = e2_mul(E2{g, 0}, zeta), g_inv{glh::inv(g), 0};
    // StarkOpeningSet::new (proof.rs:138-159; evm/src/proof.rs:190-224): trace and Zs at zeta and g * zeta, the quotient at zeta, the
    // CTL Zs at the last element of the subgroup
    {
        const uint64_t pts[4] = {zeta.a, zeta.b, g_zeta.a, g_zeta.b}, last[2] = {g_inv.a, g_inv.b};
        TRY(gl_eval_polys_ext2(trace.coeffs.p, c.num_columns, db, n, pts, 2, D + open_trace.off, ctx));
        if (has_zs) TRY(gl_eval_polys_ext2(zs.coeffs.p, nz, db, n, pts, 2, D + open_zs.off, ctx));
        TRY(gl_eval_polys_ext2(quot.coeffs.p, n_quot, db, n, pts, 1, D + open_quot.off, ctx));
        if (nctl) TRY(gl_eval_polys_ext2(zs.coeffs.p + (uint64_t)nperm * n, nctl, db, n, last, 1, D + open_last.off, ctx));
    }
    TRY(s.st.mark(5));
    // to_fri_openings (proof.rs:161-182): [local_values, permutation_zs, quotient_polys], then [next_values, permutation_zs_next], then
    // with CTLs [ctl_zs_last]; the instance of stark.rs:88-137 (evm/src/stark.rs:83-142): batch 0 everything at zeta, batch 1 trace then
    // Zs at g * zeta, batch 2 the CTL Zs at 1 / g
    std::vector<const Batch *> oracles = {&trace};
    if (has_zs) oracles.push_back(&zs);
    oracles.push_back(&quot);
    uint64_t pow_witness = 0;
    {
        std::vector<FriBatch> batches(nctl ? 3 : 2);
        batches[0].point = zeta, batches[1].point = g_zeta;
        for (const Batch *o : oracles)
            for (uint32_t k = 0; k < o->n_polys; k++) batches[0].polys.push_back(o->coeffs.p + (uint64_t)k * n);
        for (size_t o = 0; o + 1 < oracles.size(); o++)
            for (uint32_t k = 0; k < oracles[o]->n_polys; k++) batches[1].polys.push_back(oracles[o]->coeffs.p + (uint64_t)k * n);
        if (nctl) {
            batches[2].point = g_inv;
            for (uint32_t k = nperm; k < nz; k++) batches[2].polys.push_back(zs.coeffs.p + (uint64_t)k * n);
        }
        std::vector<GlObserveSrc> srcs = {GlObserveSrc{D + open_trace.off, 2ull * c.num_columns, 0}};
        if (has_zs) srcs.push_back(GlObserveSrc{D + open_zs.off, 2ull * nz, 0});
        srcs.push_back(GlObserveSrc{D + open_quot.off, 2ull * n_quot, 0});
        srcs.push_back(GlObserveSrc{D + open_trace.off + 2ull * c.num_columns, 2ull * c.num_columns, 0});
        if (has_zs) srcs.push_back(GlObserveSrc{D + open_zs.off + 2ull * nz, 2ull * nz, 0});
        if (nctl) srcs.push_back(GlObserveSrc{D + open_last.off, 2ull * nctl, 0});
        TRY(fri_prove(c, L, s, T, oracles, srcs, batches, &pow_witness));
    }
    if (ctl) TRY(gl_memcpy_d2d(ctl->d_transcript, D + T.off, 32 * 8, ctx));  // the next table goes on from here
    // everything the proof consists of, in one go
    TRY(gl_memcpy_d2d(D + cap_trace.off, trace.cap_d.p, cap_words * 8, ctx));
    if (has_zs) TRY(gl_memcpy_d2d(D + cap_zs.off, zs.cap_d.p, cap_words * 8, ctx));
    TRY(gl_memcpy_d2d(D + cap_quot.off, quot.cap_d.p, cap_words * 8, ctx));
    TRY(s.fetch(Span{fetch0.off, s.sd.top - fetch0.off}));
    TRY(gl_ctx_synchronize(ctx));
    TRY(s.st.mark(9));
    TRY(fri_check_pow(c, L, H, pow_witness));
    // ---- the wire format of StarkProofWithPublicInputs / of one StarkProof of the tables (include/plonky2_hip.h) ----
    out.keccak = c.keccak();
    out.hashes(H + cap_trace.off, cap_words / 4);
    if (has_zs) out.hashes(H + cap_zs.off, cap_words / 4);
    out.hashes(H + cap_quot.off, cap_words / 4);
    out.fields(H + open_trace.off, 4ull * c.num_columns);  // local_values, next_values
    if (has_zs) out.fields(H + open_zs.off, 4ull * nz);    // permutation_zs, permutation_zs_next
    for (uint32_t k = 0; k < nctl; k++) out.field(H[open_last.off + 2ull * k]);  // ctl_zs_last: base field elements
    out.fields(H + open_quot.off, 2ull * n_quot);          // quotient_polys
    fri_write(out, c, L, H, oracles, pow_witness);
    out.fields(H + hostin.off, npi);
    return s.st.mark(10);
}

}  // namespace plonky2_hip

extern "C" {

GlError gl_stark_create(uint32_t hasher, const GlStarkDesc *d, void **stark, void *ctx) {
    if (!d || !stark || !ctx) return fail(GL_E_INVALID, "null pointer");
    TRY(stark_check(hasher, d, 0));
    Stark *s = nullptr;
    TRY(stark_build(hasher, d, &s, ctx));
    *stark = s;
    return ok();
}

void gl_stark_destroy(void *stark) { delete static_cast<Stark *>(stark); }

GlError gl_stark_trim(void *stark) {
    if (!stark) return fail(GL_E_INVALID, "null pointer");
    return static_cast<Stark *>(stark)->trim();
}

GlError gl_stark_permutation_zs(const void *stark, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_challenges, uint64_t *d_zs,
                                void *ctx) {
    if (!stark || !d_trace || !h_challenges || !d_zs || !ctx) return fail(GL_E_INVALID, "null pointer");
    const Stark &s = *static_cast<const Stark *>(stark);
    if (!s.num_pairs) return fail(GL_E_INVALID, "the STARK has no permutation pairs");
    if (trace_stride < (1ull << s.degree_bits)) return fail(GL_E_INVALID, "trace_stride smaller than the column length");
    const plonky2_hip::NttTables *tb;
    TRY(tables_of(ctx, &tb));
    const hipError_t e = plonky2_hip::stark_permutation_zs(*tb, d_trace, trace_stride, s.pairs(), h_challenges, s.num_challenges, s.qdf, s.degree_bits, d_zs,
                                                           ctx_stream(ctx));
    if (e != hipSuccess) return hip_fail(e, "stark_permutation_zs");
    return ok();
}

// gl_stark_quotient_polys, and with `ctl` gl_stark_tables_quotient_polys
static GlError quotient_polys_call(const Stark &s, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde, uint64_t column_stride, const uint64_t *h_alphas,
                                   const uint64_t *h_challenges, const uint64_t *h_public_inputs, uint64_t *d_quotient_polys, void *ctx,
                                   const plonky2_hip::StarkCtlDev *ctl, const uint64_t *h_ctl_challenges) {
    if (s.num_pairs && (!d_zs_lde || !h_challenges)) return fail(GL_E_INVALID, "the STARK has permutation pairs: d_zs_lde and h_challenges are needed");
    if (s.num_public_inputs && !h_public_inputs) return fail(GL_E_INVALID, "null public inputs");
    if (column_stride < (1ull << (s.degree_bits + s.rate_bits))) return fail(GL_E_INVALID, "column_stride smaller than the LDE's column length n << rate_bits");
    DeviceCall device_call(ctx);  // the context's device becomes current
    DevBuf pis;
    TRY(pis.alloc(s.num_public_inputs));
    std::vector<uint64_t> h_pis(s.num_public_inputs);
    for (uint32_t i = 0; i < s.num_public_inputs; i++) h_pis[i] = h_public_inputs[i] % P;
    TRY(gl_memcpy_h2d(pis.p, h_pis.data(), 8ull * h_pis.size(), ctx));
    TRY(stark_quotient(s, d_trace_lde, d_zs_lde, column_stride, h_alphas, h_challenges, pis.p, d_quotient_polys, ctx, ctl, h_ctl_challenges));
    return gl_ctx_synchronize(ctx);  // pis is freed on return
}

GlError gl_stark_quotient_polys(const void *stark, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde, uint64_t column_stride,
                                const uint64_t *h_alphas, const uint64_t *h_challenges, const uint64_t *h_public_inputs,
                                uint64_t *d_quotient_polys, void *ctx) {
    if (!stark || !d_trace_lde || !h_alphas || !d_quotient_polys || !ctx) return fail(GL_E_INVALID, "null pointer");
    return quotient_polys_call(*static_cast<const Stark *>(stark), d_trace_lde, d_zs_lde, column_stride, h_alphas, h_challenges, h_public_inputs,
                               d_quotient_polys, ctx, nullptr, nullptr);
}

GlError gl_stark_prove(const void *stark, const uint64_t *d_trace, const uint64_t *h_public_inputs, uint8_t **proof, uint64_t *proof_len,
                       double *h_stage_ms, void *ctx) {
    if (!stark || !d_trace || !proof || !proof_len || !ctx) return fail(GL_E_INVALID, "null pointer");
    const Stark &c = *static_cast<const Stark *>(stark);
    if (c.num_public_inputs && !h_public_inputs) return fail(GL_E_INVALID, "null public inputs");
    if (h_stage_ms) memset(h_stage_ms, 0, sizeof(double) * GL_STARK_STAGES);
    Bytes out;
    TRY(stark_prove_one(c, d_trace, h_public_inputs, nullptr, out, h_stage_ms, ctx));
    return bytes_out(out, proof, proof_len);
}

GlError gl_stark_tables_create(uint32_t hasher, const GlStarkTablesDesc *d, void **tables, void *ctx) {
    if (!d || !tables || !ctx) return fail(GL_E_INVALID, "null pointer");
    std::vector<std::vector<uint32_t>> zs;  // per table (twc, challenge), cross_table_lookup_data's order
    TRY(stark_tables_check(hasher, d, &zs));
    const uint32_t nt = d->num_tables, ncol = d->num_ctl_columns, ntw = d->num_twcs, nterms = d->h_column_bounds[ncol];
    const uint32_t nch = d->tables[0].num_challenges;
    DeviceCall device_call(ctx);
    std::unique_ptr<StarkTables> T(new StarkTables());  // deleted, with its tables, on every early return
    T->hasher = hasher, T->num_challenges = nch;
    T->set_fri(d->tables[0].fri);
    for (uint32_t k = 0; k < nt; k++) {
        Stark *s = nullptr;
        TRY(stark_build(hasher, &d->tables[k], &s, ctx));
        stark_host_ctl(&s->host, d, zs[k]);
        T->tables.push_back(s);
    }
    auto upload32 = [&](DevBuf &b, const uint32_t *src, uint64_t count) -> GlError {
        TRY(b.alloc((count + 1) / 2));
        return count ? gl_memcpy_h2d(b.p, src, 4 * count, ctx) : ok();
    };
    auto upload64 = [&](DevBuf &b, const uint64_t *src, uint64_t count) -> GlError {
        std::vector<uint64_t> v(src, src + count);
        for (uint64_t &x : v) x %= P;
        TRY(b.alloc(count));
        return count ? gl_memcpy_h2d(b.p, v.data(), 8 * count, ctx) : ok();
    };
    TRY(upload32(T->d_term_columns, d->h_term_columns, nterms));
    TRY(upload64(T->d_term_coeffs, d->h_term_coeffs, nterms));
    TRY(upload32(T->d_column_bounds, d->h_column_bounds, ncol + 1ull));
    TRY(upload64(T->d_column_constants, d->h_column_constants, ncol));
    TRY(upload32(T->d_twc_column_bounds, d->h_twc_column_bounds, ntw + 1ull));
    TRY(upload32(T->d_twc_filter, d->h_twc_filter, ntw));
    T->d_zs.resize(nt);
    for (uint32_t k = 0; k < nt; k++) {
        TRY(upload32(T->d_zs[k], zs[k].data(), zs[k].size()));
        T->num_ctl_zs.push_back((uint32_t)zs[k].size() / 2);
    }
    TRY(gl_ctx_synchronize(ctx));
    *tables = T.release();
    return ok();
}

void gl_stark_tables_destroy(void *tables) { delete static_cast<StarkTables *>(tables); }

GlError gl_stark_tables_trim(void *tables) {
    if (!tables) return fail(GL_E_INVALID, "null pointer");
    StarkTables *T = static_cast<StarkTables *>(tables);
    for (Stark *s : T->tables) TRY(s->trim());
    return T->trim();
}

// the CTL Zs of table k; *d_flag is raised by a non-binary filter
static GlError tables_ctl_zs(const StarkTables &T, uint32_t k, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_ctl_challenges,
                             uint64_t *d_zs, uint64_t *d_flag, void *ctx) {
    const plonky2_hip::NttTables *tb;
    TRY(tables_of(ctx, &tb));
    const hipError_t e = plonky2_hip::stark_ctl_zs(*tb, d_trace, trace_stride, T.ctl(k), h_ctl_challenges, T.num_challenges, T.tables[k]->degree_bits, d_zs,
                                                   d_flag, ctx_stream(ctx));
    if (e == hipErrorInvalidValue) return fail(GL_E_INVALID, "inconsistent arguments of the CTL Zs (trace_stride / sizes / more Zs than the context's scratch holds block totals for)");
    if (e != hipSuccess) return hip_fail(e, "stark_ctl_zs");
    return ok();
}

GlError gl_stark_tables_ctl_zs(const void *tables, uint32_t table, const uint64_t *d_trace, uint64_t trace_stride, const uint64_t *h_ctl_challenges,
                               uint64_t *d_zs, void *ctx) {
    if (!tables || !d_trace || !h_ctl_challenges || !d_zs || !ctx) return fail(GL_E_INVALID, "null pointer");
    const StarkTables &T = *static_cast<const StarkTables *>(tables);
    if (table >= T.tables.size()) return fail(GL_E_INVALID, "table out of range");
    if (trace_stride < (1ull << T.tables[table]->degree_bits)) return fail(GL_E_INVALID, "trace_stride smaller than the column length");
    DeviceCall device_call(ctx);
    DevBuf flag;
    TRY(flag.alloc(1));
    TRY(gl_memset_zero(flag.p, 8, ctx));
    TRY(tables_ctl_zs(T, table, d_trace, trace_stride, h_ctl_challenges, d_zs, flag.p, ctx));
    uint64_t h_flag = 0;
    TRY(gl_memcpy_d2h(&h_flag, flag.p, 8, ctx));  // synchronous
    if (h_flag) return fail(GL_E_INVALID, "Non-binary filter?");
    return ok();
}

GlError gl_stark_tables_quotient_polys(const void *tables, uint32_t table, const uint64_t *d_trace_lde, const uint64_t *d_zs_lde,
                                       uint64_t column_stride, const uint64_t *h_alphas, const uint64_t *h_perm_challenges,
                                       const uint64_t *h_ctl_challenges, uint64_t *d_quotient_polys, void *ctx) {
    if (!tables || !d_trace_lde || !d_zs_lde || !h_alphas || !h_ctl_challenges || !d_quotient_polys || !ctx) return fail(GL_E_INVALID, "null pointer");
    const StarkTables &T = *static_cast<const StarkTables *>(tables);
    if (table >= T.tables.size()) return fail(GL_E_INVALID, "table out of range");
    const plonky2_hip::StarkCtlDev ctl = T.ctl(table);
    return quotient_polys_call(*T.tables[table], d_trace_lde, d_zs_lde, column_stride, h_alphas, h_perm_challenges, nullptr, d_quotient_polys, ctx, &ctl,
                               h_ctl_challenges);
}

GlError gl_stark_tables_prove(const void *tables, const uint64_t *const *d_traces, uint8_t **proof, uint64_t *proof_len, double *h_stage_ms,
                              void *ctx) {
    if (!tables || !d_traces || !proof || !proof_len || !ctx) return fail(GL_E_INVALID, "null pointer");
    const StarkTables &T = *static_cast<const StarkTables *>(tables);
    const uint32_t nt = (uint32_t)T.tables.size(), nch = T.num_challenges;
    for (uint32_t k = 0; k < nt; k++)
        if (!d_traces[k]) return fail(GL_E_INVALID, "null trace");
    // the tables' pool: the trace commitments, the CTL Zs and the shared small data (a table's own buffers: its Stark's pool); clocks run per table
    ProofSession s(T, nullptr, ctx);
    if (h_stage_ms) memset(h_stage_ms, 0, sizeof(double) * GL_STARK_STAGES * nt);
    auto ms = [&](uint32_t k) { return h_stage_ms ? h_stage_ms + (size_t)GL_STARK_STAGES * k : nullptr; };
    const uint64_t cap_words = 4ull << T.cap_height;
    const Span TR = s.take(32), chal_s = s.take(2ull * nch), flag_s = s.take(1);
    TRY(s.begin());
    uint64_t *const D = s.D, *const H = s.H;
    TRY(gl_memset_zero(D + flag_s.off, 8, ctx));
    // every trace is committed before the transcript begins (evm/src/prover.rs:86-118) and stays until its table is proved
    std::vector<Batch> traces(nt);
    for (uint32_t k = 0; k < nt; k++) {
        const Stark &c = *T.tables[k];
        Stages st(ms(k), ctx);
        TRY(commit_copy(&traces[k], d_traces[k], c.num_columns, c, ctx, nullptr));
        TRY(st.mark(0));
    }
    // a fresh Challenger observes all trace caps, then get_grand_product_challenge_set (cross_table_lookup.rs:243)
    for (uint32_t k = 0; k < nt; k += 8) {
        std::vector<GlObserveSrc> srcs;
        for (uint32_t j = k; j < nt && j < k + 8; j++) srcs.push_back(T.hashes(traces[j].cap_d.p, cap_words));
        const bool last = k + 8 >= nt;
        TRY(s.step(TR, srcs, last ? 2 * nch : 0, chal_s, k == 0 ? GL_CHALLENGER_RESET : 0));
    }
    TRY(s.fetch(chal_s));
    TRY(s.sync());
    const std::vector<uint64_t> ctl_challenges(H + chal_s.off, H + chal_s.off + 2ull * nch);
    std::vector<DevBuf> ctl_zs(nt);
    for (uint32_t k = 0; k < nt; k++) {
        const Stark &c = *T.tables[k];
        Stages st(ms(k), ctx);
        TRY(ctl_zs[k].alloc((uint64_t)T.num_ctl_zs[k] << c.degree_bits));
        TRY(tables_ctl_zs(T, k, d_traces[k], 1ull << c.degree_bits, ctl_challenges.data(), ctl_zs[k].p, D + flag_s.off, ctx));
        TRY(st.mark(1));
    }
    H[flag_s.off] = 0;
    TRY(s.fetch(flag_s));  // read at the first table's first synchronisation
    Bytes out;
    for (uint32_t k = 0; k < nt; k++) {
        CtlPart part{&traces[k], T.ctl(k), ctl_zs[k].p, ctl_challenges.data(), D + TR.off, H + flag_s.off};
        TRY(stark_prove_one(*T.tables[k], d_traces[k], nullptr, &part, out, ms(k), ctx));
        traces[k] = Batch();  // this table's trace LDE and CTL Zs return to the pool
        ctl_zs[k].reset();
    }
    return bytes_out(out, proof, proof_len);
}

}  // extern "C"
