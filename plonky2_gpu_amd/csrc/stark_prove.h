// stark_prove.h — what stark_compile.hip needs of the STARK handles of stark_prove.hip. Internal: nothing here is exported.
#pragma once
#include "prove_common.h"
#include "stark.h"
#include "stark_jit.h"

namespace plonky2_hip {

struct Stark : ProverShape {
    uint32_t num_columns = 0, num_public_inputs = 0, num_challenges = 0, qdf = 0, qdb = 0, num_instrs = 0, num_pairs = 0, num_zs = 0;
    DevBuf d_instrs, d_imms, d_column_pairs, d_pair_bounds;
    // the description on the host, for gl_stark_compile's generator; jit: the compiled quotient kernel that replaces the interpreter
    // from gl_stark_compile on (null: interpreted)
    StarkJitDesc host;
    StarkJitKernel *jit = nullptr;
    ~Stark() { stark_jit_destroy(jit); }
    StarkPairsDev pairs() const {
        StarkPairsDev p;
        p.column_pairs = reinterpret_cast<const uint32_t *>(d_column_pairs.p), p.pair_bounds = reinterpret_cast<const uint32_t *>(d_pair_bounds.p);
        p.num_pairs = num_pairs;
        return p;
    }
};

// ---- the tables of gl_stark_tables_create: one Stark per table, the CTL descriptors in device memory ----
struct StarkTables : ProverShape {  // a ProverShape for its pools: the trace commitments, the CTL Zs and the shared transcript of a proof
    std::vector<Stark *> tables;
    uint32_t num_challenges = 0;
    DevBuf d_term_columns, d_term_coeffs, d_column_bounds, d_column_constants, d_twc_column_bounds, d_twc_filter;
    std::vector<DevBuf> d_zs;          // per table: (twc, challenge) of its CTL Zs, in the order of cross_table_lookup_data
    std::vector<uint32_t> num_ctl_zs;  // per table
    ~StarkTables() {
        for (Stark *s : tables) delete s;
    }
    StarkCtlDev ctl(uint32_t k) const {
        auto u32 = [](const DevBuf &b) { return reinterpret_cast<const uint32_t *>(b.p); };
        StarkCtlDev c;
        c.term_columns = u32(d_term_columns), c.column_bounds = u32(d_column_bounds), c.twc_column_bounds = u32(d_twc_column_bounds);
        c.twc_filter = u32(d_twc_filter), c.zs = u32(d_zs[k]), c.term_coeffs = d_term_coeffs.p, c.column_constants = d_column_constants.p;
        c.num_zs = num_ctl_zs[k];
        return c;
    }
};

// Everything gl_stark_create refuses, before anything is allocated. num_ctl_zs: the CTL Zs a table of
// gl_stark_tables_create adds to the Zs oracle (0 for a STARK on its own).
GlError stark_check(uint32_t hasher, const GlStarkDesc *d, uint32_t num_ctl_zs);
// Everything gl_stark_tables_create refuses, before anything is allocated. zs: per table (twc, challenge) of its CTL Zs, in
// cross_table_lookup_data's order.
GlError stark_tables_check(uint32_t hasher, const GlStarkTablesDesc *d, std::vector<std::vector<uint32_t>> *zs_out);
// after stark_check: what the generator of the compiled quotient kernel reads (stark_jit.h), without the CTL part
StarkJitDesc stark_host_desc(const GlStarkDesc *d);
// the CTL part of table k's description: the arrays of all tables and the table's own CTL Zs
void stark_host_ctl(StarkJitDesc *h, const GlStarkTablesDesc *d, const std::vector<uint32_t> &zs);

}  // namespace plonky2_hip
