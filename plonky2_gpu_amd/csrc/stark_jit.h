// stark_jit.h — a STARK's constraint quotient as a RUN-TIME COMPILED kernel of its own (stark_jit.hip): what gate_jit.hip does for a
// circuit's gates, for the register program, the permutation checks and the cross-table-lookup checks of one STARK (one table).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "stark.h"

namespace plonky2_hip {

// What the generator reads: the validated description of one STARK on the host. Immediates, coefficients and constants are
// canonical. The CTL arrays are those of GlStarkTablesDesc (all tables'); `ctl_zs` holds (TWC, challenge) of THIS table's CTL Zs
// in the order of cross_table_lookup_data — empty for a STARK on its own.
struct StarkJitDesc {
    std::vector<uint16_t> instrs;  // 4 per instruction
    std::vector<uint64_t> imms;
    uint32_t num_challenges = 0, qdf = 0;
    std::vector<uint32_t> column_pairs, pair_bounds;  // pair_bounds empty without pairs
    std::vector<uint32_t> term_columns, column_bounds, twc_column_bounds, twc_filter, ctl_zs;
    std::vector<uint64_t> term_coeffs, column_constants;
    uint32_t num_pairs() const { return pair_bounds.empty() ? 0 : (uint32_t)pair_bounds.size() - 1; }
};

// straight-line HIP source of the kernel that replaces stark_quotient_values_kernel for this STARK
std::string stark_jit_source(const StarkJitDesc &d);

// Code objects of `sources` (equal sources are compiled once): from the kernel cache where it has them, else hiprtc, side by
// side on at most 8 threads, written to the cache. No device is touched. `written`: how many code objects were compiled.
bool stark_jit_compile_sources(const std::vector<std::string> &sources, std::vector<std::vector<char>> *codes, uint32_t *written, std::string *error);

struct StarkJitKernel;  // opaque: the code object and its module per device
// loads `code` on the current device; nullptr and `error` if it does not load
StarkJitKernel *stark_jit_load(const StarkJitDesc &d, const std::string &source, std::vector<char> &&code, std::string *error);
void stark_jit_destroy(StarkJitKernel *k);
const char *stark_jit_kernel_source(const StarkJitKernel *k);

// stark_quotient_values through the compiled kernel: same arguments (the program, the pair and CTL descriptors of `a` are not
// read: they are in the code), same output. hipErrorInvalidValue also where `a` does not have the shape the kernel was generated for.
hipError_t stark_jit_launch(const StarkJitKernel *k, const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, hipStream_t stream);

}  // namespace plonky2_hip
