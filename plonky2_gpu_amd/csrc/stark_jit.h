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

// The same description as SEVERAL kernels that run in order (stark_jit.hip, UNITS). A unit: a unit program of stark_program_split
// (stark_split.h; empty in the units behind the program) and a run check_start .. check_end - 1 of the checks behind the program
// — the permutation Zs' first-row checks, their batch checks, the CTL Zs, in the consumer's order.
struct StarkJitUnit {
    std::vector<uint16_t> instrs;
    uint32_t check_start = 0, check_end = 0;
};
constexpr uint32_t STARK_JIT_ONE_UNIT = 0xFFFFFFFFu;  // no cap: one unit, whose source is stark_jit_source's
// What gl_stark_compile_units takes for max_unit_instrs = 0: DESIGN.md 3.7.3 has the two measured curves it was read from.
constexpr uint32_t STARK_JIT_DEFAULT_UNIT_INSTRS = 1000;
// Never empty. The program is cut by the cap in instructions; the checks go into the last program unit while they fit — a check
// costs the field operations and consumer calls it generates — and into further units otherwise.
std::vector<StarkJitUnit> stark_jit_units(const StarkJitDesc &d, uint32_t max_unit_instrs);
// the source of one unit; first: the sums start at 0, else they are loaded from out; last: sj::tail, else the raw sums are stored
std::string stark_jit_unit_source(const StarkJitDesc &d, const StarkJitUnit &u, bool first, bool last);

// Code objects of `sources` (equal sources are compiled once): from the kernel cache where it has them, else hiprtc, side by
// side on at most 8 threads, written to the cache. No device is touched. `written`: how many code objects were compiled.
bool stark_jit_compile_sources(const std::vector<std::string> &sources, std::vector<std::vector<char>> *codes, uint32_t *written, std::string *error);

struct StarkJitKernel;  // opaque: the units' code objects and their modules per device
// loads the units' `codes` on the current device, all or none; nullptr and `error` if one does not load
StarkJitKernel *stark_jit_load(const StarkJitDesc &d, const std::vector<std::string> &sources, std::vector<std::vector<char>> &&codes, std::string *error);
void stark_jit_destroy(StarkJitKernel *k);
uint32_t stark_jit_kernel_units(const StarkJitKernel *k);
const char *stark_jit_kernel_source(const StarkJitKernel *k, uint32_t unit);  // nullptr beyond the units

// stark_quotient_values through the compiled kernel(s), the units in order on `stream`: same arguments (the program, the pair and CTL descriptors of `a` are not
// read: they are in the code), same output. hipErrorInvalidValue also where `a` does not have the shape the kernel was generated for.
hipError_t stark_jit_launch(const StarkJitKernel *k, const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, hipStream_t stream);

}  // namespace plonky2_hip
