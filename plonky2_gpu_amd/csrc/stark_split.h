// stark_split.h — a long STARK register program cut into UNIT programs (stark_split.hip), so that gl_stark_compile_units compiles
// several short kernels instead of one long basic block. Pure host code: no device, no HIP.
#pragma once
#include <stdint.h>

#include <vector>

namespace plonky2_hip {

// One unit: a register program of its own (the encoding of program_isa.h, accepted by stark_program_validate wherever the whole
// program is) that yields the original program's EMITs number emit_start .. emit_end - 1, in order, with the same values.
struct StarkProgramUnit {
    std::vector<uint16_t> instrs;  // 4 per instruction
    uint32_t emit_start = 0, emit_end = 0;
};

// `instrs`: a program stark_program_validate has accepted. The units' EMIT runs are contiguous and partition the program's EMITs.
// A unit's body is the backward slice of its EMITs in the original order with the original register numbers; a value that lives
// across a cut is computed again in every unit that reads it. A unit is extended constraint by constraint while its slice has at
// most `max_unit_instrs` instructions; one constraint whose slice alone is longer is a unit of its own. max_unit_instrs >=
// num_instrs: one unit, the input word for word.
std::vector<StarkProgramUnit> stark_program_split(const uint16_t *instrs, uint32_t num_instrs, uint32_t max_unit_instrs);

}  // namespace plonky2_hip
