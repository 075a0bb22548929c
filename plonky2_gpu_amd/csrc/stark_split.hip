// stark_split.hip — cuts a STARK's register program into unit programs (stark_split.h).
//
// The constraints of a program share nothing but the consumer's running sums: EMIT k only appends its value to the Horner chain.
// So a contiguous run of EMITs together with everything those EMITs read is a program of its own, and the runs in order feed the
// consumer the same values in the same order. "Everything they read" is the backward slice under "the latest write of that
// register": walking from the run's last EMIT to instruction 0 with the set of registers whose value is still wanted,
//   * an instruction that writes a wanted register is kept, the register is no longer wanted above it, its sources are;
//   * an instruction that writes an unwanted register is dropped: the next kept reader of that register below it reads a later
//     write (else the register would be wanted here), so the dropped value reaches nothing that is kept;
//   * a kept ACCR wants every ACC of its accumulator back to the previous ACCR of that accumulator, kept or not: a dropped ACCR
//     only zeroed an accumulator all of whose earlier ACCs are dropped with it, and accumulators start at 0;
//   * the EMITs of other runs are dropped.
// Order and register numbers are the original's, so nothing is renamed, and every check of stark_program_validate that held for
// the program holds for the slice: reads follow the same writes, an ACCR keeps all of its ACCs (a subset of none, so the
// overflow bound can only shrink), every unit has an EMIT.
#include "stark_split.h"

#include <algorithm>

#include "program_isa.h"

namespace plonky2_hip {

namespace {

// The slice of EMITs number s .. e (emit_pcs) as the flags of the kept instructions in `keep` (if not null); returns its length,
// or a value above `limit` as soon as the length passes it.
uint64_t slice(const uint16_t *instrs, const std::vector<uint32_t> &emit_pcs, uint32_t s, uint32_t e, uint64_t limit, std::vector<uint8_t> *keep) {
    uint64_t want = 0, count = 0;  // registers whose value a kept instruction below reads
    uint32_t want_acc = 0;         // accumulators whose ACCs a kept ACCR below sums
    const uint32_t first = emit_pcs[s];
    for (uint32_t pc = emit_pcs[e] + 1; pc-- > 0;) {
        if (pc < first && !want && !want_acc) break;
        const isa::Instr in = isa::instr_at(instrs, pc);
        bool kept = false;
        if (isa::is_emit(in.op)) {
            kept = pc >= first;
        } else if (isa::acc_in_dst(in.op)) {
            kept = want_acc >> (in.dst & (isa::MAX_ACCS - 1)) & 1;
        } else if (isa::writes_reg(in.op)) {
            const uint64_t bit = 1ull << (in.dst & (isa::MAX_REGS - 1));
            kept = want & bit;
            want &= ~bit;  // before the sources: ADD r, r, x reads the earlier r
            if (isa::acc_in_a(in.op)) want_acc = (want_acc & ~(1u << (in.a & (isa::MAX_ACCS - 1)))) | ((uint32_t)kept << (in.a & (isa::MAX_ACCS - 1)));
        }
        if (!kept) continue;
        if (isa::reads_a(in.op)) want |= 1ull << (in.a & (isa::MAX_REGS - 1));
        if (isa::reads_b(in.op)) want |= 1ull << (in.b & (isa::MAX_REGS - 1));
        if (keep) (*keep)[pc] = 1;
        if (++count > limit) return count;
    }
    return count;
}

}  // namespace

std::vector<StarkProgramUnit> stark_program_split(const uint16_t *instrs, uint32_t num_instrs, uint32_t max_unit_instrs) {
    std::vector<uint32_t> emit_pcs;
    for (uint32_t pc = 0; pc < num_instrs; pc++)
        if (isa::is_emit(instrs[4ull * pc])) emit_pcs.push_back(pc);
    const uint32_t emits = (uint32_t)emit_pcs.size();
    std::vector<StarkProgramUnit> units;
    if (max_unit_instrs >= num_instrs || !emits) {
        StarkProgramUnit u;
        u.instrs.assign(instrs, instrs + 4ull * num_instrs);
        u.emit_end = emits;
        units.push_back(std::move(u));
        return units;
    }
    std::vector<uint8_t> keep(num_instrs);
    for (uint32_t s = 0; s < emits;) {
        uint32_t e = s;
        while (e + 1 < emits && slice(instrs, emit_pcs, s, e + 1, max_unit_instrs, nullptr) <= max_unit_instrs) e++;
        std::fill(keep.begin(), keep.end(), 0);
        slice(instrs, emit_pcs, s, e, ~0ull, &keep);
        StarkProgramUnit u;
        u.emit_start = s, u.emit_end = e + 1;
        for (uint32_t pc = 0; pc <= emit_pcs[e]; pc++)
            if (keep[pc]) u.instrs.insert(u.instrs.end(), instrs + 4ull * pc, instrs + 4ull * pc + 4);
        units.push_back(std::move(u));
        s = e + 1;
    }
    return units;
}

}  // namespace plonky2_hip
