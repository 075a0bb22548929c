// program_isa.h — the register-program instruction set, once: GlGateInstr {op, dst, a, b} of include/plonky2_hip.h as the gate
// programs (plonk.hip, gate_jit.hip) and the STARK programs (stark.hip, stark_jit.hip) use it and program_asm.h's assemblers write it
// (gate_emit.hip: gates; <table>.hip: a table's program). 0..10 are common to both (1 is invalid in a STARK program), 11..14 STARK only.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace plonky2_hip {
namespace isa {

enum Op : uint16_t {
    LOAD_WIRE, LOAD_CONST, LOAD_PI, LOAD_IMM, ADD, SUB, MUL, EMIT, MULK, ACC, ACCR,  // include/plonky2_hip.h, GlGateInstr
    LOAD_NEXT, EMIT_TRANSITION, EMIT_FIRST_ROW, EMIT_LAST_ROW                         // ... and gl_stark_create
};
// one per value: the numbering include/plonky2_hip.h documents
static_assert(LOAD_WIRE == 0); static_assert(LOAD_CONST == 1); static_assert(LOAD_PI == 2); static_assert(LOAD_IMM == 3);
static_assert(ADD == 4); static_assert(SUB == 5); static_assert(MUL == 6); static_assert(EMIT == 7);
static_assert(MULK == 8); static_assert(ACC == 9); static_assert(ACCR == 10); static_assert(LOAD_NEXT == 11);
static_assert(EMIT_TRANSITION == 12); static_assert(EMIT_FIRST_ROW == 13); static_assert(EMIT_LAST_ROW == 14);

constexpr uint32_t MAX_REGS = 64, MAX_ACCS = 4;  // the device code masks indices with MAX - 1: powers of two

struct Instr { uint16_t op, dst, a, b; };
constexpr Instr instr_at(const uint16_t *instrs, size_t pc) { return Instr{instrs[4 * pc], instrs[4 * pc + 1], instrs[4 * pc + 2], instrs[4 * pc + 3]}; }

constexpr bool is_emit(uint16_t op) { return op == EMIT || (op >= EMIT_TRANSITION && op <= EMIT_LAST_ROW); }
constexpr bool reads_a(uint16_t op) { return op == ADD || op == SUB || op == MUL || op == MULK || op == ACC || is_emit(op); }  // a is a register
constexpr bool reads_b(uint16_t op) { return op == ADD || op == SUB || op == MUL; }  // b is a register
constexpr bool acc_in_dst(uint16_t op) { return op == ACC; }  // dst names an accumulator
constexpr bool acc_in_a(uint16_t op) { return op == ACCR; }  // a names an accumulator
constexpr bool writes_reg(uint16_t op) { return op <= EMIT_LAST_ROW && !is_emit(op) && !acc_in_dst(op); }  // dst is a register

// The ACC overflow contract of one accumulator: every weight below 2^32, and between two ACCRs the sum of weight * (2^32 - 1) below
// 2^63, so that neither 64-bit half can wrap (gl::fold96's precondition). The sum is kept in 128 bits: two weights near 2^32 pass 2^64.
struct AccBound {
    static constexpr unsigned __int128 LIMIT = (unsigned __int128)1 << 63;
    unsigned __int128 sum = 0;
    bool fits(unsigned __int128 weight) const { return weight < ((unsigned __int128)1 << 32) && sum + weight * 0xFFFFFFFFull < LIMIT; }
    bool add(unsigned __int128 weight) { return fits(weight) && (sum += weight * 0xFFFFFFFFull, true); }  // false: the contract is broken
    void reset() { sum = 0; }  // ACCR
};

}  // namespace isa
}  // namespace plonky2_hip
