// program_asm.h — the assembler of the register programs (host code only): GateAsm writes one gate's program (gate_emit.hip),
// StarkAsm on top of it a table's STARK program (the program() at the foot of each <table>.hip), and emit_table_program hands such
// a program out behind the C ABI. The instruction set is program_isa.h's; what the programs compute is stated where they are built.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/plonky2_hip.h"
#include "gl_field.h"
#include "program_isa.h"

namespace plonky2_hip {
namespace program_asm {

using namespace plonky2_hip::isa;  // the opcodes, MAX_REGS, AccBound

typedef unsigned __int128 u128;
constexpr uint64_t P = glh::P;
const u128 ACC_LIMIT = AccBound::LIMIT;  // each half of an accumulator stays below this (gl::fold96's precondition)

// Field constants referenced by LOAD_IMM / ACC, shared by all gates of a circuit (deduplicated)
struct ImmediatePool {
    std::vector<uint64_t> values;
    std::map<uint64_t, uint32_t> index_of;
    uint32_t index(u128 value) {
        const uint64_t v = (uint64_t)(value % P);
        auto it = index_of.find(v);
        if (it != index_of.end()) return it->second;
        if (values.size() >= 65536) throw std::runtime_error("more than 65536 distinct immediates");
        const uint32_t i = (uint32_t)values.size();
        index_of[v] = i;
        values.push_back(v);
        return i;
    }
};

inline u128 ipow(u128 base, unsigned e) {
    u128 r = 1;
    for (unsigned i = 0; i < e; i++) r *= base;
    return r;
}

// Emits one gate's register program. Registers come from a free list (lowest first; freed registers are reused last in,
// first out); release() returns all of them (between independent constraints).
struct GateAsm {
    std::vector<GlGateInstr> instrs;
    ImmediatePool *pool;
    std::vector<int> free_list;
    AccBound acc_bound[MAX_ACCS];

    explicit GateAsm(ImmediatePool *p = nullptr) : pool(p) { release(); }
    void release() {
        free_list.clear();
        for (int r = (int)MAX_REGS - 1; r >= 0; r--) free_list.push_back(r);
    }
    int reg() {
        if (free_list.empty()) throw std::runtime_error("gate program needs more than 64 live registers");
        const int r = free_list.back();
        free_list.pop_back();
        return r;
    }
    void free1(int r) {
        if (std::find(free_list.begin(), free_list.end(), r) != free_list.end()) throw std::runtime_error("register freed twice");
        free_list.push_back(r);
    }
    void free(std::initializer_list<int> regs) {
        for (int r : regs) free1(r);
    }
    // operands are 16-bit fields of the instruction word: an index that does not fit is an error, never a wrapped "valid" program
    static uint16_t field(long v) {
        if (v < 0 || v > 0xFFFF) throw std::runtime_error("gate program operand (wire, constant, immediate or register index) does not fit 16 bits");
        return (uint16_t)v;
    }
    int op(uint16_t code, int a, int b = 0, int dst = -1) {
        const int r = dst < 0 ? reg() : dst;
        instrs.push_back(GlGateInstr{code, field(r), field(a), field(b)});
        return r;
    }
    int wire(int i) { return op(LOAD_WIRE, i); }
    int constant(int i) { return op(LOAD_CONST, i); }
    int pi(int i) { return op(LOAD_PI, i); }
    ImmediatePool &need_pool() {
        if (!pool) throw std::runtime_error("this gate needs an ImmediatePool");
        return *pool;
    }
    int imm(u128 value) { return op(LOAD_IMM, (int)need_pool().index(value)); }
    int add(int a, int b, int dst = -1) { return op(ADD, a, b, dst); }
    int sub(int a, int b, int dst = -1) { return op(SUB, a, b, dst); }
    int mul(int a, int b, int dst = -1) { return op(MUL, a, b, dst); }
    int mulk(int a, int shift, int dst = -1) { return op(MULK, a, shift, dst); }
    void emit(int a) { instrs.push_back(GlGateInstr{EMIT, 0, field(a), 0}); }

    // may r * weight still be added to accumulator q without either half being able to reach 2^63?
    bool acc_fits(u128 weight, int q = 0) const { return acc_bound[q].fits(weight); }
    // acc[q] += r[a] * weight, without a modular step (ACC): weight < 2^32, bound checked here
    void acc(int a, u128 weight = 1, int q = 0) {
        ImmediatePool &pl = need_pool();
        if (!acc_bound[q].add(weight)) throw std::runtime_error("accumulator could overflow: reduce (accr) earlier");
        instrs.push_back(GlGateInstr{ACC, field(q), field(a), field((long)pl.index(weight))});
    }
    // register <- acc[q] mod p; acc[q] <- 0 (ACCR)
    int accr(int q = 0, int dst = -1) {
        acc_bound[q].reset();
        return op(ACCR, q, 0, dst);
    }
    // sum_i r[reg_i] * weight_i through accumulator q; reduces in between only if the static bound demands it
    int weighted_sum(const std::vector<std::pair<int, uint64_t>> &terms, int q = 0, int dst = -1) {
        bool started = false;
        for (auto &t : terms) {
            if (started && !acc_fits(t.second, q)) {
                const int part = accr(q);
                acc(part, 1, q);
                free1(part);
            }
            acc(t.first, t.second, q);
            started = true;
        }
        if (!started) return op(LOAD_IMM, (int)need_pool().index(0), 0, dst);
        return accr(q, dst);
    }
    // sum terms[i] * base^i (plonk_common.rs:116-128) for an integer base; returns a fresh register. `terms` are registers, or
    // with wires = true wire indices that are loaded for the purpose. Blocks of consecutive terms whose weights stay below 2^32
    // and provably fit one accumulation, joined by Horner steps with base^(block length).
    int reduce_with_powers(const std::vector<int> &terms, uint64_t base, bool wires = false, int q = 0) {
        if (terms.empty()) return imm(0);
        std::vector<std::pair<int, unsigned>> blocks;
        size_t i = 0;
        while (i < terms.size()) {
            unsigned j = 0;
            u128 bound = 0;
            while (i + j < terms.size() && ipow(base, j) < ((u128)1 << 32) && bound + ipow(base, j) * 0xFFFFFFFFull < ACC_LIMIT) {
                bound += ipow(base, j) * 0xFFFFFFFFull;
                j++;
            }
            for (unsigned k = 0; k < j; k++) {
                const int t = wires ? wire(terms[i + k]) : terms[i + k];
                acc(t, ipow(base, k), q);
                if (wires) free1(t);
            }
            blocks.push_back({accr(q), j});
            i += j;
        }
        const int accu = blocks.back().first;
        for (size_t b = blocks.size() - 1; b-- > 0;) {
            const u128 step = ipow(base, blocks[b].second);
            unsigned bits = 0;
            while (((u128)1 << bits) < step) bits++;
            if ((step & (step - 1)) == 0 && bits < 64) {
                mulk(accu, (int)bits, accu);
            } else {
                const int m = imm(step % P);
                mul(accu, m, accu);
                free1(m);
            }
            add(accu, blocks[b].first, accu);
            free1(blocks[b].first);
        }
        return accu;
    }
    // prod_{k < len(small)} (x - k); small[k] = register holding the constant k. For four factors y (y + 2) with y = x (x - 3).
    int range_product(int x, const std::vector<int> &small) {
        if (small.size() == 4) {
            const int t = sub(x, small[3]);
            const int y = mul(x, t);
            add(y, small[2], t);
            mul(y, t, y);
            free1(t);
            return y;
        }
        const int a = sub(x, small[0]);
        for (size_t k = 1; k < small.size(); k++) {
            const int t = sub(x, small[k]);
            mul(a, t, a);
            free1(t);
        }
        return a;
    }
};

typedef std::vector<GlGateInstr> Program;

// A table's STARK program: the gate assembler plus the next row, the three boundary EMITs and what the tables' constraints share
// (plonky2_gpu_amd/stark.py's StarkAsm, call for call).
struct StarkAsm : GateAsm {
    explicit StarkAsm(ImmediatePool *p) : GateAsm(p) {}
    int local(int i) { return op(LOAD_WIRE, i); }
    int next(int i) { return op(LOAD_NEXT, i); }
    void emit_transition(int a) { instrs.push_back(GlGateInstr{EMIT_TRANSITION, 0, field(a), 0}); }
    void emit_first_row(int a) { instrs.push_back(GlGateInstr{EMIT_FIRST_ROW, 0, field(a), 0}); }
    void emit_last_row(int a) { instrs.push_back(GlGateInstr{EMIT_LAST_ROW, 0, field(a), 0}); }
    // xor_gen(x, y) = x + y - 2 x y in a fresh register; x and y stay
    int xor2(int x, int y) {
        const int s = add(x, y);
        const int m = mul(x, y);
        mulk(m, 1, m);
        sub(s, m, s);
        free1(m);
        return s;
    }
    // xor3_gen(x, y, z) = xor_gen(x, xor_gen(y, z))
    int xor3(int x, int y, int z) {
        const int t = xor2(y, z);
        const int u = xor2(x, t);
        free1(t);
        return u;
    }
    // sum_{k < 32} 2^k bit(z0 + k) in two blocks of 16 weights joined by a shift; bit(z) returns a register that is freed here
    template <class Bit>
    int limb(Bit bit, int z0) {
        int halves[2];
        for (int h = 0; h < 2; h++) {
            for (int k = 0; k < 16; k++) {
                const int t = bit(z0 + 16 * h + k);
                acc(t, (u128)1 << k);
                free1(t);
            }
            halves[h] = accr();
        }
        const int lo = halves[0], hi = halves[1];
        mulk(hi, 16, hi);
        add(hi, lo, hi);
        free1(lo);
        return hi;
    }
    // eval_lookups (evm/src/lookup.rs:19-33), as StarkAsm.eval_lookups
    void eval_lookups(int col_permuted_input, int col_permuted_table) {
        const int local_perm_input = local(col_permuted_input);
        const int next_perm_table = next(col_permuted_table);
        const int next_perm_input = next(col_permuted_input);
        const int diff_input_prev = sub(next_perm_input, local_perm_input);
        const int diff_input_table = sub(next_perm_input, next_perm_table);
        emit(mul(diff_input_prev, diff_input_table));
        emit_last_row(diff_input_table);
    }
};

inline GlError emit_error(const std::string &msg) {
    GlError e;
    e.code = -1;
    e.message = strdup(msg.c_str());
    return e;
}

// a table's STARK program as a GlGatePrograms without gate descriptors; num_gate_constraints counts its EMITs of every kind
inline GlError emit_table_program(const std::string &name, Program (*build)(ImmediatePool &), GlGatePrograms *out) {
    if (!out) return emit_error(name + ": null pointer");
    memset(out, 0, sizeof *out);
    try {
        ImmediatePool pool;
        const Program prog = build(pool);
        uint32_t emits = 0;
        for (const GlGateInstr &in : prog) emits += is_emit(in.op);
        out->num_instrs = (uint32_t)prog.size();
        out->num_immediates = (uint32_t)pool.values.size();
        out->num_gate_constraints = emits;
        out->instrs = (GlGateInstr *)malloc(prog.size() * sizeof(GlGateInstr));
        out->immediates = (uint64_t *)malloc(pool.values.size() * sizeof(uint64_t));
        if (!out->instrs || !out->immediates) {
            gl_gate_programs_free(out);
            return emit_error(name + ": out of memory");
        }
        memcpy(out->instrs, prog.data(), prog.size() * sizeof(GlGateInstr));
        memcpy(out->immediates, pool.values.data(), pool.values.size() * sizeof(uint64_t));
    } catch (const std::exception &ex) {
        gl_gate_programs_free(out);
        return emit_error(name + ": " + ex.what());
    }
    GlError ok;
    ok.code = 0;
    ok.message = nullptr;
    return ok;
}

}  // namespace program_asm
}  // namespace plonky2_hip
