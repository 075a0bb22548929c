// ---- the compiled quotient kernels (stark_jit.hip) ----
// Compile a STARK handle's constraints (stark_prove.h), fill the kernel cache from a description alone, split a program (stark_split.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <string>
#include <vector>

#include "jit.h"
#include "stark_prove.h"
#include "stark_split.h"

using namespace plonky2_hip;

extern "C" {

// the sources of every description's units under the cap, flat, with bounds[i] .. bounds[i + 1] those of description i
static std::vector<std::string> stark_unit_sources(const std::vector<const plonky2_hip::StarkJitDesc *> &descs, uint32_t max_unit_instrs, std::vector<size_t> *bounds) {
    std::vector<std::string> sources;
    bounds->assign(1, 0);
    for (const plonky2_hip::StarkJitDesc *h : descs) {
        const std::vector<plonky2_hip::StarkJitUnit> units = plonky2_hip::stark_jit_units(*h, max_unit_instrs);
        for (size_t u = 0; u < units.size(); u++) sources.push_back(plonky2_hip::stark_jit_unit_source(*h, units[u], u == 0, u + 1 == units.size()));
        bounds->push_back(sources.size());
    }
    return sources;
}

// gl_*_units' max_unit_instrs: 0 is the library's default cap
static uint32_t unit_cap(uint32_t max_unit_instrs) { return max_unit_instrs ? max_unit_instrs : plonky2_hip::STARK_JIT_DEFAULT_UNIT_INSTRS; }

static GlError stark_compile_all(const std::vector<Stark *> &tables, uint32_t max_unit_instrs, void *ctx) {
    DeviceCall device_call(ctx);  // the context's device becomes current: the modules are loaded there
    std::vector<Stark *> todo;
    for (Stark *s : tables)
        if (!s->jit) todo.push_back(s);
    if (todo.empty()) return ok();  // a second call is a no-op
    std::vector<const plonky2_hip::StarkJitDesc *> descs;
    for (Stark *s : todo) descs.push_back(&s->host);
    std::vector<size_t> bounds;
    const std::vector<std::string> sources = stark_unit_sources(descs, max_unit_instrs, &bounds);
    std::vector<std::vector<char>> codes;
    std::string err;
    if (!plonky2_hip::stark_jit_compile_sources(sources, &codes, nullptr, &err)) return fail(GL_E_INVALID, err);
    // all or nothing: a handle whose compile failed stays interpreted
    std::vector<plonky2_hip::StarkJitKernel *> kernels;
    for (size_t i = 0; i < todo.size(); i++) {
        plonky2_hip::StarkJitKernel *k = plonky2_hip::stark_jit_load(
            todo[i]->host, std::vector<std::string>(sources.begin() + bounds[i], sources.begin() + bounds[i + 1]),
            std::vector<std::vector<char>>(std::make_move_iterator(codes.begin() + bounds[i]), std::make_move_iterator(codes.begin() + bounds[i + 1])), &err);
        if (!k) {
            for (plonky2_hip::StarkJitKernel *done : kernels) plonky2_hip::stark_jit_destroy(done);
            return fail(GL_E_INVALID, err);
        }
        kernels.push_back(k);
    }
    for (size_t i = 0; i < todo.size(); i++) todo[i]->jit = kernels[i];
    return ok();
}

static GlError stark_precompile_all(const std::vector<plonky2_hip::StarkJitDesc> &descs, uint32_t max_unit_instrs) {
    if (plonky2_hip::jit_cache_dir().empty())
        return fail(GL_E_INVALID, "no kernel cache to compile into: set PLONKY2_HIP_KERNEL_CACHE or create the directory kernel_cache next to the library");
    std::vector<const plonky2_hip::StarkJitDesc *> ptrs;
    for (const plonky2_hip::StarkJitDesc &h : descs) ptrs.push_back(&h);
    std::vector<size_t> bounds;
    const std::vector<std::string> sources = stark_unit_sources(ptrs, max_unit_instrs, &bounds);
    std::vector<std::vector<char>> codes;
    std::string err;
    if (!plonky2_hip::stark_jit_compile_sources(sources, &codes, nullptr, &err)) return fail(GL_E_INVALID, err);
    return ok();
}

GlError gl_stark_compile(void *stark, void *ctx) {
    if (!stark || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all({static_cast<Stark *>(stark)}, plonky2_hip::STARK_JIT_ONE_UNIT, ctx);
}

GlError gl_stark_tables_compile(void *tables, void *ctx) {
    if (!tables || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all(static_cast<StarkTables *>(tables)->tables, plonky2_hip::STARK_JIT_ONE_UNIT, ctx);
}

GlError gl_stark_compile_units(void *stark, uint32_t max_unit_instrs, void *ctx) {
    if (!stark || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all({static_cast<Stark *>(stark)}, unit_cap(max_unit_instrs), ctx);
}

GlError gl_stark_tables_compile_units(void *tables, uint32_t max_unit_instrs, void *ctx) {
    if (!tables || !ctx) return fail(GL_E_INVALID, "null pointer");
    return stark_compile_all(static_cast<StarkTables *>(tables)->tables, unit_cap(max_unit_instrs), ctx);
}

int gl_stark_is_compiled(const void *stark) { return stark && static_cast<const Stark *>(stark)->jit ? 1 : 0; }

int gl_stark_tables_is_compiled(const void *tables) {
    if (!tables) return 0;
    for (const Stark *s : static_cast<const StarkTables *>(tables)->tables)
        if (!s->jit) return 0;
    return 1;
}

int gl_stark_kernel_units(const void *stark) {
    const Stark *s = static_cast<const Stark *>(stark);
    return s && s->jit ? (int)plonky2_hip::stark_jit_kernel_units(s->jit) : 0;
}

int gl_stark_tables_kernel_units(const void *tables, uint32_t table) {
    const StarkTables *T = static_cast<const StarkTables *>(tables);
    if (!T || table >= T->tables.size()) return 0;
    return gl_stark_kernel_units(T->tables[table]);
}

const char *gl_stark_kernel_unit_source(const void *stark, uint32_t unit) {
    const Stark *s = static_cast<const Stark *>(stark);
    return s && s->jit ? plonky2_hip::stark_jit_kernel_source(s->jit, unit) : nullptr;
}

const char *gl_stark_tables_kernel_unit_source(const void *tables, uint32_t table, uint32_t unit) {
    const StarkTables *T = static_cast<const StarkTables *>(tables);
    if (!T || table >= T->tables.size()) return nullptr;
    return gl_stark_kernel_unit_source(T->tables[table], unit);
}

const char *gl_stark_kernel_source(const void *stark) { return gl_stark_kernel_unit_source(stark, 0); }

const char *gl_stark_tables_kernel_source(const void *tables, uint32_t table) { return gl_stark_tables_kernel_unit_source(tables, table, 0); }

static GlError stark_precompile_one(uint32_t hasher, const GlStarkDesc *d, uint32_t max_unit_instrs) {
    if (!d) return fail(GL_E_INVALID, "null pointer");
    TRY(stark_check(hasher, d, 0));
    return stark_precompile_all({stark_host_desc(d)}, max_unit_instrs);
}

static GlError stark_precompile_tables(uint32_t hasher, const GlStarkTablesDesc *d, uint32_t max_unit_instrs) {
    if (!d) return fail(GL_E_INVALID, "null pointer");
    std::vector<std::vector<uint32_t>> zs;
    TRY(stark_tables_check(hasher, d, &zs));
    std::vector<plonky2_hip::StarkJitDesc> descs;
    for (uint32_t k = 0; k < d->num_tables; k++) {
        descs.push_back(stark_host_desc(&d->tables[k]));
        stark_host_ctl(&descs.back(), d, zs[k]);
    }
    return stark_precompile_all(descs, max_unit_instrs);
}

GlError gl_stark_precompile(uint32_t hasher, const GlStarkDesc *d) { return stark_precompile_one(hasher, d, plonky2_hip::STARK_JIT_ONE_UNIT); }

GlError gl_stark_tables_precompile(uint32_t hasher, const GlStarkTablesDesc *d) { return stark_precompile_tables(hasher, d, plonky2_hip::STARK_JIT_ONE_UNIT); }

GlError gl_stark_precompile_units(uint32_t hasher, const GlStarkDesc *d, uint32_t max_unit_instrs) {
    return stark_precompile_one(hasher, d, unit_cap(max_unit_instrs));
}

GlError gl_stark_tables_precompile_units(uint32_t hasher, const GlStarkTablesDesc *d, uint32_t max_unit_instrs) {
    return stark_precompile_tables(hasher, d, unit_cap(max_unit_instrs));
}

// the device-free splitter (stark_split.hip) behind the checks gl_stark_create makes of the program
GlError gl_stark_split_program(const GlStarkDesc *d, uint32_t max_unit_instrs, GlGatePrograms *out) {
    if (!d || !out || !d->h_instrs || (d->num_immediates && !d->h_immediates)) return fail(GL_E_INVALID, "null pointer");
    memset(out, 0, sizeof *out);
    if (d->struct_size != sizeof(GlStarkDesc)) return struct_size_error("GlStarkDesc");
    const uint16_t *instrs = reinterpret_cast<const uint16_t *>(d->h_instrs);
    std::string verr;
    if (!plonky2_hip::stark_program_validate(instrs, d->num_instrs, d->h_immediates, d->num_immediates, d->num_columns, d->num_public_inputs, &verr))
        return fail(GL_E_INVALID, verr);
    const std::vector<plonky2_hip::StarkProgramUnit> units = plonky2_hip::stark_program_split(instrs, d->num_instrs, unit_cap(max_unit_instrs));
    size_t words = 0;
    for (const plonky2_hip::StarkProgramUnit &u : units) words += u.instrs.size();
    out->instrs = (GlGateInstr *)malloc(std::max<size_t>(1, words) * sizeof(uint16_t));
    out->gates = (GlGateDesc *)malloc(units.size() * sizeof(GlGateDesc));
    out->immediates = (uint64_t *)malloc(std::max<size_t>(1, d->num_immediates) * sizeof(uint64_t));
    if (!out->instrs || !out->gates || !out->immediates) {
        gl_gate_programs_free(out);
        return fail(GL_E_INVALID, "gl_stark_split_program: out of memory");
    }
    uint32_t at = 0;
    for (size_t k = 0; k < units.size(); k++) {
        const uint32_t len = (uint32_t)(units[k].instrs.size() / 4);
        memcpy(out->instrs + at, units[k].instrs.data(), units[k].instrs.size() * sizeof(uint16_t));
        out->gates[k] = GlGateDesc{(uint32_t)k, 0, units[k].emit_start, units[k].emit_end, at, len};
        at += len;
    }
    if (d->num_immediates) memcpy(out->immediates, d->h_immediates, d->num_immediates * sizeof(uint64_t));
    out->num_instrs = at, out->num_gates = (uint32_t)units.size(), out->num_immediates = d->num_immediates;
    out->num_gate_constraints = units.back().emit_end;
    return ok();
}

}  // extern "C"
