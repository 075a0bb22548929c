// stark_jit.hip — a STARK's constraint quotient as a RUN-TIME COMPILED kernel specialised to the STARK.
//
// stark_quotient_values_kernel (stark.hip) INTERPRETS the STARK's register program per LDE point: 64 registers in scratch memory
// (two scratch loads and a scratch store per ADD), an instruction fetch and a switch per operation, immediates and ACC weights read
// from memory, the permutation and CTL descriptors walked through pointers although they were fixed when the handle was created.
// Here the description becomes straight-line HIP source for ONE kernel that replaces the interpreter in full for that STARK — same
// inputs, same output layout, one launch per quotient:
//   * the program: registers are local variables, immediates and MULK factors literals, ACC weights scalar literals (sj::acc, the
//     gj_acc form of gate_jit.hip), LOAD_WIRE / LOAD_NEXT read local[a * stride] / next[a * stride] with stride a kernel argument,
//     LOAD_PI the device array of public inputs, the four EMITs feed starky's consumer in emission order;
//   * eval_permutation_checks: the batches, their instances and the column indices of their pairs as literals, the (beta, gamma)
//     sets kernel arguments;
//   * eval_cross_table_lookup_checks of a table: every CTL Z with its TWC's columns — terms, coefficients, constants — as
//     literals, its filter or its absence decided here, the challenges kernel arguments.
// Head and tail are the interpreter's (stark_jit_device.h, in the source once). The values are the interpreter's bit for bit:
// every operation computes the same field element and the store is canonical.
//
// Everything that varies per proof is a kernel argument BY VALUE (StarkJitArgs): no __constant__ table is written in front of a
// launch, so one compiled handle is used by several host threads on several contexts at once without taking turns.
//
// UNITS (stark_jit_units): hiprtc's instruction selection is superlinear in the length of one basic block, so a long description is
// cut into several kernels the way gate_jit.hip cuts a circuit's gates. The program is cut by stark_program_split (stark_split.h),
// the permutation and CTL checks behind it by the field operations they generate. Unit 0 starts the consumer's sums at 0, every
// later unit loads them from p.out[c * size + q.i], every unit but the last stores them there raw, only the last runs sj::tail;
// the units run in order on the call's stream and a thread reads and writes only its own elements. That is the same Horner chain
// over the same operands — a 64-bit word stored and loaded is the same word — so the stored quotient is the interpreter's bit for
// bit by the argument for one kernel; there is no new one. Every unit calls sj::head in full: what a unit does not read of the
// Point (the inversion and root_pow in a unit of plain EMITs, zh_inv in every unit but the last) is dead code to the compiler,
// and the text in front of the generated body stays the single kernel's.
//
// Occupancy: __launch_bounds__(128) as the interpreter, and no waves-per-SIMD attribute — the program's live values decide the
// registers (at most 64 program registers = 128 VGPRs plus the running sums and what the scheduler hoists), the compiler may take
// up to 512 and never spills into scratch; a fixed occupancy would trade that for spills on the programs that need the registers.
#include "stark_jit.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <map>
#include <mutex>
#include <sstream>
#include <thread>

#include "gl_field.h"
#include "jit.h"
#include "program_isa.h"
#include "stark_jit_device.h"
#include "stark_split.h"

namespace plonky2_hip {

namespace {

const char *const POINT_DEVICE_SRC =
#include "build/point_device_src.inc"
    ;
const char *const SJ_DEVICE_SRC =
#include "build/stark_jit_device_src.inc"
    ;

using isa::MAX_REGS;
const char *const KERNEL_NAME = "stark_quotient_kernel";

std::string lit(uint64_t v) {
    char b[32];
    snprintf(b, sizeof b, "0x%llxull", (unsigned long long)v);
    return b;
}

// the program (validated by stark_program_validate) as statements
void generate_program(std::ostringstream &o, const StarkJitDesc &d, const std::vector<uint16_t> &instrs) {
    const size_t n = instrs.size() / 4;
    bool reg_used[MAX_REGS] = {}, acc_used[isa::MAX_ACCS] = {};
    for (size_t pc = 0; pc < n; pc++) {
        const isa::Instr in = isa::instr_at(instrs.data(), pc);
        if (isa::acc_in_dst(in.op))
            acc_used[in.dst & (isa::MAX_ACCS - 1)] = true;
        else if (isa::writes_reg(in.op))
            reg_used[in.dst & (MAX_REGS - 1)] = true;
    }
    for (uint32_t r = 0; r < MAX_REGS; r++)
        if (reg_used[r]) o << "  uint64_t r" << r << ";\n";
    for (uint32_t q = 0; q < isa::MAX_ACCS; q++)
        if (acc_used[q]) o << "  uint64_t a" << q << "l = 0, a" << q << "h = 0;\n";
    for (size_t pc = 0; pc < n; pc++) {
        const isa::Instr in = isa::instr_at(instrs.data(), pc);
        const uint16_t op = in.op, dst = in.dst & (MAX_REGS - 1), a = in.a, b = in.b;
        const uint32_t ra = a & (MAX_REGS - 1), rb = b & (MAX_REGS - 1);
        switch (op) {
            case isa::LOAD_WIRE: o << "  r" << dst << " = q.local[" << a << " * p.stride];\n"; break;
            case isa::LOAD_NEXT: o << "  r" << dst << " = q.next[" << a << " * p.stride];\n"; break;
            case isa::LOAD_PI: o << "  r" << dst << " = p.pis[" << a << "];\n"; break;
            case isa::LOAD_IMM: o << "  r" << dst << " = " << lit(d.imms[a]) << ";\n"; break;
            case isa::ADD: o << "  r" << dst << " = gl::add(r" << ra << ", r" << rb << ");\n"; break;
            case isa::SUB: o << "  r" << dst << " = gl::sub(r" << ra << ", r" << rb << ");\n"; break;
            case isa::MUL: o << "  r" << dst << " = gl::mul(r" << ra << ", r" << rb << ");\n"; break;
            case isa::MULK: o << "  r" << dst << " = gl::mul(r" << ra << ", " << lit(1ull << (b & 63)) << ");\n"; break;
            case isa::ACC: o << "  sj::acc(a" << (dst & 3) << "l, a" << (dst & 3) << "h, r" << ra << ", " << d.imms[b] << "u);\n"; break;
            case isa::ACCR:
                o << "  r" << dst << " = gl::fold96(a" << (a & 3) << "l, a" << (a & 3) << "h); a" << (a & 3) << "l = 0; a" << (a & 3) << "h = 0;\n";
                break;
            case isa::EMIT: o << "  sj::constraint(sums, p, r" << ra << ");\n"; break;
            case isa::EMIT_TRANSITION: o << "  sj::constraint(sums, p, gl::mul(r" << ra << ", q.z_last));\n"; break;
            case isa::EMIT_FIRST_ROW: o << "  sj::constraint(sums, p, gl::mul(r" << ra << ", q.l_first));\n"; break;
            case isa::EMIT_LAST_ROW: o << "  sj::constraint(sums, p, gl::mul(r" << ra << ", q.l_last));\n"; break;
            default: break;  // refused by stark_program_validate
        }
    }
}

// eval_permutation_checks (permutation.rs:284-322): Z(1) = 1 for every Z, then per batch Z(g x) prod rhs = Z(x) prod lhs; batch
// z holds the instances f = z * qdf + k, instance f = (pair f / num_challenges, challenge f % num_challenges) under SET k
void generate_permutation_first_rows(std::ostringstream &o, uint32_t z0, uint32_t z1) {
    for (uint32_t z = z0; z < z1; z++)
        o << "  sj::constraint(sums, p, gl::mul(gl::sub(p.zs[" << z << " * p.stride + q.t], 1), q.l_first));\n";
}

void generate_permutation_batches(std::ostringstream &o, const StarkJitDesc &d, uint32_t z0, uint32_t z1) {
    const uint32_t nch = d.num_challenges, instances = d.num_pairs() * nch;
    for (uint32_t z = z0; z < z1; z++) {
        o << "  {\n    uint64_t lhs = 1, rhs = 1;\n";
        for (uint32_t k = 0; k < d.qdf; k++) {
            const uint32_t f = z * d.qdf + k;
            if (f >= instances) break;  // the last batch may be short
            const uint32_t pair = f / nch, c = f % nch, slot = k * nch + c;
            o << "    {\n      const uint64_t beta = p.perm_beta[" << slot << "], gamma = p.perm_gamma[" << slot << "];\n      uint64_t l = 0, r = 0;\n";
            for (uint32_t j = d.pair_bounds[pair + 1]; j-- > d.pair_bounds[pair];) {  // Horner from the last column pair
                o << "      l = gl::mac(q.local[" << d.column_pairs[2 * j] << " * p.stride], l, beta);\n";
                o << "      r = gl::mac(q.local[" << d.column_pairs[2 * j + 1] << " * p.stride], r, beta);\n";
            }
            o << "      lhs = gl::mul(lhs, gl::add(l, gamma));\n      rhs = gl::mul(rhs, gl::add(r, gamma));\n    }\n";
        }
        o << "    sj::constraint(sums, p, gl::sub(gl::mul(p.zs[" << z << " * p.stride + q.t_next], rhs), gl::mul(p.zs[" << z
          << " * p.stride + q.t], lhs)));\n  }\n";
    }
}

uint32_t num_permutation_zs(const StarkJitDesc &d) { return d.num_pairs() ? stark_num_zs(d.num_pairs(), d.num_challenges, d.qdf) : 0; }

// Column::eval (cross_table_lookup.rs:100-119) of CTL column k at `row` as an expression statement into `name`
void generate_ctl_column(std::ostringstream &o, const StarkJitDesc &d, const std::string &name, uint32_t k, const char *row) {
    o << "      uint64_t " << name << " = " << lit(d.column_constants[k]) << ";\n";
    for (uint32_t j = d.column_bounds[k]; j < d.column_bounds[k + 1]; j++)
        o << "      " << name << " = gl::mac(" << name << ", " << row << "[" << d.term_columns[j] << " * p.stride], " << lit(d.term_coeffs[j]) << ");\n";
}

// eval_cross_table_lookup_checks (evm/src/cross_table_lookup.rs:421-450), the CTL Zs behind the permutation Zs: with
// select(f, x) = f x + 1 - f, Z(1) = select(filter, combine) on the first row and Z(g x) = Z(x) select(filter', combine') on every
// row but the last
void generate_ctl_checks(std::ostringstream &o, const StarkJitDesc &d, uint32_t z0, uint32_t z1) {
    const uint32_t num_perm_zs = num_permutation_zs(d);
    for (uint32_t z = z0; z < z1; z++) {
        const uint32_t tw = d.ctl_zs[2 * z], c = d.ctl_zs[2 * z + 1], filter = d.twc_filter[tw];
        o << "  {\n    const uint64_t beta = p.ctl_beta[" << c << "], gamma = p.ctl_gamma[" << c << "];\n    uint64_t sel[2];\n";
        for (int side = 0; side < 2; side++) {
            const char *row = side ? "q.next" : "q.local";
            o << "    {\n      uint64_t acc = 0;\n";
            // GrandProductChallenge::combine (evm/src/permutation.rs:61-73): gamma + sum_j beta^j column_j, Horner from the last column
            for (uint32_t k = d.twc_column_bounds[tw + 1]; k-- > d.twc_column_bounds[tw];) {
                const std::string name = "c" + std::to_string(k);
                generate_ctl_column(o, d, name, k, row);
                o << "      acc = gl::add(gl::mul(acc, beta), " << name << ");\n";
            }
            o << "      acc = gl::add(acc, gamma);\n";
            if (filter != STARK_CTL_NO_FILTER) {
                generate_ctl_column(o, d, "f", filter, row);
                o << "      acc = gl::sub(gl::mac(1, f, acc), f);\n";
            }
            o << "      sel[" << side << "] = acc;\n    }\n";
        }
        const uint32_t slot = num_perm_zs + z;
        o << "    const uint64_t z_local = p.zs[" << slot << " * p.stride + q.t], z_next = p.zs[" << slot << " * p.stride + q.t_next];\n"
          << "    sj::constraint(sums, p, gl::mul(gl::sub(z_local, sel[0]), q.l_first));\n"
          << "    sj::constraint(sums, p, gl::mul(gl::sub(z_next, gl::mul(z_local, sel[1])), q.z_last));\n  }\n";
    }
}

// The checks behind the program in the consumer's order, as items that a cut may fall between: the permutation Zs' first-row
// checks, their batch checks, then the CTL Zs — one CTL Z's pair of constraints is one item.
uint32_t num_check_items(const StarkJitDesc &d) { return 2 * num_permutation_zs(d) + (uint32_t)d.ctl_zs.size() / 2; }

void generate_checks(std::ostringstream &o, const StarkJitDesc &d, uint32_t i0, uint32_t i1) {
    const uint32_t nz = num_permutation_zs(d);
    auto clip = [&](uint32_t base, uint32_t i) { return std::min(std::max(i, base), num_check_items(d)) - base; };
    generate_permutation_first_rows(o, clip(0, i0), std::min(clip(0, i1), nz));
    generate_permutation_batches(o, d, std::min(clip(nz, i0), nz), std::min(clip(nz, i1), nz));
    generate_ctl_checks(o, d, clip(2 * nz, i0), clip(2 * nz, i1));
}

// what an item costs against the cap: the field operations and consumer calls of its generated text, the unit in which an
// instruction of the program costs one
uint32_t check_item_cost(const StarkJitDesc &d, uint32_t i) {
    std::ostringstream o;
    generate_checks(o, d, i, i + 1);
    const std::string text = o.str();
    uint32_t cost = 0;
    for (size_t at = 0; (at = text.find("::", at)) != std::string::npos; at += 2) cost++;
    return cost;
}

}  // namespace

std::vector<StarkJitUnit> stark_jit_units(const StarkJitDesc &d, uint32_t max_unit_instrs) {
    std::vector<StarkJitUnit> units;
    const uint32_t items = num_check_items(d);
    if (max_unit_instrs == STARK_JIT_ONE_UNIT) {
        units.push_back(StarkJitUnit{d.instrs, 0, items});
        return units;
    }
    for (StarkProgramUnit &u : stark_program_split(d.instrs.data(), (uint32_t)(d.instrs.size() / 4), max_unit_instrs))
        units.push_back(StarkJitUnit{std::move(u.instrs), 0, 0});
    // the checks go into the last program unit while they fit and into further units otherwise; an item above the cap is a unit
    uint64_t used = units.back().instrs.size() / 4;
    for (uint32_t i = 0; i < items; i++) {
        const uint32_t cost = check_item_cost(d, i);
        const bool empty = units.back().instrs.empty() && units.back().check_start == units.back().check_end;
        if (used + cost > max_unit_instrs && !empty) {
            units.push_back(StarkJitUnit{{}, i, i});
            used = 0;
        }
        if (units.back().check_start == units.back().check_end) units.back().check_start = i;
        units.back().check_end = i + 1;
        used += cost;
    }
    return units;
}

std::string stark_jit_unit_source(const StarkJitDesc &d, const StarkJitUnit &u, bool first, bool last) {
    std::ostringstream o;
    o << "#define GL_JIT 1\n" << jit_field_source() << "\n" << POINT_DEVICE_SRC << "\n" << SJ_DEVICE_SRC << "\n";
    o << "#define NCH " << d.num_challenges << "\n#define QDB " << glh::log2_ceil(d.qdf) << "\n";
    o << "extern \"C\" __global__ __launch_bounds__(128) void " << KERNEL_NAME << "(const StarkJitArgs p) {\n"
         "  sj::Point q;\n  if (!sj::head<QDB>(p, q)) return;\n  uint64_t sums[NCH];\n";
    // the running sums between units live in the call's own out, raw, at the elements the tail will store to
    o << (first ? "  for (int c = 0; c < NCH; c++) sums[c] = 0;\n" : "  for (int c = 0; c < NCH; c++) sums[c] = p.out[(uint64_t)c * q.size + q.i];\n");
    generate_program(o, d, u.instrs);
    generate_checks(o, d, u.check_start, u.check_end);
    o << (last ? "  sj::tail(sums, p, q);\n}\n" : "  for (int c = 0; c < NCH; c++) p.out[(uint64_t)c * q.size + q.i] = sums[c];\n}\n");
    return o.str();
}

std::string stark_jit_source(const StarkJitDesc &d) { return stark_jit_unit_source(d, stark_jit_units(d, STARK_JIT_ONE_UNIT)[0], true, true); }

bool stark_jit_compile_sources(const std::vector<std::string> &sources, std::vector<std::vector<char>> *codes, uint32_t *written, std::string *error) {
    const std::string dir = jit_cache_dir();
    std::map<std::string, size_t> first;  // source -> the first index that has it
    std::vector<size_t> distinct;
    for (size_t i = 0; i < sources.size(); i++)
        if (first.emplace(sources[i], i).second) distinct.push_back(i);
    codes->assign(sources.size(), {});
    std::vector<std::string> paths(sources.size());
    std::vector<std::string> listed;
    for (size_t i : distinct) listed.push_back(paths[i] = jit_cache_path(dir, sources[i], "stark_"));
    jit_cache_list(listed);
    std::vector<size_t> missing;
    for (size_t i : distinct)
        if (!jit_cache_read(paths[i], &(*codes)[i])) missing.push_back(i);
    if (written) *written = (uint32_t)missing.size();
    std::vector<std::string> errors(sources.size());
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t j; (j = next.fetch_add(1)) < missing.size();) {
            const size_t i = missing[j];
            if (!jit_compile(sources[i], "stark_quotient.hip", paths[i], &(*codes)[i], &errors[i])) (*codes)[i].clear();
        }
    };
    const size_t threads = std::min<size_t>(8, missing.size());
    std::vector<std::thread> pool;
    for (size_t t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
    for (size_t i : missing)
        if ((*codes)[i].empty()) {
            *error = "compiling the STARK quotient kernel: " + errors[i];
            return false;
        }
    for (size_t i = 0; i < sources.size(); i++)
        if ((*codes)[i].empty()) (*codes)[i] = (*codes)[first[sources[i]]];
    return true;
}

struct StarkJitKernel {
    std::vector<std::string> sources;      // per unit, in launch order
    std::vector<std::vector<char>> codes;
    uint32_t num_challenges = 0, qdf = 0, num_pairs = 0, num_ctl_zs = 0;
    // a module per unit per device the handle has launched on
    struct Loaded {
        std::vector<hipModule_t> modules;
        std::vector<hipFunction_t> fns;
    };
    std::mutex mu;
    std::map<int, Loaded> loaded;
    hipError_t functions(const std::vector<hipFunction_t> **fns) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        auto it = loaded.find(dev);
        if (it == loaded.end()) {
            Loaded l;
            for (const std::vector<char> &code : codes) {
                hipModule_t module = nullptr;
                hipFunction_t fn = nullptr;
                e = hipModuleLoadData(&module, code.data());
                if (module) l.modules.push_back(module);
                if (e == hipSuccess) e = hipModuleGetFunction(&fn, module, KERNEL_NAME);
                if (e != hipSuccess) {  // all units or none
                    for (hipModule_t m : l.modules) (void)hipModuleUnload(m);
                    return e;
                }
                l.fns.push_back(fn);
            }
            it = loaded.emplace(dev, std::move(l)).first;
        }
        *fns = &it->second.fns;  // the map's nodes stay where they are
        return hipSuccess;
    }
};

StarkJitKernel *stark_jit_load(const StarkJitDesc &d, const std::vector<std::string> &sources, std::vector<std::vector<char>> &&codes, std::string *error) {
    for (size_t u = 0; u < codes.size(); u++)
        if (!code_object_whole(codes[u])) {
            const std::string path = jit_cache_path(jit_cache_dir(), sources[u], "stark_");
            *error = "loading the compiled STARK quotient kernel: the code object is no whole ELF file" +
                     (path.empty() ? std::string() : " (a damaged cache entry? " + path + ".hsaco)");
            return nullptr;
        }
    StarkJitKernel *k = new StarkJitKernel();
    k->sources = sources, k->codes = std::move(codes);
    k->num_challenges = d.num_challenges, k->qdf = d.qdf, k->num_pairs = d.num_pairs(), k->num_ctl_zs = (uint32_t)d.ctl_zs.size() / 2;
    const std::vector<hipFunction_t> *fns;
    if (hipError_t e = k->functions(&fns); e != hipSuccess) {
        (void)hipGetLastError();
        *error = std::string("loading the compiled STARK quotient kernel: ") + hipGetErrorString(e);
        delete k;
        return nullptr;
    }
    return k;
}

void stark_jit_destroy(StarkJitKernel *k) {
    if (!k) return;
    for (auto &kv : k->loaded)
        for (hipModule_t m : kv.second.modules) (void)hipModuleUnload(m);
    delete k;
}

uint32_t stark_jit_kernel_units(const StarkJitKernel *k) { return (uint32_t)k->sources.size(); }

const char *stark_jit_kernel_source(const StarkJitKernel *k, uint32_t unit) { return unit < k->sources.size() ? k->sources[unit].c_str() : nullptr; }

hipError_t stark_jit_launch(const StarkJitKernel *kc, const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, hipStream_t stream) {
    StarkJitKernel *k = const_cast<StarkJitKernel *>(kc);  // the modules per device are the object's own
    if (a.degree_bits == 0 || a.num_challenges != k->num_challenges || a.qdf != k->qdf || a.pairs.num_pairs != k->num_pairs || a.ctl.num_zs != k->num_ctl_zs)
        return hipErrorInvalidValue;
    StarkJitArgs p;
    uint32_t qdb = 0;
    if (hipError_t e = stark_point_args(tb, a, out, &p, &qdb); e != hipSuccess) return e;
    const std::vector<hipFunction_t> *fns;
    if (hipError_t e = k->functions(&fns); e != hipSuccess) return e;
    const uint64_t size = 1ull << (a.degree_bits + qdb);
    void *args[] = {&p};
    // the units in order on one stream: unit k + 1 reads the sums unit k stored, each thread its own
    for (hipFunction_t fn : *fns)
        if (hipError_t e = hipModuleLaunchKernel(fn, (unsigned)((size + 127) / 128), 1, 1, 128, 1, 1, 0, stream, args, nullptr); e != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace plonky2_hip
