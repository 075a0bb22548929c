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
void generate_program(std::ostringstream &o, const StarkJitDesc &d) {
    const size_t n = d.instrs.size() / 4;
    bool reg_used[MAX_REGS] = {}, acc_used[isa::MAX_ACCS] = {};
    for (size_t pc = 0; pc < n; pc++) {
        const isa::Instr in = isa::instr_at(d.instrs.data(), pc);
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
        const isa::Instr in = isa::instr_at(d.instrs.data(), pc);
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
uint32_t generate_permutation_checks(std::ostringstream &o, const StarkJitDesc &d) {
    const uint32_t np = d.num_pairs(), nch = d.num_challenges;
    if (!np) return 0;
    const uint32_t instances = np * nch, num_zs = stark_num_zs(np, nch, d.qdf);
    for (uint32_t z = 0; z < num_zs; z++)
        o << "  sj::constraint(sums, p, gl::mul(gl::sub(p.zs[" << z << " * p.stride + q.t], 1), q.l_first));\n";
    for (uint32_t z = 0; z < num_zs; z++) {
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
    return num_zs;
}

// Column::eval (cross_table_lookup.rs:100-119) of CTL column k at `row` as an expression statement into `name`
void generate_ctl_column(std::ostringstream &o, const StarkJitDesc &d, const std::string &name, uint32_t k, const char *row) {
    o << "      uint64_t " << name << " = " << lit(d.column_constants[k]) << ";\n";
    for (uint32_t j = d.column_bounds[k]; j < d.column_bounds[k + 1]; j++)
        o << "      " << name << " = gl::mac(" << name << ", " << row << "[" << d.term_columns[j] << " * p.stride], " << lit(d.term_coeffs[j]) << ");\n";
}

// eval_cross_table_lookup_checks (evm/src/cross_table_lookup.rs:421-450), the CTL Zs behind the permutation Zs: with
// select(f, x) = f x + 1 - f, Z(1) = select(filter, combine) on the first row and Z(g x) = Z(x) select(filter', combine') on every
// row but the last
void generate_ctl_checks(std::ostringstream &o, const StarkJitDesc &d, uint32_t num_perm_zs) {
    for (uint32_t z = 0; z < d.ctl_zs.size() / 2; z++) {
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

}  // namespace

std::string stark_jit_source(const StarkJitDesc &d) {
    std::ostringstream o;
    o << "#define GL_JIT 1\n" << jit_field_source() << "\n" << POINT_DEVICE_SRC << "\n" << SJ_DEVICE_SRC << "\n";
    o << "#define NCH " << d.num_challenges << "\n#define QDB " << glh::log2_ceil(d.qdf) << "\n";
    o << "extern \"C\" __global__ __launch_bounds__(128) void " << KERNEL_NAME << "(const StarkJitArgs p) {\n"
         "  sj::Point q;\n  if (!sj::head<QDB>(p, q)) return;\n  uint64_t sums[NCH];\n  for (int c = 0; c < NCH; c++) sums[c] = 0;\n";
    generate_program(o, d);
    const uint32_t num_perm_zs = generate_permutation_checks(o, d);
    generate_ctl_checks(o, d, num_perm_zs);
    o << "  sj::tail(sums, p, q);\n}\n";
    return o.str();
}

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
    std::string source;
    std::vector<char> code;
    uint32_t num_challenges = 0, qdf = 0, num_pairs = 0, num_ctl_zs = 0;
    // a module per device the handle has launched on
    struct Loaded {
        hipModule_t module;
        hipFunction_t fn;
    };
    std::mutex mu;
    std::map<int, Loaded> loaded;
    hipError_t function(hipFunction_t *fn) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        auto it = loaded.find(dev);
        if (it == loaded.end()) {
            Loaded l{nullptr, nullptr};
            e = hipModuleLoadData(&l.module, code.data());
            if (e == hipSuccess) e = hipModuleGetFunction(&l.fn, l.module, KERNEL_NAME);
            if (e != hipSuccess) {
                if (l.module) (void)hipModuleUnload(l.module);
                return e;
            }
            it = loaded.emplace(dev, l).first;
        }
        *fn = it->second.fn;
        return hipSuccess;
    }
};

StarkJitKernel *stark_jit_load(const StarkJitDesc &d, const std::string &source, std::vector<char> &&code, std::string *error) {
    if (!code_object_whole(code)) {
        const std::string path = jit_cache_path(jit_cache_dir(), source, "stark_");
        *error = "loading the compiled STARK quotient kernel: the code object is no whole ELF file" +
                 (path.empty() ? std::string() : " (a damaged cache entry? " + path + ".hsaco)");
        return nullptr;
    }
    StarkJitKernel *k = new StarkJitKernel();
    k->source = source, k->code = std::move(code);
    k->num_challenges = d.num_challenges, k->qdf = d.qdf, k->num_pairs = d.num_pairs(), k->num_ctl_zs = (uint32_t)d.ctl_zs.size() / 2;
    hipFunction_t fn;
    if (hipError_t e = k->function(&fn); e != hipSuccess) {
        (void)hipGetLastError();
        *error = std::string("loading the compiled STARK quotient kernel: ") + hipGetErrorString(e);
        delete k;
        return nullptr;
    }
    return k;
}

void stark_jit_destroy(StarkJitKernel *k) {
    if (!k) return;
    for (auto &kv : k->loaded) (void)hipModuleUnload(kv.second.module);
    delete k;
}

const char *stark_jit_kernel_source(const StarkJitKernel *k) { return k->source.c_str(); }

hipError_t stark_jit_launch(const StarkJitKernel *kc, const NttTables &tb, const StarkQuotientArgs &a, uint64_t *out, hipStream_t stream) {
    StarkJitKernel *k = const_cast<StarkJitKernel *>(kc);  // the modules per device are the object's own
    if (a.degree_bits == 0 || a.num_challenges != k->num_challenges || a.qdf != k->qdf || a.pairs.num_pairs != k->num_pairs || a.ctl.num_zs != k->num_ctl_zs)
        return hipErrorInvalidValue;
    StarkJitArgs p;
    uint32_t qdb = 0;
    if (hipError_t e = stark_point_args(tb, a, out, &p, &qdb); e != hipSuccess) return e;
    hipFunction_t fn;
    if (hipError_t e = k->function(&fn); e != hipSuccess) return e;
    const uint64_t size = 1ull << (a.degree_bits + qdb);
    void *args[] = {&p};
    return hipModuleLaunchKernel(fn, (unsigned)((size + 127) / 128), 1, 1, 128, 1, 1, 0, stream, args, nullptr);
}

}  // namespace plonky2_hip
