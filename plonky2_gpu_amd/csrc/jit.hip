// jit.hip — the hiprtc runtime (jit.h). What is compiled side by side and how code objects are loaded is the generators' business.
#include "jit.h"

#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

namespace plonky2_hip {

namespace {
const char *const GL_FIELD_SRC =
#include "build/gl_field_src.inc"
    ;
const char *const JIT_ARCH = "gfx950";
}  // namespace
const char *jit_field_source() { return GL_FIELD_SRC; }

// Where compiled code objects are kept: $PLONKY2_HIP_KERNEL_CACHE (empty = no cache), else the directory
// `kernel_cache` next to this shared library if it exists — the place __graft_entry__.build() precompiles the
// compiled-in ed25519 gate kernel into, so that it ships with the library like any ahead-of-time kernel.
std::string jit_cache_dir() {
    if (const char *dir = getenv("PLONKY2_HIP_KERNEL_CACHE")) return dir;
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void *>(&jit_cache_dir), &info) || !info.dli_fname) return "";
    std::string lib(info.dli_fname);
    size_t slash = lib.rfind('/');
    std::string dir = (slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/kernel_cache";
    struct stat st;
    return (stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) ? dir : "";
}

// Cache file name of a compiled source: keyed by a hash of the generated source and of what turns the same source into a different
// code object — the hiprtc version and the target. `prefix`: "gate_" for a circuit's units, "stark_" for a STARK's quotient kernel.
std::string jit_cache_path(const std::string &dir, const std::string &source, const char *prefix) {
    if (dir.empty()) return "";
    int rtc_major = 0, rtc_minor = 0;
    (void)hiprtcVersion(&rtc_major, &rtc_minor);
    const std::string salt = "hiprtc " + std::to_string(rtc_major) + "." + std::to_string(rtc_minor) + " " + JIT_ARCH + "\n";
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a
    for (unsigned char ch : salt) h = (h ^ ch) * 0x100000001b3ull;
    for (unsigned char ch : source) h = (h ^ ch) * 0x100000001b3ull;
    char name[64];
    snprintf(name, sizeof name, "/%s%016llx", prefix, (unsigned long long)h);
    return dir + name;
}

// $PLONKY2_HIP_KERNEL_CACHE_LIST=<file>: the cache entries this build uses, one path per line (appended) — how build() tells the
// current generator's units from whatever else the cache directory holds without compiling anything twice (__graft_entry__.py)
void jit_cache_list(const std::vector<std::string> &cache_paths) {
    if (const char *lf = getenv("PLONKY2_HIP_KERNEL_CACHE_LIST"))
        if (FILE *f = fopen(lf, "a")) {
            for (const std::string &cp : cache_paths)
                if (!cp.empty()) fprintf(f, "%s\n", cp.c_str());
            fclose(f);
        }
}

bool jit_cache_read(const std::string &cache_path, std::vector<char> *code) {
    if (cache_path.empty()) return false;
    std::ifstream f(cache_path + ".hsaco", std::ios::binary);
    if (f) code->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return !code->empty();
}

// hiprtc on one source; the code object (and the source, for inspection) goes to the cache. May run on a thread of its own.
bool jit_compile(const std::string &source, const char *program_name, const std::string &cache_path, std::vector<char> *code, std::string *error) {
    hiprtcProgram prog;
    hiprtcResult r = hiprtcCreateProgram(&prog, source.c_str(), program_name, 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) {
        *error = std::string("hiprtcCreateProgram: ") + hiprtcGetErrorString(r);
        return false;
    }
    const std::string arch = std::string("--offload-arch=") + JIT_ARCH;
    const char *opts[] = {arch.c_str(), "-O3", "-std=c++17"};
    r = hiprtcCompileProgram(prog, 3, opts);
    if (r != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, '\0');
        if (ls) hiprtcGetProgramLog(prog, &log[0]);
        *error = std::string("hiprtcCompileProgram: ") + hiprtcGetErrorString(r) + "\n" + log.substr(0, 4000);
        hiprtcDestroyProgram(&prog);
        return false;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    code->resize(cs);
    hiprtcGetCode(prog, code->data());
    hiprtcDestroyProgram(&prog);
    if (!cache_path.empty()) {
        // Several processes (one per GPU) may build the same circuit at once: each writes a file of its own and
        // renames it into place, so a reader sees either nothing or a whole code object.
        const std::string pid = std::to_string((long long)getpid()) + "." + std::to_string((unsigned long long)(uintptr_t)code);
        const std::string tmp = cache_path + ".tmp." + pid, tmp_src = cache_path + ".hip." + pid;
        std::ofstream(tmp_src) << source;
        (void)rename(tmp_src.c_str(), (cache_path + ".hip").c_str());
        bool written = false;
        {
            std::ofstream f(tmp, std::ios::binary);
            f.write(code->data(), (std::streamsize)code->size());
            f.flush();
            written = f.good();
        }
        if (!written || rename(tmp.c_str(), (cache_path + ".hsaco").c_str()) != 0) (void)remove(tmp.c_str());
    }
    return true;
}

bool code_object_whole(const std::vector<char> &code) {
    if (code.size() < 64 || memcmp(code.data(), "\177ELF", 4) != 0) return false;
    uint64_t shoff = 0;
    uint16_t shentsize = 0, shnum = 0;
    memcpy(&shoff, code.data() + 0x28, 8), memcpy(&shentsize, code.data() + 0x3A, 2), memcpy(&shnum, code.data() + 0x3C, 2);
    return shoff >= 64 && shnum != 0 && shoff <= code.size() && (uint64_t)shentsize * shnum <= code.size() - shoff;
}

}  // namespace plonky2_hip
