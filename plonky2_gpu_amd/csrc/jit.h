// jit.h — what every run-time compiled kernel of the library shares (a circuit's gates in gate_jit.hip, a STARK's quotient in
// stark_jit.hip): where code objects are kept ($PLONKY2_HIP_KERNEL_CACHE, else `kernel_cache` next to the library; "" = no cache),
// the file name <dir>/<prefix><FNV-1a of hiprtc version + target + source> without its extension, the list $PLONKY2_HIP_KERNEL_CACHE_LIST
// receives, the cached code object if there is one, and hiprtc itself (writes <path>.hsaco and <path>.hip). None touches a device.
#pragma once
#include <string>
#include <vector>

namespace plonky2_hip {

std::string jit_cache_dir();
std::string jit_cache_path(const std::string &dir, const std::string &source, const char *prefix);
void jit_cache_list(const std::vector<std::string> &cache_paths);
bool jit_cache_read(const std::string &cache_path, std::vector<char> *code);
bool jit_compile(const std::string &source, const char *program_name, const std::string &cache_path, std::vector<char> *code, std::string *error);

// a code object that hipModuleLoadData may be given: an ELF whose section header table lies inside the buffer (a file cut short
// loses it: the table is the last thing in the file)
bool code_object_whole(const std::vector<char> &code);
// gl_field.h as text: the field arithmetic of the ahead-of-time kernels, in front of every generated source behind `#define GL_JIT 1`
const char *jit_field_source();

}  // namespace plonky2_hip
