// Run-time compiled vector fields.
// The reference calls a Julia closure f (and f.jac / ForwardDiff) in the middle of every step
// (src/perform_step.jl:106,116-121).  A device kernel cannot call back into the host, so a user vector field is
// handed over as SOURCE: a struct with the interface of the compiled-in registry (csrc/rhs.h) -- f generic in the
// scalar type, so that the same text serves the step (double) and the Taylor-mode initialisation (truncated jets,
// src/state_initialization.jl:2-53), plus the analytic Jacobian for EK1 (optional).  hipcc compiles the very same
// kernels AND their host-side launchers around it for gfx950, as a shared object that exports the field's FieldLaunch
// table (launch.h): from there the field runs exactly as a compiled-in one.
#include <elf.h>
#include <dirent.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <spawn.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cerrno>

#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "jit.h"

extern char** environ;

namespace odef {
namespace {

struct JitRhs {
  std::string name, source, include_dir;
  int d, np;
  bool has_time = false;  // f(u, p, t): `static constexpr bool has_time = true` in the struct (rhs.h)
};

std::mutex g_mu;
std::vector<JitRhs> g_rhs;                                                      // id = kJitFirstId + index
std::map<std::tuple<int, int, int, int, int>, const FieldLaunch*> g_fields;      // (id, q, ek1, mv, ieks): shared objects, never unloaded

// path of this library (the run-time compiled shared objects link against it: note_kernel)
std::string this_library() {
  Dl_info info;
  if (dladdr((const void*)&this_library, &info) && info.dli_fname) return info.dli_fname;
  return std::string();
}

// Where the kernel headers live: $ODEFILTER_HIP_INCLUDE, else `../csrc` next to the directory this library was loaded
// from (odefilters.jl_amd/lib/libodefilter_hip.so -> odefilters.jl_amd/csrc; found with dladdr, so a tree that was moved
// or copied after the build still compiles user vector fields), else the directory of the build.
std::string default_include_dir() {
  if (const char* e = getenv("ODEFILTER_HIP_INCLUDE")) return e;
  Dl_info info;
  if (dladdr((const void*)&default_include_dir, &info) && info.dli_fname) {
    std::string lib = info.dli_fname;
    const size_t slash = lib.rfind('/');
    const std::string dir = (slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/../csrc";
    if (access((dir + "/ek_lane.h").c_str(), R_OK) == 0) return dir;
  }
#ifdef ODEF_DEFAULT_CSRC
  return ODEF_DEFAULT_CSRC;
#else
  return ".";
#endif
}

// a kernel whose NAME says whether the struct is a time-dependent field (HasTime, rhs.h): jit_register reads it off the code object
const char* const kTimeFlag =
    "template <bool HAS_TIME>\n__global__ void odef_jit_time_flag() {}\n"
    "template __global__ void odef_jit_time_flag<HasTime<RhsJit>::value>();\n";

// The module of one order and algorithm: the launchers of the compiled-in fields instantiated around the user's struct --
// the lane / row-team ones of ek_kernels.h up to state dimension 20, the workgroup-per-trajectory ones of team_launch_impl.h
// (kernels: team_kernels.h) above (exactly what inst_lorenz63.hip / inst_lorenz96.hip are for a compiled-in field) -- exporting their table.
// mv: with the kernels of the MV diffusion models (lane path, EK0; an MV context only, so that a scalar-model module is not
// built any slower); ieks: with the IEKS kernels (lane path, EK1; an IEKS context only, likewise)
std::string module_source(const JitRhs& r, int q, int ek1, int mv, int ieks) {
  const int D = r.d * (q + 1);
  const bool team = jit_team_path(r.d, q);
  const std::string Q = std::to_string(q), EK = ek1 ? "true" : "false", DD = std::to_string(r.d), MV = mv ? "true" : "false",
                    T = DD + ", " + Q + ", " + MV;
  const std::string TT = DD + ", " + Q;  // (the workgroup-per-trajectory launchers: scalar models only)
  std::string s;
  if (D > 12 && !team) s += "#define ODEF_ROWSTORE_FREE_OFFSET 1\n";  // see RowStore (ek_lane.h)
  s += team ? "#include \"team_launch_impl.h\"\n" : "#include \"ek_kernels.h\"\n";
  s += "#include \"errors_field.h\"\n";  // the solution-error kernels, when the struct has an `analytic`
  s += "namespace odef {\n";
  s += r.source;
  s += "\nstruct RhsJit : " + r.name + " { static constexpr const char* name = \"" + r.name + "\"; };\n";
  s += "static_assert(RhsJit::d == " + DD + ", \"d of the struct differs from the d passed to odef_rhs_compile\");\n";
  s += "static_assert(RhsJit::np == " + std::to_string(r.np) + ", \"np of the struct differs from the n_params passed to odef_rhs_compile\");\n";
  s += kTimeFlag;
  s += "}  // namespace odef\n";
  s += "extern \"C\" unsigned long odef_jit_abi() { return odef::team_abi_stamp(); }\n";
  s += "extern \"C\" const odef::FieldLaunch* odef_jit_field() {\n  using namespace odef;\n  static const FieldLaunch t = {" + DD + ", ";
  if (team)
    s += "team_filter<RhsJit, " + Q + ", " + EK + ">, team_smooth_inplace<" + TT + ">, team_smooth_staged<" + TT + ">, team_dense<" + TT +
         ">, team_sample<" + TT + ">, team_smooth_ws<" + TT + ">";
  else
    s += "lane_filter<RhsJit, " + Q + ", " + EK + ", " + MV + ", " + (ieks ? "true" : "false") + ">, lane_smooth<" + T + ">, nullptr, lane_dense<" + T + ">, lane_sample<" + T + ">, nullptr";
  s += ", errors_launcher<RhsJit>()};\n  return &t;\n}\n";
  return s;
}

// What odef_rhs_compile builds for d > 10 (no lane kernel exists to try the text on): the vector field in double, in
// forward mode (the Jacobian EK1 needs when the struct has none), on Taylor jets (the initialisation), and its `analytic` if it has one
// -- through the wrappers of rhs.h, so that a time-dependent field (has_time) is probed with its own signatures
std::string probe_translation_unit(const JitRhs& r) {
  const std::string DD = std::to_string(r.d);
  std::string s = "#include \"ek_lane.h\"\n#include \"errors_field.h\"\nnamespace odef {\n";
  s += r.source;
  s += "\nusing RhsJit = " + r.name + ";\n";
  s += "static_assert(RhsJit::d == " + DD + ", \"d of the struct differs from the d passed to odef_rhs_compile\");\n";
  s += "static_assert(RhsJit::np == " + std::to_string(r.np) + ", \"np of the struct differs from the n_params passed to odef_rhs_compile\");\n";
  s += "template <class R>\n__device__ void probe_analytic(const double (&u0)[R::d], const double* p, double t, double& acc) {\n"
       "  if constexpr (HasAnalytic<R>::value) {\n    TruthAnalytic<R> tr(AnalyticArgs{u0, p, &t, 1, 0, 0, 1});\n    tr.init(0);\n    tr.at(0, 0);\n    acc += tr.get(0);\n  }\n}\n";
  s += "extern \"C\" __global__ void odef_jit_probe(const double* u, const double* p, double* out) {\n"
       "  constexpr int d = " + DD + ";\n"
       "  double uu[d], du[d], J[d][d], m0[2 * d];\n"
       "  for (int a = 0; a < d; ++a) uu[a] = u[a];\n"
       "  rhs_eval<RhsJit>(uu, p, u[0], du);\n"
       "  rhs_jacobian<RhsJit>(uu, p, u[0], J);\n"
       "  taylor_init<RhsJit, 1>(uu, p, m0, u[0]);\n"
       "  double acc = 0.0;\n"
       "  probe_analytic<RhsJit>(uu, p, u[0], acc);\n"
       "  for (int a = 0; a < d; ++a) acc += du[a] + J[a][a] + m0[d + a];\n"
       "  out[0] = acc;\n}\n";
  s += kTimeFlag;
  s += "}  // namespace odef\n";
  return s;
}

std::string read_file(const std::string& path) {
  std::string out;
  if (FILE* f = fopen(path.c_str(), "rb")) {
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
  }
  return out;
}

// Names of the device functions a code object keeps OUT OF LINE (FUNC symbols without a kernel descriptor `<name>.kd`).
// Such a function is compiled once, for the loosest register budget among its callers; called from a kernel with a
// tighter one (the row-team kernels are pinned to 128 registers) it would address registers its wavefront does not own --
// a memory access fault at run time.  The modules are built with every device function inline, and refused otherwise.
std::string out_of_line_device_functions(const std::string& co) {
  const size_t at = co.find("\x7f" "ELF");
  if (at == std::string::npos || co.size() - at < sizeof(Elf64_Ehdr)) return "";
  const char* base = co.data() + at;
  const size_t avail = co.size() - at;
  Elf64_Ehdr eh;
  std::memcpy(&eh, base, sizeof eh);
  if (eh.e_shentsize != sizeof(Elf64_Shdr) || eh.e_shoff + (size_t)eh.e_shnum * sizeof(Elf64_Shdr) > avail) return "";
  std::set<std::string> funcs, descriptors;
  for (unsigned i = 0; i < eh.e_shnum; ++i) {
    Elf64_Shdr sh;
    std::memcpy(&sh, base + eh.e_shoff + (size_t)i * sizeof sh, sizeof sh);
    if (sh.sh_type != SHT_SYMTAB || sh.sh_link >= eh.e_shnum || sh.sh_offset + sh.sh_size > avail) continue;
    Elf64_Shdr st;
    std::memcpy(&st, base + eh.e_shoff + (size_t)sh.sh_link * sizeof st, sizeof st);
    if (st.sh_offset + st.sh_size > avail) continue;
    for (size_t k = 0; k + sizeof(Elf64_Sym) <= sh.sh_size; k += sizeof(Elf64_Sym)) {
      Elf64_Sym sym;
      std::memcpy(&sym, base + sh.sh_offset + k, sizeof sym);
      if (sym.st_shndx == SHN_UNDEF || sym.st_name >= st.sh_size) continue;
      const char* nm = base + st.sh_offset + sym.st_name;
      const std::string name(nm, strnlen(nm, st.sh_size - sym.st_name));
      if (ELF64_ST_TYPE(sym.st_info) == STT_FUNC) funcs.insert(name);
      else if (name.size() > 3 && name.compare(name.size() - 3, 3, ".kd") == 0) descriptors.insert(name.substr(0, name.size() - 3));
    }
  }
  std::string names;
  for (const auto& f : funcs)
    if (!descriptors.count(f)) names += f + "\n";
  return names;
}

// The lane smoother (smooth_lane.h) keeps a packed matrix and the carried mean in a HAND-MANAGED file at the top of the
// lane's AGPRs, with register numbers fixed in inline assembly the compiler knows nothing about.  That is sound only while
// the compiler's own AGPR use (it parks VGPRs there under pressure, lowest register first) stays below the file.  The
// compiled-in kernels are checked at build time (tests/test_build_hygiene.py); a user's vector field changes nothing in
// that kernel, but the check costs nothing, so the run-time compiled ones are checked on their ISA listing here, by the
// same rule: returns the offending line, or "" when every AGPR reference of the rts_smooth_lane_kernel<d, q, ...> kernels
// outside the file's own assembly lies below its first slot, 2 (128 - (D(D+1)/2 + D)) for D = d(q+1).
std::string agpr_file_violation(const std::string& isa) {
  int first_slot = -1;  // >= 0: inside a lane smoother kernel
  bool in_asm = false;
  size_t pos = 0;
  while (pos < isa.size()) {
    size_t eol = isa.find('\n', pos);
    if (eol == std::string::npos) eol = isa.size();
    const std::string line = isa.substr(pos, eol - pos);
    pos = eol + 1;
    const size_t colon = line.find(':'), k = line.find("rts_smooth_lane_kernel");
    int d = 0, q = 0;
    if (line.rfind("_Z", 0) == 0 && colon != std::string::npos && k < colon &&
        std::sscanf(line.c_str() + k, "rts_smooth_lane_kernelILi%dELi%d", &d, &q) == 2) {
      const int D = d * (q + 1);
      first_slot = 2 * (128 - (D * (D + 1) / 2 + D));  // MS of smooth_lane_v2 (smooth_lane.h), in 32-bit registers
    } else if (line.rfind(".Lfunc_end", 0) == 0) {
      first_slot = -1;
    }
    if (first_slot < 0) continue;
    if (line.find("ASMSTART") != std::string::npos) { in_asm = true; continue; }
    if (line.find("ASMEND") != std::string::npos) { in_asm = false; continue; }
    if (in_asm) continue;
    const std::string code = line.substr(0, line.find(';'));
    for (size_t k = 0; k + 1 < code.size(); ++k) {
      if (code[k] != 'a') continue;
      if (k > 0 && (isalnum((unsigned char)code[k - 1]) || code[k - 1] == '_')) continue;
      size_t j = k + 1;
      if (code[j] == '[') ++j;
      if (j >= code.size() || !isdigit((unsigned char)code[j])) continue;
      // every number of a register or register range: a12, a[12], a[12:13], a[0xdc]
      while (j < code.size() && (isalnum((unsigned char)code[j]) || code[j] == ':')) {
        if (isdigit((unsigned char)code[j])) {
          char* end = nullptr;
          const long r = strtol(code.c_str() + j, &end, 0);
          if (r >= first_slot) return line + " (first slot a" + std::to_string(first_slot) + ")";
          j = (size_t)(end - code.c_str());
        } else {
          ++j;
        }
      }
    }
  }
  return "";
}

void remove_tree(const std::string& dir) {  // the compiler's temporaries (flat directory)
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n != "." && n != "..") remove((dir + "/" + n).c_str());
    }
    closedir(d);
  }
  rmdir(dir.c_str());
}

// Source -> host + device shared object for gfx950, linked against this library (note_kernel), its device code checked
// (out_of_line_device_functions; agpr_file_violation when it holds the lane smoother).  `handle` != nullptr: the module is
// loaded and *handle receives the dlopen handle; else it is discarded.  On failure `err` holds the compiler log.
// The compiler runs as a CHILD PROCESS, not in-process through hiprtc: hiprtc/comgr of ROCm 7.2 aborts the whole host
// process ("LLVM ERROR: Unsupported instruction") on the larger lane kernels (state dimension 14 and up), which the
// offline compiler builds without complaint; a child process can only fail with a log.
// $ODEFILTER_HIP_HIPCC overrides the compiler path (default: hipcc on PATH, then /opt/rocm/bin/hipcc).
// `has_time` != nullptr: receives whether the module's field is time-dependent (kTimeFlag).
bool compile(const std::string& src, const std::string& include_dir, std::string& err, void** handle = nullptr, bool* has_time = nullptr) {
  err.clear();
  char tmpl[] = "/tmp/odef_jit_XXXXXX";
  const char* dir = mkdtemp(tmpl);
  if (!dir) {
    err = "odef_rhs_compile: cannot create a temporary directory under /tmp";
    return false;
  }
  const std::string base = dir, srcp = base + "/rhs.hip", outp = base + "/rhs.so", logp = base + "/log.txt";
  // (handed to the linker with -Wl: hipcc would take a bare path for another HIP source)
  const std::string self_path = this_library(), self = "-Wl," + self_path;
  if (self_path.empty()) {
    err = "odef_rhs_compile: cannot locate libodefilter_hip.so (dladdr) to link the run-time compiled module against";
    remove_tree(base);
    return false;
  }
  {
    FILE* f = fopen(srcp.c_str(), "wb");
    const bool written = f && fwrite(src.data(), 1, src.size(), f) == src.size();
    if (f && fclose(f) != 0) { /* reported below through `written` of the next open */ }
    if (!written) {
      err = "odef_rhs_compile: cannot write the generated source to " + srcp;
      remove_tree(base);
      return false;
    }
  }
  const std::string inc = "-I" + (include_dir.empty() ? default_include_dir() : include_dir);
  const char* env_cc = getenv("ODEFILTER_HIP_HIPCC");
  const char* candidates[] = {env_cc ? env_cc : "hipcc", "/opt/rocm/bin/hipcc"};
  int status = -1;
  bool spawned = false;
  for (const char* cc : candidates) {
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_addopen(&fa, 1, logp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
    posix_spawn_file_actions_adddup2(&fa, 1, 2);
    // (--save-temps=obj: the device code object and its ISA listing land next to the output, for the checks below;
    // -amdgpu-function-calls=false: every device function inline -- kernels with different register budgets must not
    // share an out-of-line callee, see out_of_line_device_functions)
    const char* argv_so[] = {cc, "--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-shared", "--save-temps=obj", "-fno-crash-diagnostics",
                             "-mllvm", "-amdgpu-function-calls=false", inc.c_str(), srcp.c_str(), "-o", outp.c_str(), self.c_str(), nullptr};
    // $ODEFILTER_HIP_JIT_FLAGS: extra compiler flags, space-separated (diagnostic builds: e.g. the LDS poisoning of filter_mfma.h)
    std::vector<std::string> extra;
    if (const char* ef = getenv("ODEFILTER_HIP_JIT_FLAGS")) {
      std::string tok;
      for (const char* c = ef;; ++c) {
        if (*c == ' ' || *c == 0) {
          if (!tok.empty()) extra.push_back(tok);
          tok.clear();
          if (*c == 0) break;
        } else
          tok += *c;
      }
    }
    std::vector<const char*> argv = {cc};  // (the extra flags right behind the compiler's name)
    for (const auto& x : extra) argv.push_back(x.c_str());
    argv.insert(argv.end(), argv_so + 1, argv_so + sizeof argv_so / sizeof *argv_so);
    pid_t pid = 0;
    const int rc = posix_spawnp(&pid, cc, &fa, nullptr, const_cast<char* const*>(argv.data()), environ);
    posix_spawn_file_actions_destroy(&fa);
    if (rc != 0) continue;
    spawned = true;
    while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {
    }
    if (WIFEXITED(status) && WEXITSTATUS(status) == 127) {  // exec failed inside the child: try the next candidate
      spawned = false;
      continue;
    }
    break;
  }
  if (!spawned || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
    if (!spawned) {
      err = "odef_rhs_compile: cannot start hipcc (set ODEFILTER_HIP_HIPCC)";
    } else {
      const std::string log = read_file(logp);
      err = "hipcc: compilation of the user vector field failed\n";
      if (log.find("illegal VGPR to SGPR copy") != std::string::npos || log.find("ran out of registers") != std::string::npos)
        err += "(the lane-per-trajectory kernels keep the whole filter state of a trajectory in registers; this state dimension does not fit)\n";
      err += log.substr(0, 6000);
    }
    remove_tree(base);
    return false;
  }
  const std::string co = read_file(base + "/rhs-hip-amdgcn-amd-amdhsa-gfx950.out");
  const std::string stray = out_of_line_device_functions(co);
  if (has_time) *has_time = co.find("odef_jit_time_flagILb1E") != std::string::npos;
  if (co.empty()) {
    err = "odef_rhs_compile: the compiler left no device code object (rhs-hip-amdgcn-amd-amdhsa-gfx950.out)";
  } else if (!stray.empty()) {
    err = "odef_rhs_compile: the compiler left device functions out of line (kernels with different register budgets would share them):\n" + stray.substr(0, 4000);
  } else if (co.find("rts_smooth_lane_kernel") != std::string::npos) {
    const std::string isa = read_file(base + "/rhs-hip-amdgcn-amd-amdhsa-gfx950.s");
    const std::string bad = isa.empty() ? std::string("(no ISA listing was produced)") : agpr_file_violation(isa);
    if (!bad.empty()) err = "odef_rhs_compile: the compiler's register allocation reaches the smoother's hand-managed AGPR file: " + bad;
  }
  if (err.empty() && handle) {
    // (the mapping outlives the file: the temporary directory goes away below)
    *handle = dlopen(outp.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!*handle) {
      const char* de = dlerror();
      err = std::string("odef_rhs_compile: dlopen of the run-time compiled module failed: ") + (de ? de : "?");
    }
  }
  remove_tree(base);
  return err.empty();
}

}  // namespace

int jit_register(const char* name, const char* source, int d, int np, const char* include_dir, std::string& err) {
  if (!name || !source || !*name) {
    err = "odef_rhs_compile: null or empty name/source";
    return -1;
  }
  if (d < 1 || d > 32 || np < 0) {
    err = "odef_rhs_compile: d must be in 1..32 (lane kernels: d(q+1) <= 20; above that the workgroup-per-trajectory kernels, even d) and n_params >= 0";
    return -1;
  }
  JitRhs r{name, source, include_dir ? include_dir : "", d, np};
  // compile the order-1 EK1 module (d <= 10; a probe kernel above) once now so that errors in the user's text surface here,
  // with the compiler log
  if (!compile(d <= 10 ? module_source(r, 1, 1, 0, 0) : probe_translation_unit(r), r.include_dir, err, nullptr, &r.has_time)) return -1;
  std::lock_guard<std::mutex> lk(g_mu);
  g_rhs.push_back(std::move(r));
  return kJitFirstId + (int)g_rhs.size() - 1;
}

bool jit_lookup(int rhs_id, int* d, int* np) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int k = rhs_id - kJitFirstId;
  if (k < 0 || k >= (int)g_rhs.size()) return false;
  *d = g_rhs[k].d;
  *np = g_rhs[k].np;
  return true;
}

bool jit_has_time(int rhs_id) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int k = rhs_id - kJitFirstId;
  return k >= 0 && k < (int)g_rhs.size() && g_rhs[k].has_time;
}

const FieldLaunch* jit_field(int rhs_id, int q, int ek1, int mv, int ieks, unsigned long abi_stamp, std::string& err) {
  // The hipcc child process takes seconds to minutes: it runs OUTSIDE the registry lock, so that odef_create for other
  // vector fields (jit_lookup, cached modules) is not blocked meanwhile.  Two threads asking for the same uncached
  // module may both compile; the first to publish wins.
  const auto key = std::make_tuple(rhs_id, q, ek1, mv ? 1 : 0, ieks ? 1 : 0);
  JitRhs r;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    const int k = rhs_id - kJitFirstId;
    if (k < 0 || k >= (int)g_rhs.size()) {
      err = "unknown run-time rhs id";
      return nullptr;
    }
    auto it = g_fields.find(key);
    if (it != g_fields.end()) return it->second;
    r = g_rhs[k];  // copy: the vector may grow while we compile
  }
  void* handle = nullptr;
  if (!compile(module_source(r, q, ek1, mv, ieks), r.include_dir, err, &handle)) return nullptr;
  using Entry = const FieldLaunch* (*)();
  using Stamp = unsigned long (*)();
  const Entry entry = (Entry)dlsym(handle, "odef_jit_field");
  const Stamp stamp = (Stamp)dlsym(handle, "odef_jit_abi");
  if (!entry || !stamp || stamp() != abi_stamp) {
    err = !entry || !stamp ? "odef_jit_field / odef_jit_abi missing from the run-time compiled module"
                           : "the run-time compiled module was built from headers that do not match this library (parameter struct layouts differ): rebuild libodefilter_hip.so or point ODEFILTER_HIP_INCLUDE at its csrc";
    dlclose(handle);
    return nullptr;
  }
  const FieldLaunch* t = entry();
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_fields.find(key);
  if (it != g_fields.end()) return it->second;  // (somebody else published it meanwhile; the duplicate module stays loaded, unused)
  g_fields[key] = t;
  return t;
}

}  // namespace odef
