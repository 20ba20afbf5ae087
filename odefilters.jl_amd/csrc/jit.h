// Internal interface of the run-time compilation layer (jit.hip) used by the C-ABI layer (api.hip).
#pragma once
#include <string>

namespace odef {

constexpr int kJitFirstId = 100;  // rhs ids >= 100 are run-time compiled vector fields

// a run-time compiled field runs on the lane / row-team kernels up to state dimension 20 (d <= 10), on the
// workgroup-per-trajectory kernels above (even d <= 32)
inline bool jit_team_path(int d, int q) { return d * (q + 1) > 20 || d > 10; }
// returns the new rhs id (>= kJitFirstId) or -1 with the compiler log in `err`
int jit_register(const char* name, const char* source, int d, int np, const char* include_dir, std::string& err);
bool jit_lookup(int rhs_id, int* d, int* np);
// whether the field is time-dependent (`has_time` in its struct, rhs.h): such a field runs on the lane and row-team kernels only
bool jit_has_time(int rhs_id);
// The launch table (launch.h) of a run-time compiled field for one order and algorithm: compiled once per (rhs, order, alg)
// into a host + device shared object around the field (seconds; minutes on the workgroup-per-trajectory kernels).
// abi_stamp: team_abi_stamp() of the library
struct FieldLaunch;
// mv: the MV diffusion models' kernels are built (only) for an MV context -- a module of its own, the key includes it;
// ieks: the same for the IEKS kernels and an IEKS context
const FieldLaunch* jit_field(int rhs_id, int q, int ek1, int mv, int ieks, unsigned long abi_stamp, std::string& err);

}  // namespace odef
