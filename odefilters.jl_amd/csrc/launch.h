// Internal launcher interface between the C-ABI layer (api.hip) and the kernel TUs.
#pragma once
#include <hip/hip_runtime.h>
#include "ek_lane.h"
#include "team.h"
#include "dense_lane.h"
#include "sample_lane.h"
#include "rows_launch.h"

namespace odef {
struct ErrArgs;       // errors_kernels.h
struct AnalyticArgs;  // errors_kernels.h
// The launchers say which kernel they picked (printf-style; the name a profiler prints); api.hip hands it out through
// odef_kernel_name.  One slot per host thread: read back right after the launch call.
void note_kernel(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* last_kernel();
inline const char* tf(bool b) { return b ? "true" : "false"; }
// The launch functions of one vector field, one table per field: the compiled-in ones in their inst_*.hip, a run-time
// compiled one in the shared object jit.hip builds around it.  The launch functions return 0 on success, -2 when the order
// (or algorithm) is not instantiated, -3 when the state dimension is outside the kernels' range.
struct FieldLaunch {
  int d;
  // fixed grid or adaptive; workgroup-per-trajectory fields: every-step records through `stage` when all of them fit, and
  // `staged_recs` (may be null) set to the number of records the kernel left there (trajectory-major, record r at r N ld), 0 if none
  int (*filter)(int q, int ek1, const FilterParams& P, hipStream_t s, int adaptive, double* stage, size_t stage_doubles, long* staged_recs);
  int (*smooth)(int q, const SmoothParams& P, double* ws, hipStream_t s);  // records in place
  // `filter_recs_in_stage` == n_rec: the filter's records 0 .. n_rec - 1 are still in `stage` (nothing to copy in)
  int (*smooth_staged)(int q, const SmoothParams& P, long n_rec, double* ws, double* stage, size_t stage_doubles, hipStream_t s, long filter_recs_in_stage);
  int (*dense)(int q, const DenseParams& P, double* ws, hipStream_t s);    // ws: dense_d28_grid(items) x smooth_ws(q) doubles
  int (*sample)(int q, const SampleParams& P, double* ws, hipStream_t s);
  size_t (*smooth_ws)(int q);  // doubles of workspace per trajectory (smoother) / per grid slot (dense output, sampling)
  // smooth_staged and smooth_ws are null for the lane / row-team fields (their launchers ignore `ws` and the stage): a table
  // with them is a field on the workgroup-per-trajectory kernels
  // solution errors against the field's own `analytic` (errors_field.h); null for a field that has none
  int (*errors)(const ErrArgs& a, const AnalyticArgs& t, unsigned grid, unsigned block, size_t lds, double* truth_out, hipStream_t s,
                char* kname, size_t kname_n) = nullptr;
};
// Layout stamp of what crosses between the library and a run-time compiled module (jit.hip builds one from the headers it
// finds at run time: a tree whose headers moved on without a rebuild of the library must be refused, not launched)
inline unsigned long team_abi_stamp() {
  return sizeof(FilterParams) * 1000003ul + sizeof(SmoothParams) * 10007ul + sizeof(DenseParams) * 101ul + sizeof(SampleParams) + sizeof(FieldLaunch) * 7ul;
}
const FieldLaunch* field_fhn();
const FieldLaunch* field_lorenz63();
const FieldLaunch* field_lotka_volterra();
const FieldLaunch* field_vanderpol();
const FieldLaunch* field_linear();
const FieldLaunch* field_forced();  // time-dependent: f(u, p, t)
const FieldLaunch* field_pleiades();  // d = 28 (BASELINE config 4)
const FieldLaunch* field_lorenz96();  // d = 16: the same kernels on a second shape
const FieldLaunch* field_launch(int rhs_id);  // the compiled-in fields; nullptr for any other id
long dense_d28_grid(long items);  // grid of the dense-output / sampling kernels (workspaces of smooth_ws(q) doubles)
}  // namespace odef
