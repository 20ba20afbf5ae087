// Per-trajectory solution errors on the device (include/odefilter.h, odef_errors_field): for every trajectory,
// over its own saves, FINAL / L2 / LINF of e = u - u* (DiffEqBase's calculate_solution_errors!, restated), the calibration
// statistic CHI2 = mean_k e' Sigma_k^+ e / d, the number of saves used, and on request u* itself.  Host-side interface of
// errors.hip; this header includes none of the step headers, so that no filter / smoother kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "pass_host.h"

namespace odef {

struct ErrArgs;       // errors_kernels.h
struct AnalyticArgs;  // errors_kernels.h
// The launcher a vector field with an `analytic` member provides (errors_field.h; FieldLaunch::errors in launch.h).  truth_out ==
// nullptr: errors_partial_kernel over `grid` workgroups of `block` threads; else errors_truth_kernel into truth_out.
using ErrorsFieldFn = int (*)(const ErrArgs& a, const AnalyticArgs& t, unsigned grid, unsigned block, size_t lds, double* truth_out,
                              hipStream_t s, char* kname, size_t kname_n);

// the cached arrays of one source, device memory owned by the context
struct ErrorsCache {
  double* val[4] = {nullptr, nullptr, nullptr, nullptr};  // FINAL, L2, LINF, CHI2 [N]
  long long* nused = nullptr;                             // [N]
  double* truth = nullptr;                                // U_ANALYTIC [n_save][d][N], filled when asked for
  size_t truth_cap = 0;
  bool truth_valid = false;
  bool valid = false;
};

struct ErrorsState {
  ErrorsCache src[2];
  double* part = nullptr;   // per-chunk partials [n_split][4][N]
  int* part_cnt = nullptr;  // [n_split][2][N]
  size_t part_cap = 0, cnt_cap = 0;
  PassTimer timer;
};

struct ErrorsRequest {
  const double* mean;   // [n_save][D][N]
  const double* cov;    // [n_save][TRI][N]
  const double* tsave;  // adaptive: [n_save][N]
  const int* nsaved;    // adaptive: [N]
  long N, n_save;
  int d, D, TRI;
  const double* ref;    // bound reference [n_save][d][N], or nullptr: the field's analytic
  ErrorsFieldFn field;  // (ref == nullptr)
  const double* u0;     // [d][N]
  const double* p;      // [np] or [np][N]
  int p_shared;
  const double* t;      // time of save k of trajectory i at t[k t_sk + i t_si]
  long t_sk, t_si;
};

// Runs the pass on `stream` (two launches) into `c` and waits.  Returns 0, or -1 with `err` set.  kname: the partial kernel that ran.
int errors_run(ErrorsState& st, ErrorsCache& c, const ErrorsRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname,
               size_t kname_n, std::string& err);
// u* at every save slot from the field's analytic, into c.truth (one launch); waits
int errors_truth(ErrorsCache& c, const ErrorsRequest& r, hipStream_t stream, std::string& err);
void errors_free(ErrorsState& st);

}  // namespace odef
