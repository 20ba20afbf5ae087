// Ensemble summary on the device (include/odefilter.h, odef_summary_field): per time the count of the
// included trajectories, the mean of their posterior means, the mean of their posterior covariances (within) and the
// covariance of their means (between), over the solution part (rows 0..d-1) of a record.  Host-side interface of
// summary.hip; this header includes none of the step headers, so that no filter / smoother kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "pass_host.h"

namespace odef {

// the four cached arrays of one source, device memory owned by the context
struct SummaryCache {
  long long* count = nullptr;  // [n_t]
  double* mean = nullptr;      // [n_t][d]
  double* within = nullptr;    // [n_t][tri(d)]
  double* between = nullptr;   // [n_t][tri(d)]
  long cap_t = 0;              // capacity in times
  long n_t = 0;
  bool valid = false;
};

struct SummaryState {
  SummaryCache src[3];
  double* part = nullptr;  // per-wavefront partial sums of a pass [n_t][n_wave][d + tri(d)]
  int* part_cnt = nullptr; // per-wavefront counts [n_t][n_wave]
  size_t part_cap = 0, cnt_cap = 0;
  PassTimer timer;
};

struct SummaryArgs {
  const double* mean;  // [n_t][D][N]
  const double* cov;   // [n_t][TRI][N]
  const int* retcode;  // [N]
  long N, n_t;
  int d, D, TRI;
};

// Reduces `a` into `c` on `stream` (four launches) and waits for them.  Returns 0, or -1 with `err` set.  walk: the template
// argument K of the two reduction kernels that ran (trajectories per lane).
int summary_run(SummaryState& st, SummaryCache& c, const SummaryArgs& a, hipStream_t stream, float* ms, int* n_launches,
                int* walk, std::string& err);
void summary_free(SummaryState& st);

}  // namespace odef
