// Weighted ensemble summary on the device (include/odefilter.h, odef_wsummary_field): per time the moments of the
// importance-weighted mixture of the trajectories' Gaussians -- weights w_i proportional to exp(l_i) with l the bound
// log-weights --, the effective sample size and the log evidence.  Host-side interface of wsummary.hip; this header includes
// none of the step headers, so that no filter / smoother kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "pass_host.h"

namespace odef {

// the six cached arrays of one source, device memory owned by the context
struct WSummaryCache {
  long long* count = nullptr;  // [n_t]
  double* mean = nullptr;      // [n_t][d]
  double* within = nullptr;    // [n_t][tri(d)]
  double* between = nullptr;   // [n_t][tri(d)]
  double* logev = nullptr;     // [n_t]
  double* ess = nullptr;       // [n_t]
  size_t count_cap = 0, mean_cap = 0, within_cap = 0, between_cap = 0, logev_cap = 0, ess_cap = 0;  // bytes
  long n_t = 0;
  bool valid = false;
};

struct WSummaryState {
  WSummaryCache src[3];
  // workspace of one request (wsummary_kernels.h), grown like SummaryState::part
  void* key = nullptr;       // the shift L as an order-preserving key
  void* v = nullptr;         // exp(l_i - L) [N]
  void* zsum = nullptr;      // Z per time [n_t]
  void* part = nullptr;      // per-wavefront partial sums of a pass [n_t][n_wave][2 + d + tri(d)]
  void* part_cnt = nullptr;  // per-wavefront counts [n_t][n_wave]
  size_t key_cap = 0, v_cap = 0, zsum_cap = 0, part_cap = 0, cnt_cap = 0;
  PassTimer timer;
};

struct WSummaryArgs {
  const double* mean;   // [n_t][D][N]
  const double* cov;    // [n_t][TRI][N]
  const int* retcode;   // [N]
  const double* logw;   // [N], the caller's
  long N, n_t;
  int d, D, TRI;
};

// Reduces `a` into `c` on `stream` (six launches) and waits for them.  Returns 0, or -1 with `err` set.  walk: the template
// argument K of the two reduction kernels that ran (trajectories per lane).
int wsummary_run(WSummaryState& st, WSummaryCache& c, const WSummaryArgs& a, hipStream_t stream, float* ms, int* n_launches,
                 int* walk, std::string& err);
void wsummary_free(WSummaryState& st);

}  // namespace odef
