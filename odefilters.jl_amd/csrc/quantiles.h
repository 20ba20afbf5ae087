// Ensemble quantiles on the device (include/odefilter.h, odef_quantile_field): per time the type-7 quantiles of
// every solution component of the posterior means over the included trajectories -- the order statistics that the ensemble
// summary (summary.h) leaves out.  Host-side interface of quantiles.hip; this header includes none of the step headers, so that
// no filter / smoother kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "pass_host.h"

namespace odef {

// the two cached arrays of one source, device memory owned by the context
struct QuantileCache {
  long long* count = nullptr;  // [n_t]
  double* q = nullptr;         // [n_t][P][d]
  size_t count_cap = 0, q_cap = 0;  // bytes
  long n_t = 0;
  int P = 0;
  bool valid = false;
};

struct QuantileState {
  QuantileCache src[3];
  // workspace of one slab of times (quantile_kernels.h), grown like SummaryState::part
  void* mask = nullptr;
  void* range = nullptr;   // kmin, kmax
  void* rows = nullptr;    // low, max_low
  void* ranks = nullptr;   // prefix, rem, owner
  void* hist = nullptr;
  size_t mask_cap = 0, range_cap = 0, rows_cap = 0, ranks_cap = 0, hist_cap = 0;
  PassTimer timer;
};

struct QuantileArgs {
  const double* mean;  // [n_t][D][N]
  const int* retcode;  // [N]
  long N, n_t;
  int d, D, P;
  double probs[8];     // validated: finite, in [0, 1]
};

// Selects the quantiles of `a` into `c` on `stream` and waits for them (it synchronises the stream once per slab of times).  Returns 0, or -1 with `err` set.
int quantiles_run(QuantileState& st, QuantileCache& c, const QuantileArgs& a, hipStream_t stream, float* ms, int* n_launches,
                  std::string& err);
void quantiles_free(QuantileState& st);

}  // namespace odef
