// Data log-likelihood of noisy observations per trajectory on the device (include/odefilter.h, odef_data_field):
// the marginal likelihood of y_j = H x(t_{k_j}) + N(0, diag r) under the Gauss-Markov posterior that the filter records and the
// smoother's backward transitions define, by one backward sweep over the records of a fixed grid.  Host-side interface of
// datalik.hip; this header includes none of the step headers, so that no filter / smoother kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "pass_host.h"

namespace odef {

struct PriorConsts;  // ek_math.h

struct DataLikState {
  double* out[2] = {nullptr, nullptr};  // DATA_LOGLIK, DATA_MAHALANOBIS [N], device memory owned by the context
  bool valid = false;
  PassTimer timer;
};

// what a request says whichever way the observations are placed in time: the filter records and the observed components
struct DataLikObsRequest {
  const PriorConsts* pc;
  long N, n_save;          // fixed grid: number of saves; adaptive: capacity of the records
  int d, q;
  const double* mean;      // filter records, ABI layout
  const double* cov;
  const double* diff;
  const void* obs_comp;    // [o] int64
  const double* obs_val;   // [M][o] or [M][o][N]
  const double* obs_noise; // [o]
  size_t comp_bytes, val_bytes, noise_bytes;
};

struct DataLikRequest : DataLikObsRequest {
  const double* ptab;      // the grid's tables, as the smoother takes them
  const int* tab_idx;
  const double* hs;
  const void* obs_save;    // [M] int64
  size_t save_bytes;
};

// true when data_loglik_kernel<d, q> is instantiated (d <= 4, q <= 5, d (q + 1) <= 20)
bool datalik_has(int d, int q);
// Copies saves, components and noise to the host (M + 2 o words) and validates them, runs the pass on `stream` (one launch) into
// `st` and waits.  Returns 0, or -1 with `err` set.
int datalik_run(DataLikState& st, const DataLikRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname, size_t kname_n,
                std::string& err);
void datalik_free(DataLikState& st);

// The same likelihood at arbitrary observation times, on fixed and on adaptive grids (datalik_times.hip): the sweep
// runs over every trajectory's own records plus one predicted node per time that is no save.  Same state, same outputs.
struct DataLikTimesRequest : DataLikObsRequest {
  int adaptive;
  double t0;               // the first save time (of every trajectory)
  double t_last;           // fixed grid: the last save time
  const double* tgrid;     // fixed: [n_save], device
  const double* tsave;     // adaptive: [n_save][N]
  const int* nsaved;       // adaptive: [N]
  const double* obs_time;  // [M] doubles
  size_t time_bytes;
};

// true when data_loglik_times_kernel<d, q> is instantiated (d <= 4, q <= 5, d (q + 1) <= 12)
bool datalik_times_has(int d, int q);
// Copies times, components and noise to the host (M + 2 o words) and validates them, runs the pass on `stream` (one launch) into
// `st` and waits.  Returns 0, or -1 with `err` set.
int datalik_times_run(DataLikState& st, const DataLikTimesRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname,
                      size_t kname_n, std::string& err);

}  // namespace odef
