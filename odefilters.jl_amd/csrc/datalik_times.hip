// Data log-likelihood at arbitrary observation times, on fixed and on adaptive grids (datalik.h).  One lane per
// trajectory sweeps its own filter records backwards and inserts a predicted node per observation time that is no save; one
// launch.  The kernels depend on (d, q) only and are instantiated here once, for the pairs the lane dense output serves.
#include "datalik_times_kernels.h"

#include "datalik_host.h"

namespace odef {

bool datalik_times_has(int d, int q) { return has_dq<kDataLikMaxD, kDataLikTimesMaxState>(d, q); }

int datalik_times_run(DataLikState& st, const DataLikTimesRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname,
                      size_t kname_n, std::string& err) {
  st.valid = false;
  if (!datalik_times_has(r.d, r.q))
    return pass_fail(err, "data log-likelihood at times: no kernel for (d, q) = (%d, %d); built for d <= 4, q <= 5, d (q + 1) <= 12", r.d,
                     r.q);
  const DataLikWhen<double> when{r.obs_time, r.time_bytes, (size_t)((1ull << 31) - 1), "ODEF_L_OBS_TIME", "1 .. 2^31 - 1 doubles", "times"};
  auto check_times = [&](const double* tau, size_t M, std::string& err) {
    for (size_t j = 0; j < M; ++j) {
      if (!std::isfinite(tau[j]))
        return pass_fail(err, "data log-likelihood: observation times must be finite (entry %zu is %g)", j, tau[j]);
      if (j > 0 && !(tau[j] > tau[j - 1]))
        return pass_fail(err, "data log-likelihood: observation times must be strictly increasing (entry %zu is %.17g after %.17g)", j,
                         tau[j], tau[j - 1]);
    }
    if (tau[0] < r.t0)
      return pass_fail(err, "data log-likelihood: observation time %.17g lies before the first save t0 = %.17g", tau[0], r.t0);
    if (!r.adaptive && tau[M - 1] > r.t_last)
      return pass_fail(err, "data log-likelihood: observation time %.17g lies above the last save of the grid, %.17g (a time meant as "
                            "that save must equal it exactly)", tau[M - 1], r.t_last);
    return 0;
  };
  DataLikTimesArgs a;
  if (datalik_prepare(st, r, when, stream, check_times, a, err)) return -1;
  a.adaptive = r.adaptive;
  a.tgrid = r.tgrid;
  a.tsave = r.tsave;
  a.nsaved = r.nsaved;
  a.obs_time = r.obs_time;
  a.host_n_hi = 0;
  auto launch = [&]<int d, int q>() {
    hipLaunchKernelGGL((data_loglik_times_kernel<d, q>), dim3((unsigned)((a.N + kDataLikWave - 1) / kDataLikWave)), dim3(kDataLikWave), 0,
                       stream, a);
  };
  return datalik_launch<kDataLikTimesMaxState>(st, r.d, r.q, launch, "data log-likelihood at times", "data_loglik_times_kernel", stream, ms,
                                               n_launches, kname, kname_n, err);
}

}  // namespace odef
