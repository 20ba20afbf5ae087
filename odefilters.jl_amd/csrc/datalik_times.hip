// Data log-likelihood at arbitrary observation times, on fixed and on adaptive grids (datalik.h).  One lane per
// trajectory sweeps its own filter records backwards and inserts a predicted node per observation time that is no save; one
// launch.  The kernels depend on (d, q) only and are instantiated here once, for the pairs the lane dense output serves.
#include "datalik.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "datalik_times_kernels.h"

namespace odef {
namespace {

template <int d, int q>
void launch(const DataLikTimesArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((data_loglik_times_kernel<d, q>), dim3((unsigned)((a.N + kDataLikWave - 1) / kDataLikWave)), dim3(kDataLikWave), 0,
                     st, a);
}

template <int d, int q>
bool launch_if(const DataLikTimesArgs& a, hipStream_t st) {
  if constexpr (d * (q + 1) <= kDataLikTimesMaxState) {
    launch<d, q>(a, st);
    return true;
  }
  return false;
}

template <int d>
bool launch_order(int q, const DataLikTimesArgs& a, hipStream_t st) {
  switch (q) {
    case 1: return launch_if<d, 1>(a, st);
    case 2: return launch_if<d, 2>(a, st);
    case 3: return launch_if<d, 3>(a, st);
    case 4: return launch_if<d, 4>(a, st);
    case 5: return launch_if<d, 5>(a, st);
    default: return false;
  }
}

}  // namespace

bool datalik_times_has(int d, int q) {
  return d >= 1 && d <= kDataLikMaxD && q >= 1 && q <= 5 && d * (q + 1) <= kDataLikTimesMaxState;
}

int datalik_times_run(DataLikState& st, const DataLikTimesRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname,
                      size_t kname_n, std::string& err) {
  st.valid = false;
  if (!datalik_times_has(r.d, r.q))
    return pass_fail(err, "data log-likelihood at times: no kernel for (d, q) = (%d, %d); built for d <= 4, q <= 5, d (q + 1) <= 12", r.d,
                     r.q);
  const int D = r.d * (r.q + 1), TRI = D * (D + 1) / 2;
  if (r.N < 1 || r.n_save < 2 || (size_t)TRI * (size_t)r.N * sizeof(double) >= (1ull << 31))
    return pass_fail(err, "data log-likelihood: n_traj * D(D+1)/2 * 8 bytes must stay below 2 GiB per save slot; shard the ensemble");
  // M and o follow from the byte counts
  if (r.time_bytes == 0 || r.time_bytes % 8 || r.time_bytes / 8 >= (1ull << 31) || r.comp_bytes == 0 || r.comp_bytes % 8 ||
      r.comp_bytes / 8 > (size_t)r.d)
    return pass_fail(err, "data log-likelihood: byte counts do not agree: ODEF_L_OBS_TIME holds %zu bytes (1 .. 2^31 - 1 doubles), "
                          "ODEF_L_OBS_COMPONENT %zu (1 .. d int64)", r.time_bytes, r.comp_bytes);
  const size_t M = r.time_bytes / 8, o = r.comp_bytes / 8;
  if (r.noise_bytes != o * 8 || (r.val_bytes != M * o * 8 && r.val_bytes != M * o * (size_t)r.N * 8))
    return pass_fail(err,
                     "data log-likelihood: byte counts do not agree: M = %zu times and o = %zu components need ODEF_L_OBS_NOISE of %zu bytes "
                     "(got %zu) and ODEF_L_OBS_VALUE of %zu (shared) or %zu (per trajectory) bytes (got %zu)",
                     M, o, o * 8, r.noise_bytes, M * o * 8, M * o * (size_t)r.N * 8, r.val_bytes);
  std::vector<double> tau(M), noise(o);
  std::vector<long long> comp(o);
  hipError_t e = hipMemcpyAsync(tau.data(), r.obs_time, M * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(comp.data(), r.obs_comp, o * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(noise.data(), r.obs_noise, o * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return pass_fail(err, "data log-likelihood: %s", hipGetErrorString(e));
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
  for (size_t a = 0; a < o; ++a)
    if (comp[a] < 0 || comp[a] >= r.d || (a > 0 && comp[a] <= comp[a - 1]))
      return pass_fail(err, "data log-likelihood: observed components must be strictly increasing within 0 .. d - 1 = %d "
                            "(entry %zu is %lld)", r.d - 1, a, comp[a]);
  for (size_t a = 0; a < o; ++a)
    if (!std::isfinite(noise[a]) || !(noise[a] > 0.0))
      return pass_fail(err, "data log-likelihood: noise variances must be finite and positive (entry %zu is %g)", a, noise[a]);
  for (double*& v : st.out)
    if (!v && hipMalloc((void**)&v, sizeof(double) * r.N) != hipSuccess) {
      (void)hipGetLastError();
      v = nullptr;
      return pass_fail(err, "data log-likelihood: out of device memory");
    }
  DataLikTimesArgs a;
  a.pc = *r.pc;
  a.N = r.N;
  a.n_save = r.n_save;
  a.adaptive = r.adaptive;
  a.tgrid = r.tgrid;
  a.tsave = r.tsave;
  a.nsaved = r.nsaved;
  a.mean = r.mean;
  a.cov = r.cov;
  a.diff = r.diff;
  a.obs_time = r.obs_time;
  a.obs_comp = (const long long*)r.obs_comp;
  a.obs_val = r.obs_val;
  a.obs_noise = r.obs_noise;
  a.M = (int)M;
  a.o = (int)o;
  a.per_traj = r.val_bytes != M * o * 8;
  a.loglik = st.out[0];
  a.maha = st.out[1];
  a.host_n_hi = 0;
  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "data log-likelihood: hipEventCreate failed");
  bool ok = false;
  switch (r.d) {
    case 1: ok = launch_order<1>(r.q, a, stream); break;
    case 2: ok = launch_order<2>(r.q, a, stream); break;
    case 3: ok = launch_order<3>(r.q, a, stream); break;
    case 4: ok = launch_order<4>(r.q, a, stream); break;
    default: break;
  }
  if (!ok) return pass_fail(err, "data log-likelihood at times: no kernel");
  if (kname) std::snprintf(kname, kname_n, "odef::data_loglik_times_kernel<%d, %d>", r.d, r.q);
  if (e = st.timer.end(stream, ms); e != hipSuccess) return pass_fail(err, "data log-likelihood: %s", hipGetErrorString(e));
  if (n_launches) *n_launches += 1;  // a running count: a request served from the cache leaves it unchanged
  st.valid = true;
  return 0;
}

}  // namespace odef
