// What datalik_run (datalik.hip) and datalik_times_run (datalik_times.hip) do alike: everything about a request that does not
// depend on how the observations are placed in time -- by save index or by time, the `when` input --, and the timed launch.
// Host code; included after the kernels of the pass.
#pragma once
#include "datalik.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "datalik_kernels.h"
#include "dispatch_dq.h"

namespace odef {

// the input that places the M observations in time: M words of 8 bytes, at most max_count of them
template <class W>
struct DataLikWhen {
  const W* ptr;
  size_t bytes, max_count;
  const char *field, *range;  // for the messages: "ODEF_L_OBS_SAVE", "1 .. n_save int64"
  const char* noun;           // "saves" / "times"
};

// Derives M and o from the byte counts, copies `when`, components and noise to the host (M + 2 o words) and validates them --
// check_when(words, M, err) judges the first, 0 or the result of pass_fail --, allocates the outputs of `st` and fills the fields
// of the kernel arguments `a` that both passes have (M and o land in a.M, a.o).  Returns 0, or -1 with `err` set.
template <class W, class Args, class CheckWhen>
int datalik_prepare(DataLikState& st, const DataLikObsRequest& r, const DataLikWhen<W>& w, hipStream_t stream, CheckWhen&& check_when,
                    Args& a, std::string& err) {
  static_assert(sizeof(W) == 8);
  const int D = r.d * (r.q + 1), TRI = D * (D + 1) / 2;
  if (r.N < 1 || r.n_save < 2 || (size_t)TRI * (size_t)r.N * sizeof(double) >= (1ull << 31))
    return pass_fail(err, "data log-likelihood: n_traj * D(D+1)/2 * 8 bytes must stay below 2 GiB per save slot; shard the ensemble");
  // M and o follow from the byte counts
  if (w.bytes == 0 || w.bytes % 8 || w.bytes / 8 > w.max_count || r.comp_bytes == 0 || r.comp_bytes % 8 ||
      r.comp_bytes / 8 > (size_t)r.d)
    return pass_fail(err, "data log-likelihood: byte counts do not agree: %s holds %zu bytes (%s), "
                          "ODEF_L_OBS_COMPONENT %zu (1 .. d int64)", w.field, w.bytes, w.range, r.comp_bytes);
  const size_t M = w.bytes / 8, o = r.comp_bytes / 8;
  if (r.noise_bytes != o * 8 || (r.val_bytes != M * o * 8 && r.val_bytes != M * o * (size_t)r.N * 8))
    return pass_fail(err,
                     "data log-likelihood: byte counts do not agree: M = %zu %s and o = %zu components need ODEF_L_OBS_NOISE of %zu bytes "
                     "(got %zu) and ODEF_L_OBS_VALUE of %zu (shared) or %zu (per trajectory) bytes (got %zu)",
                     M, w.noun, o, o * 8, r.noise_bytes, M * o * 8, M * o * (size_t)r.N * 8, r.val_bytes);
  std::vector<W> when(M);
  std::vector<long long> comp(o);
  std::vector<double> noise(o);
  hipError_t e = hipMemcpyAsync(when.data(), w.ptr, M * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(comp.data(), r.obs_comp, o * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(noise.data(), r.obs_noise, o * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return pass_fail(err, "data log-likelihood: %s", hipGetErrorString(e));
  if (check_when(when.data(), M, err)) return -1;
  for (size_t c = 0; c < o; ++c)
    if (comp[c] < 0 || comp[c] >= r.d || (c > 0 && comp[c] <= comp[c - 1]))
      return pass_fail(err, "data log-likelihood: observed components must be strictly increasing within 0 .. d - 1 = %d "
                            "(entry %zu is %lld)", r.d - 1, c, comp[c]);
  for (size_t c = 0; c < o; ++c)
    if (!std::isfinite(noise[c]) || !(noise[c] > 0.0))
      return pass_fail(err, "data log-likelihood: noise variances must be finite and positive (entry %zu is %g)", c, noise[c]);
  for (double*& v : st.out)
    if (!v && hipMalloc((void**)&v, sizeof(double) * r.N) != hipSuccess) {
      (void)hipGetLastError();
      v = nullptr;
      return pass_fail(err, "data log-likelihood: out of device memory");
    }
  a.pc = *r.pc;
  a.N = r.N;
  a.n_save = r.n_save;
  a.mean = r.mean;
  a.cov = r.cov;
  a.diff = r.diff;
  a.obs_comp = (const long long*)r.obs_comp;
  a.obs_val = r.obs_val;
  a.obs_noise = r.obs_noise;
  a.M = (int)M;
  a.o = (int)o;
  a.per_traj = r.val_bytes != M * o * 8;
  a.loglik = st.out[0];
  a.maha = st.out[1];
  return 0;
}

// The timed launch: f.template operator()<d, q>() launches `kernel`<d, q>, one lane per trajectory; `what` heads the refusal.
template <int MaxState, class F>
int datalik_launch(DataLikState& st, int d, int q, F&& f, const char* what, const char* kernel, hipStream_t stream, float* ms,
                   int* n_launches, char* kname, size_t kname_n, std::string& err) {
  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "data log-likelihood: hipEventCreate failed");
  if (!dispatch_dq<kDataLikMaxD, MaxState>(d, q, f)) return pass_fail(err, "%s: no kernel", what);
  if (kname) std::snprintf(kname, kname_n, "odef::%s<%d, %d>", kernel, d, q);
  if (const hipError_t e = st.timer.end(stream, ms); e != hipSuccess) return pass_fail(err, "data log-likelihood: %s", hipGetErrorString(e));
  if (n_launches) *n_launches += 1;  // a running count: a request served from the cache leaves it unchanged
  st.valid = true;
  return 0;
}

}  // namespace odef
