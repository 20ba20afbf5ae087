// Data log-likelihood of noisy observations per trajectory (datalik.h).  One lane per trajectory sweeps the
// filter records of a fixed grid backwards; the time axis is a recursion, so there is one launch, no chunking and no fold.  The
// kernels depend on (d, q) only and are instantiated here once, for the compiled-in and the run-time compiled fields alike.
#include "datalik.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "datalik_kernels.h"

namespace odef {
namespace {

template <int d, int q>
void launch(const DataLikArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((data_loglik_kernel<d, q>), dim3((unsigned)((a.N + kDataLikWave - 1) / kDataLikWave)), dim3(kDataLikWave), 0, st, a);
}

template <int d>
bool launch_order(int q, const DataLikArgs& a, hipStream_t st) {
  switch (q) {
    case 1: launch<d, 1>(a, st); return true;
    case 2: launch<d, 2>(a, st); return true;
    case 3: launch<d, 3>(a, st); return true;
    case 4: launch<d, 4>(a, st); return true;
    case 5:
      if constexpr (d * 6 <= kDataLikMaxState) {
        launch<d, 5>(a, st);
        return true;
      }
      return false;
    default: return false;
  }
}

}  // namespace

bool datalik_has(int d, int q) { return d >= 1 && d <= kDataLikMaxD && q >= 1 && q <= 5 && d * (q + 1) <= kDataLikMaxState; }

int datalik_run(DataLikState& st, const DataLikRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname, size_t kname_n,
                std::string& err) {
  st.valid = false;
  if (!datalik_has(r.d, r.q)) return pass_fail(err, "data log-likelihood: no kernel for (d, q) = (%d, %d)", r.d, r.q);
  const int D = r.d * (r.q + 1), TRI = D * (D + 1) / 2;
  if (r.N < 1 || r.n_save < 2 || (size_t)TRI * (size_t)r.N * sizeof(double) >= (1ull << 31))
    return pass_fail(err, "data log-likelihood: n_traj * D(D+1)/2 * 8 bytes must stay below 2 GiB per save slot; shard the ensemble");
  // M and o follow from the byte counts
  if (r.save_bytes == 0 || r.save_bytes % 8 || r.comp_bytes == 0 || r.comp_bytes % 8 || r.comp_bytes / 8 > (size_t)r.d ||
      r.save_bytes / 8 > (size_t)r.n_save)
    return pass_fail(err, "data log-likelihood: byte counts do not agree: ODEF_L_OBS_SAVE holds %zu bytes (1 .. n_save int64), "
                          "ODEF_L_OBS_COMPONENT %zu (1 .. d int64)", r.save_bytes, r.comp_bytes);
  const size_t M = r.save_bytes / 8, o = r.comp_bytes / 8;
  if (r.noise_bytes != o * 8 || (r.val_bytes != M * o * 8 && r.val_bytes != M * o * (size_t)r.N * 8))
    return pass_fail(err,
                     "data log-likelihood: byte counts do not agree: M = %zu saves and o = %zu components need ODEF_L_OBS_NOISE of %zu bytes "
                     "(got %zu) and ODEF_L_OBS_VALUE of %zu (shared) or %zu (per trajectory) bytes (got %zu)",
                     M, o, o * 8, r.noise_bytes, M * o * 8, M * o * (size_t)r.N * 8, r.val_bytes);
  std::vector<long long> idx(M + o);
  std::vector<double> noise(o);
  hipError_t e = hipMemcpyAsync(idx.data(), r.obs_save, M * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(idx.data() + M, r.obs_comp, o * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(noise.data(), r.obs_noise, o * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return pass_fail(err, "data log-likelihood: %s", hipGetErrorString(e));
  for (size_t j = 0; j < M; ++j)
    if (idx[j] < 0 || idx[j] >= r.n_save || (j > 0 && idx[j] <= idx[j - 1]))
      return pass_fail(err, "data log-likelihood: observed saves must be strictly increasing within 0 .. n_save - 1 = %ld "
                            "(entry %zu is %lld)", r.n_save - 1, j, idx[j]);
  for (size_t a = 0; a < o; ++a)
    if (idx[M + a] < 0 || idx[M + a] >= r.d || (a > 0 && idx[M + a] <= idx[M + a - 1]))
      return pass_fail(err, "data log-likelihood: observed components must be strictly increasing within 0 .. d - 1 = %d "
                            "(entry %zu is %lld)", r.d - 1, a, idx[M + a]);
  for (size_t a = 0; a < o; ++a)
    if (!std::isfinite(noise[a]) || !(noise[a] > 0.0))
      return pass_fail(err, "data log-likelihood: noise variances must be finite and positive (entry %zu is %g)", a, noise[a]);
  for (double*& v : st.out)
    if (!v && hipMalloc((void**)&v, sizeof(double) * r.N) != hipSuccess) {
      (void)hipGetLastError();
      v = nullptr;
      return pass_fail(err, "data log-likelihood: out of device memory");
    }
  DataLikArgs a;
  a.pc = *r.pc;
  a.N = r.N;
  a.n_save = r.n_save;
  a.ptab = r.ptab;
  a.tab_idx = r.tab_idx;
  a.hs = r.hs;
  a.mean = r.mean;
  a.cov = r.cov;
  a.diff = r.diff;
  a.obs_save = (const long long*)r.obs_save;
  a.obs_comp = (const long long*)r.obs_comp;
  a.obs_val = r.obs_val;
  a.obs_noise = r.obs_noise;
  a.M = (int)M;
  a.o = (int)o;
  a.per_traj = r.val_bytes != M * o * 8;
  a.loglik = st.out[0];
  a.maha = st.out[1];
  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "data log-likelihood: hipEventCreate failed");
  bool ok = false;
  switch (r.d) {
    case 1: ok = launch_order<1>(r.q, a, stream); break;
    case 2: ok = launch_order<2>(r.q, a, stream); break;
    case 3: ok = launch_order<3>(r.q, a, stream); break;
    case 4: ok = launch_order<4>(r.q, a, stream); break;
    default: break;
  }
  if (!ok) return pass_fail(err, "data log-likelihood: no kernel");
  if (kname) std::snprintf(kname, kname_n, "odef::data_loglik_kernel<%d, %d>", r.d, r.q);
  if (e = st.timer.end(stream, ms); e != hipSuccess) return pass_fail(err, "data log-likelihood: %s", hipGetErrorString(e));
  if (n_launches) *n_launches += 1;  // a running count: a request served from the cache leaves it unchanged
  st.valid = true;
  return 0;
}

void datalik_free(DataLikState& st) {
  free_device(st.out[0], st.out[1]);
  st.timer.destroy();
  st = DataLikState{};
}

}  // namespace odef
