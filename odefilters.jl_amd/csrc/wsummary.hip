// Weighted ensemble summary kernels (wsummary.h).  The two passes of summary.hip with a weight per trajectory,
// both deterministic: no floating-point atomics, a fixed summation order that depends on (N, d, n_t) only.
//
//   weights wsummary_max_kernel      L = max of the finite log-weights of the successful trajectories (integer atomicMax on
//                                    order-preserving keys: a maximum does not depend on the order)
//           wsummary_weights_kernel  v_i = exp(l_i - L) [N]: one exp per trajectory and request, none per time
//   pass 1  wsummary_sums_kernel     per wavefront: count, sums of v, v^2, v mu_i (d rows) and v Sigma_i (tri(d) rows)
//           wsummary_fold_kernel     per time: folds the partials in wavefront order, divides by Z = sum v
//                                    -> COUNT, MEAN, COV_WITHIN, ESS, LOG_EVIDENCE
//   pass 2  wsummary_centred_kernel  per wavefront: sum of v (mu_i - mean)(mu_i - mean)' with the mean of pass 1
//           wsummary_fold_centred_kernel -> COV_BETWEEN
//
// Mapping, K and the LDS tile [d][K][256]: those of summary.hip.  The row v [N] is read once per time and pass (512 contiguous
// bytes per wavefront, like every record row) and stays in cache across the times.
#include "wsummary.h"

#include <cstdint>

#include "wsummary_kernels.h"

namespace odef {
namespace {

template <int K>
void launch_sums(const WSummaryArgs& a, const double* v, int n_block, int n_wave, size_t lds, double* part, int* part_cnt,
                 hipStream_t st) {
  hipLaunchKernelGGL(wsummary_sums_kernel<K>, dim3((unsigned)(n_block * a.n_t)), dim3(kWBlock), lds, st, a.mean, a.cov, a.retcode, v,
                     a.N, a.d, a.D, a.TRI, n_wave, part, part_cnt);
}
template <int K>
void launch_centred(const WSummaryArgs& a, const double* v, int n_block, int n_wave, size_t lds, const double* mbar, double* part,
                    hipStream_t st) {
  hipLaunchKernelGGL(wsummary_centred_kernel<K>, dim3((unsigned)(n_block * a.n_t)), dim3(kWBlock), lds, st, a.mean, a.retcode, v,
                     mbar, a.N, a.d, a.D, n_wave, part);
}

}  // namespace

int wsummary_run(WSummaryState& st, WSummaryCache& c, const WSummaryArgs& a, hipStream_t stream, float* ms, int* n_launches,
                 int* walk, std::string& err) {
  c.valid = false;
  if (a.d < 1 || a.d > 32 || a.d > a.D || a.N < 1 || a.n_t < 1) return pass_fail(err, "weighted ensemble summary: built for d <= 32");
  const int tri = a.d * (a.d + 1) / 2, R = 2 + a.d + tri;
  if (tri > a.TRI) return pass_fail(err, "weighted ensemble summary: inconsistent record shape");
  int K = 1;
  while (K < 8 && a.d * (K * 2) <= 32) K *= 2;
  auto blocks = [&](int k) { return (long)((a.N + (long)kWBlock * k - 1) / ((long)kWBlock * k)); };
  while (K > 1 && blocks(K) * a.n_t < 1024) K /= 2;  // four workgroups per compute unit (256 CUs) before a lane walks further
  const int n_block = (int)blocks(K), n_wave = n_block * (kWBlock / kWWave);
  const size_t lds = (size_t)a.d * K * kWBlock * sizeof(double);
  if ((long)n_block * a.n_t >= (1l << 31) || blocks(1) >= (1l << 31))
    return pass_fail(err, "weighted ensemble summary: more than 2^31 workgroups; shard the ensemble");
  if (!grow((void**)&c.count, &c.count_cap, sizeof(long long) * (size_t)a.n_t) ||
      !grow((void**)&c.mean, &c.mean_cap, sizeof(double) * (size_t)a.n_t * a.d) ||
      !grow((void**)&c.within, &c.within_cap, sizeof(double) * (size_t)a.n_t * tri) ||
      !grow((void**)&c.between, &c.between_cap, sizeof(double) * (size_t)a.n_t * tri) ||
      !grow((void**)&c.logev, &c.logev_cap, sizeof(double) * (size_t)a.n_t) ||
      !grow((void**)&c.ess, &c.ess_cap, sizeof(double) * (size_t)a.n_t) ||
      !grow(&st.key, &st.key_cap, sizeof(unsigned long long)) || !grow(&st.v, &st.v_cap, sizeof(double) * (size_t)a.N) ||
      !grow(&st.zsum, &st.zsum_cap, sizeof(double) * (size_t)a.n_t) ||
      !grow(&st.part, &st.part_cap, sizeof(double) * (size_t)a.n_t * n_wave * R) ||
      !grow(&st.part_cnt, &st.cnt_cap, sizeof(int) * (size_t)a.n_t * n_wave))
    return pass_fail(err, "weighted ensemble summary: out of device memory");
  unsigned long long* key = (unsigned long long*)st.key;
  double* v = (double*)st.v;
  double* zsum = (double*)st.zsum;
  double* part = (double*)st.part;
  int* part_cnt = (int*)st.part_cnt;
  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "weighted ensemble summary: hipEventCreate failed");
  if (const hipError_t e = hipMemsetAsync(key, 0, sizeof(unsigned long long), stream); e != hipSuccess) {
    (void)st.timer.end(stream, nullptr);
    return pass_fail(err, "weighted ensemble summary: %s", hipGetErrorString(e));
  }
  const long n_flat = blocks(1);
  hipLaunchKernelGGL(wsummary_max_kernel, dim3((unsigned)(n_flat < 1024 ? n_flat : 1024)), dim3(kWBlock), 0, stream, a.logw, a.retcode,
                     a.N, key);
  hipLaunchKernelGGL(wsummary_weights_kernel, dim3((unsigned)n_flat), dim3(kWBlock), 0, stream, a.logw, a.retcode, a.N,
                     (const unsigned long long*)key, v);
  switch (K) {
    case 8: launch_sums<8>(a, v, n_block, n_wave, lds, part, part_cnt, stream); break;
    case 4: launch_sums<4>(a, v, n_block, n_wave, lds, part, part_cnt, stream); break;
    case 2: launch_sums<2>(a, v, n_block, n_wave, lds, part, part_cnt, stream); break;
    default: launch_sums<1>(a, v, n_block, n_wave, lds, part, part_cnt, stream); break;
  }
  hipLaunchKernelGGL(wsummary_fold_kernel, dim3((unsigned)a.n_t), dim3(kWWave), 0, stream, (const double*)part, (const int*)part_cnt,
                     n_wave, a.d, tri, (const unsigned long long*)key, c.count, zsum, c.mean, c.within, c.logev, c.ess);
  switch (K) {
    case 8: launch_centred<8>(a, v, n_block, n_wave, lds, c.mean, part, stream); break;
    case 4: launch_centred<4>(a, v, n_block, n_wave, lds, c.mean, part, stream); break;
    case 2: launch_centred<2>(a, v, n_block, n_wave, lds, c.mean, part, stream); break;
    default: launch_centred<1>(a, v, n_block, n_wave, lds, c.mean, part, stream); break;
  }
  hipLaunchKernelGGL(wsummary_fold_centred_kernel, dim3((unsigned)a.n_t), dim3(kWWave), 0, stream, (const double*)part, n_wave, tri,
                     (const double*)zsum, c.between);
  if (const hipError_t e = st.timer.end(stream, ms); e != hipSuccess)
    return pass_fail(err, "weighted ensemble summary: %s", hipGetErrorString(e));
  if (n_launches) *n_launches = 6;
  c.n_t = a.n_t;
  c.valid = true;
  if (walk) *walk = K;
  return 0;
}

void wsummary_free(WSummaryState& st) {
  for (WSummaryCache& c : st.src) free_device(c.count, c.mean, c.within, c.between, c.logev, c.ess);
  free_device(st.key, st.v, st.zsum, st.part, st.part_cnt);
  st.timer.destroy();
  st = WSummaryState{};
}

}  // namespace odef
