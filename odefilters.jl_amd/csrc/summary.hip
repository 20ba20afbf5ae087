// Ensemble summary kernels (summary.h).  Two passes over the solution rows of the records, both
// deterministic: no floating-point atomics, a fixed summation order that depends on (N, d, n_t) only.
//
//   pass 1  summary_sums_kernel     per wavefront: count, sum of mu_i (d rows) and of Sigma_i (tri(d) rows)
//           summary_fold_kernel     per time: folds the wavefront partials in wavefront order -> COUNT, MEAN, COV_WITHIN
//   pass 2  summary_centred_kernel  per wavefront: sum of (mu_i - mean)(mu_i - mean)' with the mean of pass 1
//           summary_fold_kernel     -> COV_BETWEEN
//
// Mapping: a workgroup of 256 lanes serves 256 K consecutive trajectories of one time, lane t the trajectories
// base + k 256 + t (k < K): every row read is 512 contiguous bytes per wavefront.  A lane keeps its d K mean entries in its own
// column of an LDS tile [d][K][256] (a run-time indexed private array; no lane reads another lane's column, so there is no
// barrier), sums a row over its K trajectories, and the wavefront reduces that sum with a butterfly of fixed order.  The d + 2
// tri(d) running sums are never live together, so one kernel serves every d <= 32.  K is the largest power of two with
// d K <= 32 (tile <= 64 KiB), halved until the grid holds at least four workgroups per compute unit.
#include "summary.h"

#include <cstdint>

#include "summary_kernels.h"

namespace odef {
namespace {

template <int K>
void launch_sums(const SummaryArgs& a, int n_block, int n_wave, size_t lds, double* part, int* part_cnt, hipStream_t st) {
  hipLaunchKernelGGL(summary_sums_kernel<K>, dim3((unsigned)(n_block * a.n_t)), dim3(kSumBlock), lds, st, a.mean, a.cov,
                     a.retcode, a.N, a.d, a.D, a.TRI, n_wave, part, part_cnt);
}
template <int K>
void launch_centred(const SummaryArgs& a, int n_block, int n_wave, size_t lds, const double* mbar, double* part, hipStream_t st) {
  hipLaunchKernelGGL(summary_centred_kernel<K>, dim3((unsigned)(n_block * a.n_t)), dim3(kSumBlock), lds, st, a.mean, a.retcode,
                     mbar, a.N, a.d, a.D, n_wave, part);
}

}  // namespace

int summary_run(SummaryState& st, SummaryCache& c, const SummaryArgs& a, hipStream_t stream, float* ms, int* n_launches,
                int* walk, std::string& err) {
  c.valid = false;
  if (a.d < 1 || a.d > 32 || a.d > a.D || a.N < 1 || a.n_t < 1) return pass_fail(err, "ensemble summary: built for d <= 32");
  const int tri = a.d * (a.d + 1) / 2, R = a.d + tri;
  if (tri > a.TRI) return pass_fail(err, "ensemble summary: inconsistent record shape");
  int K = 1;
  while (K < 8 && a.d * (K * 2) <= 32) K *= 2;
  auto blocks = [&](int k) { return (long)((a.N + (long)kSumBlock * k - 1) / ((long)kSumBlock * k)); };
  while (K > 1 && blocks(K) * a.n_t < 1024) K /= 2;  // four workgroups per compute unit (256 CUs) before a lane walks further
  const int n_block = (int)blocks(K), n_wave = n_block * (kSumBlock / kWave);
  const size_t lds = (size_t)a.d * K * kSumBlock * sizeof(double);
  if ((long)n_block * a.n_t >= (1l << 31)) return pass_fail(err, "ensemble summary: more than 2^31 workgroups; shard the ensemble");
  if (c.cap_t < a.n_t) {
    free_device(c.count, c.mean, c.within, c.between);
    c.cap_t = 0;
    if (hipMalloc((void**)&c.count, sizeof(long long) * a.n_t) != hipSuccess ||
        hipMalloc((void**)&c.mean, sizeof(double) * a.n_t * a.d) != hipSuccess ||
        hipMalloc((void**)&c.within, sizeof(double) * a.n_t * tri) != hipSuccess ||
        hipMalloc((void**)&c.between, sizeof(double) * a.n_t * tri) != hipSuccess) {
      (void)hipGetLastError();
      return pass_fail(err, "ensemble summary: out of device memory");
    }
    c.cap_t = a.n_t;
  }
  if (!grow((void**)&st.part, &st.part_cap, sizeof(double) * (size_t)a.n_t * n_wave * R) ||
      !grow((void**)&st.part_cnt, &st.cnt_cap, sizeof(int) * (size_t)a.n_t * n_wave))
    return pass_fail(err, "ensemble summary: out of device memory");
  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "ensemble summary: hipEventCreate failed");
  switch (K) {
    case 8: launch_sums<8>(a, n_block, n_wave, lds, st.part, st.part_cnt, stream); break;
    case 4: launch_sums<4>(a, n_block, n_wave, lds, st.part, st.part_cnt, stream); break;
    case 2: launch_sums<2>(a, n_block, n_wave, lds, st.part, st.part_cnt, stream); break;
    default: launch_sums<1>(a, n_block, n_wave, lds, st.part, st.part_cnt, stream); break;
  }
  hipLaunchKernelGGL(summary_fold_kernel, dim3((unsigned)a.n_t), dim3(kWave), 0, stream, (const double*)st.part,
                     (const int*)st.part_cnt, n_wave, R, a.d, c.count, c.mean, c.within);
  switch (K) {
    case 8: launch_centred<8>(a, n_block, n_wave, lds, c.mean, st.part, stream); break;
    case 4: launch_centred<4>(a, n_block, n_wave, lds, c.mean, st.part, stream); break;
    case 2: launch_centred<2>(a, n_block, n_wave, lds, c.mean, st.part, stream); break;
    default: launch_centred<1>(a, n_block, n_wave, lds, c.mean, st.part, stream); break;
  }
  hipLaunchKernelGGL(summary_fold_kernel, dim3((unsigned)a.n_t), dim3(kWave), 0, stream, (const double*)st.part, (const int*)nullptr,
                     n_wave, tri, tri, c.count, c.between, (double*)nullptr);
  if (const hipError_t e = st.timer.end(stream, ms); e != hipSuccess)
    return pass_fail(err, "ensemble summary: %s", hipGetErrorString(e));
  if (n_launches) *n_launches = 4;
  c.n_t = a.n_t;
  c.valid = true;
  if (walk) *walk = K;
  return 0;
}

void summary_free(SummaryState& st) {
  for (SummaryCache& c : st.src) free_device(c.count, c.mean, c.within, c.between);
  free_device(st.part, st.part_cnt);
  st.timer.destroy();
  st = SummaryState{};
}

}  // namespace odef
