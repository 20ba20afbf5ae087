// Ensemble quantile kernels (quantiles.h).  Exact radix selection of 2 P ranks per (time, component) row on
// order-preserving 64-bit keys; integer counts only, so two runs agree bit for bit whatever the order of the atomics.
//
// The times are worked in slabs of T; per slab
//   quantile_init_kernel     resets count, key range and histograms
//   quantile_mask_kernel     one pass over the d rows of every time: inclusion mask, count, smallest / largest key per row
//   quantile_start_kernel    per row: the width kmax - kmin of the offset keys k - kmin says where the digit passes start
//   up to 8 digit passes, most significant first, as many as the widest row of the slab needs (read back: one int)
//     quantile_hist_kernel   (row, chunk): 8-bit digit histogram per rank in LDS, then integer atomics into the row's histograms
//     quantile_select_kernel per row: prefix sums, the bin of each remaining rank extends its prefix
//   quantile_finish_kernel   keys back to doubles, Q = x_lo + g (x_hi - x_lo)
// A row is read once by the mask pass and once per digit pass it still needs: at most 1 + 8 times.
//
// Mapping: a workgroup of 256 lanes serves `iters` 256 consecutive trajectories of one row, lane t the trajectories
// base + j 256 + t, so every read is 512 contiguous bytes per wavefront.  iters is 8, halved until a slab gives 1024 workgroups.
// T is bounded by T d <= 1024 rows (the histograms of a slab stay under 16 MiB); slabs sized to the last-level cache were
// measured and were not faster.  The pass synchronises the stream once per slab, for the read-back.
#include "quantiles.h"

#include <cstdint>

#include "quantile_kernels.h"

namespace odef {

int quantiles_run(QuantileState& st, QuantileCache& c, const QuantileArgs& a, hipStream_t stream, float* ms, int* n_launches,
                  std::string& err) {
  c.valid = false;
  if (a.d < 1 || a.d > kQMaxDim || a.d > a.D) return pass_fail(err, "ensemble quantiles: built for d <= 32");
  if (a.P < 1 || a.P > kQMaxProbs) return pass_fail(err, "ensemble quantiles: 1 <= P <= 8 probabilities");
  if (a.N < 1 || a.n_t < 1) return pass_fail(err, "ensemble quantiles: no records");
  if (a.N >= (1l << 31)) return pass_fail(err, "ensemble quantiles: more than 2^31 trajectories; shard the ensemble");
  const int R = 2 * a.P, W = (int)((a.N + kQWave - 1) / kQWave);
  long T = 1024 / a.d;
  if (T > a.n_t) T = a.n_t;
  int iters = 8;
  auto chunks = [&](int k) { return (long)((a.N + (long)kQBlock * k - 1) / ((long)kQBlock * k)); };
  while (iters > 1 && chunks(iters) * T < 1024) iters /= 2;
  const long n_chunk = chunks(iters);
  const long rows_max = T * a.d;
  if (rows_max * n_chunk >= (1l << 31)) return pass_fail(err, "ensemble quantiles: more than 2^31 workgroups; shard the ensemble");
  QuantileProbs probs{};
  for (int p = 0; p < a.P; ++p) probs.p[p] = a.probs[p];

  if (!grow((void**)&c.count, &c.count_cap, sizeof(long long) * (size_t)a.n_t) ||
      !grow((void**)&c.q, &c.q_cap, sizeof(double) * (size_t)a.n_t * a.P * a.d) ||
      !grow(&st.mask, &st.mask_cap, sizeof(qkey_t) * (size_t)T * W) ||
      !grow(&st.range, &st.range_cap, sizeof(qkey_t) * 2 * (size_t)rows_max) ||
      !grow(&st.rows, &st.rows_cap, sizeof(int) * ((size_t)rows_max + 1)) ||
      !grow(&st.ranks, &st.ranks_cap, (sizeof(qkey_t) + sizeof(unsigned) + sizeof(int)) * (size_t)rows_max * R) ||
      !grow(&st.hist, &st.hist_cap, sizeof(unsigned) * (size_t)rows_max * R * kQBins))
    return pass_fail(err, "ensemble quantiles: out of device memory");
  qkey_t* mask = (qkey_t*)st.mask;
  qkey_t* kmin = (qkey_t*)st.range;
  qkey_t* kmax = kmin + rows_max;
  int* low = (int*)st.rows;
  int* max_low = low + rows_max;
  qkey_t* prefix = (qkey_t*)st.ranks;
  unsigned* rem = (unsigned*)(prefix + rows_max * R);
  int* owner = (int*)(rem + rows_max * R);
  unsigned* hist = (unsigned*)st.hist;

  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "ensemble quantiles: hipEventCreate failed");
  // a failure inside the pass closes the timer's event pair before it returns
  auto fail_in_pass = [&](const char* what) {
    (void)st.timer.end(stream, nullptr);
    return pass_fail(err, "ensemble quantiles: %s", what);
  };
  int launches = 0;
  for (long s0 = 0; s0 < a.n_t; s0 += T) {
    const long Ts = a.n_t - s0 < T ? a.n_t - s0 : T;
    const long rows = Ts * a.d;
    const double* mean = a.mean + (size_t)s0 * a.D * a.N;
    long long* count = c.count + s0;
    hipLaunchKernelGGL(quantile_init_kernel, dim3((unsigned)rows), dim3(kQBlock), 0, stream, a.d, R, count, kmin, kmax, hist,
                       max_low);
    hipLaunchKernelGGL(quantile_mask_kernel, dim3((unsigned)(Ts * n_chunk)), dim3(kQBlock), 0, stream, mean, a.retcode, a.N, a.d,
                       a.D, W, (int)n_chunk, iters, mask, count, kmin, kmax);
    hipLaunchKernelGGL(quantile_start_kernel, dim3((unsigned)((rows + kQBlock - 1) / kQBlock)), dim3(kQBlock), 0, stream, rows,
                       a.d, a.P, probs, (const long long*)count, (const qkey_t*)kmin, (const qkey_t*)kmax, low, prefix, rem,
                       owner, max_low);
    launches += 3;
    int widest = 0;  // the unselected key bits of the widest row: the slab needs ceil(widest / 8) digit passes
    hipError_t e = hipMemcpyAsync(&widest, max_low, sizeof(int), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail_in_pass(hipGetErrorString(e));
    if (widest < 0 || widest > 64) return fail_in_pass("inconsistent key range");
    const int passes = (widest + 7) / 8;
    for (int k = 0; k < passes; ++k) {
      hipLaunchKernelGGL(quantile_hist_kernel, dim3((unsigned)(rows * n_chunk)), dim3(kQBlock), 0, stream, mean,
                         (const qkey_t*)mask, a.N, a.d, a.D, W, (int)n_chunk, iters, R, (const qkey_t*)kmin, (const int*)low, (const qkey_t*)prefix,
                         (const int*)owner, hist);
      hipLaunchKernelGGL(quantile_select_kernel, dim3((unsigned)rows), dim3(kQBlock), 0, stream, R, low, prefix, rem, owner, hist);
    }
    hipLaunchKernelGGL(quantile_finish_kernel, dim3((unsigned)((rows * a.P + kQBlock - 1) / kQBlock)), dim3(kQBlock), 0, stream,
                       rows, a.d, a.P, probs, (const long long*)count, (const qkey_t*)kmin, (const qkey_t*)prefix, c.q + (size_t)s0 * a.P * a.d);
    launches += 2 * passes + 1;
  }
  if (const hipError_t e = st.timer.end(stream, ms); e != hipSuccess)
    return pass_fail(err, "ensemble quantiles: %s", hipGetErrorString(e));
  if (n_launches) *n_launches = launches;
  c.n_t = a.n_t;
  c.P = a.P;
  c.valid = true;
  return 0;
}

void quantiles_free(QuantileState& st) {
  for (QuantileCache& c : st.src) free_device(c.count, c.q);
  free_device(st.mask, st.range, st.rows, st.ranks, st.hist);
  st.timer.destroy();
  st = QuantileState{};
}

}  // namespace odef
