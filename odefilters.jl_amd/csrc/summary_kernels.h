// Device source of the ensemble-summary reduction (summary.hip launches it; tests/emul/emul_summary.cpp builds the same text for
// the host, one thread per lane, to check it without a GPU).  Includes nothing: the including file provides the HIP runtime.
#pragma once

// the dynamic LDS tile [d][K][256] of a workgroup (the host emulation points it at a plain array)
#ifndef ODEF_SUMMARY_TILE
#define ODEF_SUMMARY_TILE extern __shared__ double tile[]
#endif

namespace odef {
namespace {

constexpr int kSumBlock = 256;  // lanes per workgroup
constexpr int kWave = 64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// Loads the d mean entries of the lane's K trajectories of time s into its LDS column and returns the inclusion mask (bit k:
// trajectory base + k 256 + t exists, finished with ODEF_RET_SUCCESS and has d finite mean entries at this time).
template <int K>
__device__ __forceinline__ unsigned load_means(const double* __restrict__ mean_s /* record s: [D][N] */, const int* __restrict__ retcode,
                                               long N, int d, long base, double* __restrict__ tile, long (&idx)[K]) {
  const int t = threadIdx.x;
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long i = base + (long)k * kSumBlock + t;
    idx[k] = i < N ? i : N - 1;  // a lane past the end reads the last trajectory and drops it
    if (i < N && retcode[idx[k]] == 0) mask |= 1u << k;
  }
  for (int a = 0; a < d; ++a) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = mean_s[(size_t)a * N + idx[k]];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!(__builtin_fabs(v[k]) <= 1.79769313486231570815e308)) mask &= ~(1u << k);  // NaN or Inf
      tile[((size_t)a * K + k) * kSumBlock + t] = v[k];
    }
  }
  return mask;
}

}  // namespace

template <int K>
__global__ __launch_bounds__(kSumBlock) void summary_sums_kernel(const double* __restrict__ mean, const double* __restrict__ cov,
                                                                 const int* __restrict__ retcode, long N, int d, int D, int TRI,
                                                                 int n_wave, double* __restrict__ part, int* __restrict__ part_cnt) {
  ODEF_SUMMARY_TILE;
  const int n_block = n_wave / (kSumBlock / kWave), blk = blockIdx.x % n_block;
  const long s = blockIdx.x / n_block;
  const long base = (long)blk * (kSumBlock * K);
  const int t = threadIdx.x, lane = t % kWave;
  const int wave = blk * (kSumBlock / kWave) + t / kWave;
  const int tri = d * (d + 1) / 2, R = d + tri;
  long idx[K];
  const unsigned mask = load_means<K>(mean + (size_t)s * D * N, retcode, N, d, base, tile, idx);
  double* out = part + ((size_t)s * n_wave + wave) * R;
  {
    int n = __popc(mask);
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, kWave);
    if (lane == 0) part_cnt[(size_t)s * n_wave + wave] = n;
  }
  for (int a = 0; a < d; ++a) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double v = tile[((size_t)a * K + k) * kSumBlock + t];
      acc += (mask >> k & 1u) ? v : 0.0;
    }
    acc = wave_sum(acc);
    if (lane == 0) out[a] = acc;
  }
  const double* cov_s = cov + (size_t)s * TRI * N;
  for (int p = 0; p < tri; ++p) {  // the first tri(d) packed rows are the d x d solution block
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = cov_s[(size_t)p * N + idx[k]];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) acc += (mask >> k & 1u) ? v[k] : 0.0;
    acc = wave_sum(acc);
    if (lane == 0) out[d + p] = acc;
  }
}

template <int K>
__global__ __launch_bounds__(kSumBlock) void summary_centred_kernel(const double* __restrict__ mean, const int* __restrict__ retcode,
                                                                    const double* __restrict__ mbar /* [n_t][d] */, long N, int d,
                                                                    int D, int n_wave, double* __restrict__ part) {
  ODEF_SUMMARY_TILE;
  const int n_block = n_wave / (kSumBlock / kWave), blk = blockIdx.x % n_block;
  const long s = blockIdx.x / n_block;
  const long base = (long)blk * (kSumBlock * K);
  const int t = threadIdx.x, lane = t % kWave;
  const int wave = blk * (kSumBlock / kWave) + t / kWave;
  const int tri = d * (d + 1) / 2;
  long idx[K];
  const unsigned mask = load_means<K>(mean + (size_t)s * D * N, retcode, N, d, base, tile, idx);
  for (int a = 0; a < d; ++a) {  // centre before squaring; a dropped trajectory contributes exact zeros
    const double m = mbar[(size_t)s * d + a];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double* e = &tile[((size_t)a * K + k) * kSumBlock + t];
      *e = (mask >> k & 1u) ? *e - m : 0.0;
    }
  }
  double* out = part + ((size_t)s * n_wave + wave) * tri;
  int p = 0;
  for (int a = 0; a < d; ++a)
    for (int b = 0; b <= a; ++b, ++p) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k)
        acc += tile[((size_t)a * K + k) * kSumBlock + t] * tile[((size_t)b * K + k) * kSumBlock + t];
      acc = wave_sum(acc);
      if (lane == 0) out[p] = acc;
    }
}

// Folds the wavefront partials of one time in wavefront order and divides by the count: rows < RA go to outA [n_t][RA], the
// others to outB [n_t][R - RA].  part_cnt != nullptr: the counts are folded too and written to count; else count is read.
__global__ void summary_fold_kernel(const double* __restrict__ part, const int* __restrict__ part_cnt, int n_wave, int R, int RA,
                                    long long* __restrict__ count, double* __restrict__ outA, double* __restrict__ outB) {
  const long s = blockIdx.x;
  long long n = 0;
  if (part_cnt) {
    for (int w = 0; w < n_wave; ++w) n += part_cnt[(size_t)s * n_wave + w];
  } else {
    n = count[s];
  }
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < n_wave; ++w) acc += part[((size_t)s * n_wave + w) * R + r];
    const double v = n > 0 ? acc / (double)n : __builtin_nan("");
    if (r < RA) outA[(size_t)s * RA + r] = v;
    else outB[(size_t)s * (R - RA) + (r - RA)] = v;
  }
  if (part_cnt && threadIdx.x == 0) count[s] = n;
}

}  // namespace odef
