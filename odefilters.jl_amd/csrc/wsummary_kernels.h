// Device source of the weighted ensemble-summary reduction (wsummary.hip launches it; tests/emul/emul_wsummary.cpp builds the same
// text for the host, one thread per lane, to check it without a GPU).  Includes nothing: the including file provides the HIP
// runtime and exp / log.  The wave butterfly and the loading of the means are those of summary_kernels.h, copied: including
// that header would define its fold kernel in a second translation unit.
#pragma once

// the dynamic LDS tile [d][K][256] of a workgroup (the host emulation points it at a plain array)
#ifndef ODEF_WSUMMARY_TILE
#define ODEF_WSUMMARY_TILE extern __shared__ double tile[]
#endif

namespace odef {
namespace {

constexpr int kWBlock = 256;  // lanes per workgroup
constexpr int kWWave = 64;
constexpr double kWMaxDouble = 1.79769313486231570815e308;

__device__ __forceinline__ double wsum_wave(double v) {
#pragma unroll
  for (int m = kWWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWWave);
  return v;
}

__device__ __forceinline__ bool wsum_finite(double x) { return __builtin_fabs(x) <= kWMaxDouble; }

// Order-preserving key of a finite double (a < b <=> key(a) < key(b)); no finite double has key 0, which stands for "nobody".
__device__ __forceinline__ unsigned long long wsum_key(double x) {
  const unsigned long long b = (unsigned long long)__builtin_bit_cast(long long, x);
  return (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ double wsum_unkey(unsigned long long k) {
  if (k == 0) return __builtin_nan("");
  const unsigned long long b = (k >> 63) ? k & ~(1ull << 63) : ~k;
  return __builtin_bit_cast(double, (long long)b);
}

// Loads the d mean entries of the lane's K trajectories of time s into its LDS column and their weights into w; returns the
// inclusion mask (bit k: trajectory base + k 256 + t exists, finished with ODEF_RET_SUCCESS, has d finite mean entries at this
// time and a finite log-weight, which v marks by v >= 0).  w[k] is 0 for a trajectory that is not included.
template <int K>
__device__ __forceinline__ unsigned wsum_load(const double* __restrict__ mean_s /* record s: [D][N] */, const int* __restrict__ retcode,
                                              const double* __restrict__ v /* [N] */, long N, int d, long base,
                                              double* __restrict__ tile, long (&idx)[K], double (&w)[K]) {
  const int t = threadIdx.x;
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long i = base + (long)k * kWBlock + t;
    idx[k] = i < N ? i : N - 1;  // a lane past the end reads the last trajectory and drops it
    w[k] = v[idx[k]];
    if (i < N && retcode[idx[k]] == 0 && w[k] >= 0.0) mask |= 1u << k;
  }
  for (int a = 0; a < d; ++a) {
    double x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = mean_s[(size_t)a * N + idx[k]];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!wsum_finite(x[k])) mask &= ~(1u << k);  // NaN or Inf
      tile[((size_t)a * K + k) * kWBlock + t] = x[k];
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = (mask >> k & 1u) ? w[k] : 0.0;
  return mask;
}

}  // namespace

// L = max of the finite log-weights of the trajectories that finished with ODEF_RET_SUCCESS, as an order-preserving key in *key
// (zeroed before the launch).  A maximum does not depend on the order, so the integer atomic keeps the result deterministic.
__global__ __launch_bounds__(kWBlock) void wsummary_max_kernel(const double* __restrict__ logw, const int* __restrict__ retcode, long N,
                                                               unsigned long long* __restrict__ key) {
  double m = -__builtin_inf();
  for (long i = (long)blockIdx.x * kWBlock + threadIdx.x; i < N; i += (long)gridDim.x * kWBlock) {
    const double l = logw[i];
    if (retcode[i] == 0 && wsum_finite(l) && l > m) m = l;
  }
#pragma unroll
  for (int s = kWWave / 2; s >= 1; s >>= 1) {
    const double o = __shfl_xor(m, s, kWWave);
    m = o > m ? o : m;
  }
  if (threadIdx.x % kWWave == 0 && wsum_finite(m)) atomicMax(key, wsum_key(m));
}

// v_i = exp(l_i - L) for a finite l_i of a trajectory that finished with ODEF_RET_SUCCESS, 0 for a finite l_i of any other, and
// -1 for an l_i that is not finite: the mark by which the two passes leave that trajectory out.
__global__ __launch_bounds__(kWBlock) void wsummary_weights_kernel(const double* __restrict__ logw, const int* __restrict__ retcode,
                                                                   long N, const unsigned long long* __restrict__ key,
                                                                   double* __restrict__ v) {
  const long i = (long)blockIdx.x * kWBlock + threadIdx.x;
  if (i >= N) return;
  const double L = wsum_unkey(*key), l = logw[i];
  v[i] = !wsum_finite(l) ? -1.0 : retcode[i] == 0 ? exp(l - L) : 0.0;
}

// Pass 1, per wavefront: the count and the sums of v, v^2, v mu (d rows) and v Sigma (tri(d) rows) over the included.
template <int K>
__global__ __launch_bounds__(kWBlock) void wsummary_sums_kernel(const double* __restrict__ mean, const double* __restrict__ cov,
                                                                const int* __restrict__ retcode, const double* __restrict__ v,
                                                                long N, int d, int D, int TRI, int n_wave,
                                                                double* __restrict__ part, int* __restrict__ part_cnt) {
  ODEF_WSUMMARY_TILE;
  const int n_block = n_wave / (kWBlock / kWWave), blk = blockIdx.x % n_block;
  const long s = blockIdx.x / n_block;
  const long base = (long)blk * (kWBlock * K);
  const int t = threadIdx.x, lane = t % kWWave;
  const int wave = blk * (kWBlock / kWWave) + t / kWWave;
  const int tri = d * (d + 1) / 2, R = 2 + d + tri;
  long idx[K];
  double w[K];
  const unsigned mask = wsum_load<K>(mean + (size_t)s * D * N, retcode, v, N, d, base, tile, idx, w);
  double* out = part + ((size_t)s * n_wave + wave) * R;
  {
    int n = __popc(mask);
#pragma unroll
    for (int m = kWWave / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, kWWave);
    if (lane == 0) part_cnt[(size_t)s * n_wave + wave] = n;
  }
  {
    double z = 0.0, z2 = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      z += w[k];
      z2 += w[k] * w[k];
    }
    z = wsum_wave(z);
    z2 = wsum_wave(z2);
    if (lane == 0) {
      out[0] = z;
      out[1] = z2;
    }
  }
  for (int a = 0; a < d; ++a) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double x = tile[((size_t)a * K + k) * kWBlock + t];
      acc += (mask >> k & 1u) ? w[k] * x : 0.0;  // (the mean of a dropped trajectory may be NaN: 0 NaN is not 0)
    }
    acc = wsum_wave(acc);
    if (lane == 0) out[2 + a] = acc;
  }
  const double* cov_s = cov + (size_t)s * TRI * N;
  for (int p = 0; p < tri; ++p) {  // the first tri(d) packed rows are the d x d solution block
    double x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = cov_s[(size_t)p * N + idx[k]];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) acc += (mask >> k & 1u) ? w[k] * x[k] : 0.0;
    acc = wsum_wave(acc);
    if (lane == 0) out[2 + d + p] = acc;
  }
}

// Folds the pass-1 partials of one time in wavefront order: COUNT, Z (kept in zsum for pass 2), MEAN and COV_WITHIN as sums
// over Z, ESS = Z^2 / sum v^2 and LOG_EVIDENCE = L + log Z - log n.  n = 0 and Z = 0 take the IEEE route: 0 / 0 is NaN,
// log 0 is -inf.
__global__ void wsummary_fold_kernel(const double* __restrict__ part, const int* __restrict__ part_cnt, int n_wave, int d, int tri,
                                     const unsigned long long* __restrict__ key, long long* __restrict__ count,
                                     double* __restrict__ zsum, double* __restrict__ m, double* __restrict__ within,
                                     double* __restrict__ logev, double* __restrict__ ess) {
  const long s = blockIdx.x;
  const int R = 2 + d + tri;
  double Z = 0.0;
  for (int w = 0; w < n_wave; ++w) Z += part[((size_t)s * n_wave + w) * R];
  for (int r = threadIdx.x; r < d + tri; r += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < n_wave; ++w) acc += part[((size_t)s * n_wave + w) * R + 2 + r];
    const double q = acc / Z;
    if (r < d) m[(size_t)s * d + r] = q;
    else within[(size_t)s * tri + (r - d)] = q;
  }
  if (threadIdx.x == 0) {
    long long n = 0;
    double Z2 = 0.0;
    for (int w = 0; w < n_wave; ++w) {
      n += part_cnt[(size_t)s * n_wave + w];
      Z2 += part[((size_t)s * n_wave + w) * R + 1];
    }
    count[s] = n;
    zsum[s] = Z;
    ess[s] = Z * Z / Z2;
    logev[s] = wsum_unkey(*key) + log(Z) - log((double)n);
  }
}

// Pass 2, per wavefront: the sum of v (mu - m)(mu - m)' with the m of pass 1, centred before it is squared.
template <int K>
__global__ __launch_bounds__(kWBlock) void wsummary_centred_kernel(const double* __restrict__ mean, const int* __restrict__ retcode,
                                                                   const double* __restrict__ v,
                                                                   const double* __restrict__ mbar /* [n_t][d] */, long N, int d,
                                                                   int D, int n_wave, double* __restrict__ part) {
  ODEF_WSUMMARY_TILE;
  const int n_block = n_wave / (kWBlock / kWWave), blk = blockIdx.x % n_block;
  const long s = blockIdx.x / n_block;
  const long base = (long)blk * (kWBlock * K);
  const int t = threadIdx.x, lane = t % kWWave;
  const int wave = blk * (kWBlock / kWWave) + t / kWWave;
  const int tri = d * (d + 1) / 2;
  long idx[K];
  double w[K];
  const unsigned mask = wsum_load<K>(mean + (size_t)s * D * N, retcode, v, N, d, base, tile, idx, w);
  for (int a = 0; a < d; ++a) {  // centre before squaring; a dropped trajectory contributes exact zeros
    const double m = mbar[(size_t)s * d + a];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double* e = &tile[((size_t)a * K + k) * kWBlock + t];
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
        acc += w[k] * (tile[((size_t)a * K + k) * kWBlock + t] * tile[((size_t)b * K + k) * kWBlock + t]);
      acc = wsum_wave(acc);
      if (lane == 0) out[p] = acc;
    }
}

// Folds the pass-2 partials of one time in wavefront order and divides by the Z of pass 1: COV_BETWEEN.
__global__ void wsummary_fold_centred_kernel(const double* __restrict__ part, int n_wave, int tri, const double* __restrict__ zsum,
                                             double* __restrict__ between) {
  const long s = blockIdx.x;
  const double Z = zsum[s];
  for (int r = threadIdx.x; r < tri; r += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < n_wave; ++w) acc += part[((size_t)s * n_wave + w) * tri + r];
    between[(size_t)s * tri + r] = acc / Z;
  }
}

}  // namespace odef
