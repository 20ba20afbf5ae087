// Device source of the ensemble quantiles (quantiles.hip launches it; tests/emul/emul_quantiles.cpp builds the same text for the
// host, one thread per lane of a workgroup, to check it without a GPU).  Includes nothing: the including file provides the HIP
// runtime.  Exact radix selection on order-preserving 64-bit keys: every count is an integer, no floating-point atomic appears.
//
// One SLAB of T consecutive times is worked at once; a ROW is one (time, component) pair of the slab, rw = ts d + a, and holds the
// N values mean[ts][a][0..N-1].  R = 2 P ranks are selected per row (lo and hi of every probability).  Workspace of a slab:
//   mask    [T][W]            inclusion bits of the trajectories, W = ceil(N / 64)
//   kmin / kmax [T d]         smallest / largest key of the included values of a row
//   low     [T d]             number of low key bits of the row that are not selected yet (0: the row is finished)
//   prefix  [T d][R]          the selected high bits of every rank's offset key k - kmin (the low `low` bits are zero)
//   rem     [T d][R]          the rank that remains among the keys that share the prefix
//   owner   [T d][R]          the first rank with the same prefix: ranks that share a prefix share one histogram
//   hist    [T d][R][256]     digit counts of the keys under the prefix of rank r (filled for owners only, zero between passes)
#pragma once

namespace odef {
namespace {

constexpr int kQBlock = 256;  // lanes per workgroup
constexpr int kQWave = 64;
constexpr int kQBins = 256;     // 8-bit digits
constexpr int kQMaxProbs = 8;
constexpr int kQMaxRanks = 2 * kQMaxProbs;
constexpr int kQMaxDim = 32;
constexpr int kQMaxIters = 32;  // a lane walks at most this many trajectories of a chunk (one bit each in an unsigned)

typedef unsigned long long qkey_t;

struct QuantileProbs {
  double p[kQMaxProbs];
};

// order-preserving key of a double: negative values complement, the others set the top bit (-0 sorts below +0)
__device__ __forceinline__ qkey_t quantile_key(double v) {
  const qkey_t b = __builtin_bit_cast(qkey_t, v);
  return (b >> 63) ? ~b : (b | 1ull << 63);
}
__device__ __forceinline__ double quantile_value(qkey_t k) { return __builtin_bit_cast(double, (k >> 63) ? (k ^ 1ull << 63) : ~k); }

// type-7 position of probability p among n >= 1 sorted values: the two ranks and the weight of the upper one
__device__ __forceinline__ void quantile_rank(long long n, double p, long long& lo, long long& hi, double& g) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double h = (double)(n - 1) * p;
  lo = (long long)__builtin_floor(h);
  if (lo > n - 1) lo = n - 1;
  hi = lo + 1 < n ? lo + 1 : n - 1;
  g = h - (double)lo;
}

// Q = x_lo if g == 0, else x_lo + g (x_hi - x_lo): difference, product and sum are rounded once each
__device__ __forceinline__ double quantile_mix(double xl, double xh, double g) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (g == 0.0) return xl;
  const double diff = xh - xl;
  const double prod = g * diff;
  return xl + prod;
}

__device__ __forceinline__ qkey_t wave_min_key(qkey_t v) {
#pragma unroll
  for (int m = kQWave / 2; m >= 1; m >>= 1) {
    const qkey_t o = __shfl_xor(v, m, kQWave);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ qkey_t wave_max_key(qkey_t v) {
#pragma unroll
  for (int m = kQWave / 2; m >= 1; m >>= 1) {
    const qkey_t o = __shfl_xor(v, m, kQWave);
    v = o > v ? o : v;
  }
  return v;
}

}  // namespace

// Resets the workspace of a slab: one workgroup per row.
__global__ __launch_bounds__(kQBlock) void quantile_init_kernel(int d, int R, long long* __restrict__ count /* [T] of the slab */,
                                                                qkey_t* __restrict__ kmin, qkey_t* __restrict__ kmax,
                                                                unsigned* __restrict__ hist, int* __restrict__ max_low) {
  const long rw = blockIdx.x;
  const int t = threadIdx.x;
  for (int r = 0; r < R; ++r) hist[((size_t)rw * R + r) * kQBins + t] = 0u;
  if (t == 0) {
    kmin[rw] = ~0ull;
    kmax[rw] = 0ull;
    if (rw % d == 0) count[rw / d] = 0;
    if (rw == 0) *max_low = 0;
  }
}

// Pass over the d mean rows of a time: grid (time of the slab, chunk of `iters` 256 trajectories).  Lane t serves the
// trajectories base + j 256 + t: every row read is 512 contiguous bytes per wavefront.  Writes the inclusion mask (the rule of
// load_means in summary_kernels.h), adds the count, and lowers / raises the key range of every row with one 64-bit integer
// atomic per row and workgroup.  The second walk over the rows reads what the first has just brought into the cache.
__global__ __launch_bounds__(kQBlock) void quantile_mask_kernel(const double* __restrict__ mean /* slab: [T][D][N] */,
                                                                const int* __restrict__ retcode, long N, int d, int D, int W,
                                                                int n_chunk, int iters, qkey_t* __restrict__ mask,
                                                                long long* __restrict__ count, qkey_t* __restrict__ kmin,
                                                                qkey_t* __restrict__ kmax) {
  __shared__ qkey_t sh_min[kQMaxDim][kQBlock / kQWave];
  __shared__ qkey_t sh_max[kQMaxDim][kQBlock / kQWave];
  __shared__ int sh_cnt[kQBlock / kQWave];
  const int t = threadIdx.x, lane = t % kQWave, wave = t / kQWave;
  const long ts = blockIdx.x / n_chunk;
  const long base = (long)(blockIdx.x % n_chunk) * iters * kQBlock;
  const double* mean_s = mean + (size_t)ts * D * N;
  unsigned mine = 0;
  for (int j = 0; j < iters; ++j) {
    const long i = base + (long)j * kQBlock + t;
    const long ic = i < N ? i : N - 1;  // a lane past the end reads the last trajectory and drops it
    bool in = i < N && retcode[ic] == 0;
    for (int a = 0; a < d; ++a) {
      const double v = mean_s[(size_t)a * N + ic];
      if (!(__builtin_fabs(v) <= 1.79769313486231570815e308)) in = false;  // NaN or Inf
    }
    const qkey_t word = __ballot(in);
    if (lane == 0 && i < N) mask[(size_t)ts * W + i / kQWave] = word;
    if (in) mine |= 1u << j;
  }
  {
    int n = __popc(mine);
#pragma unroll
    for (int m = kQWave / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, kQWave);
    if (lane == 0) sh_cnt[wave] = n;
  }
  for (int a = 0; a < d; ++a) {
    qkey_t mn = ~0ull, mx = 0ull;
    for (int j = 0; j < iters; ++j)
      if (mine >> j & 1u) {
        const qkey_t k = quantile_key(mean_s[(size_t)a * N + base + (long)j * kQBlock + t]);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
      }
    mn = wave_min_key(mn);
    mx = wave_max_key(mx);
    if (lane == 0) {
      sh_min[a][wave] = mn;
      sh_max[a][wave] = mx;
    }
  }
  __syncthreads();
  int n = 0;
  for (int w = 0; w < kQBlock / kQWave; ++w) n += sh_cnt[w];
  if (n == 0) return;  // nothing included here: the range and the count stay
  if (t == 0) atomicAdd((unsigned long long*)&count[ts], (unsigned long long)n);
  if (t < d) {
    qkey_t mn = ~0ull, mx = 0ull;
    for (int w = 0; w < kQBlock / kQWave; ++w) {
      mn = sh_min[t][w] < mn ? sh_min[t][w] : mn;
      mx = sh_max[t][w] > mx ? sh_max[t][w] : mx;
    }
    atomicMin(&kmin[ts * d + t], mn);
    atomicMax(&kmax[ts * d + t], mx);
  }
}

// Per row: the selection works on the OFFSET keys k - kmin, which lie in [0, kmax - kmin]: the leading zero bits of that width
// are the prefix of every rank and the digit passes start below them.  (The bits that kmin and kmax share would serve as well
// for most rows, but a row that straddles a value with a short mantissa -- 27 +- 1e-6 around 0x403B000000000000 -- shares 15
// bits where its width needs 30: the offset costs one subtraction per key and always leaves ceil(log2(width + 1)) bits.)  One
// lane per row.
__global__ __launch_bounds__(kQBlock) void quantile_start_kernel(long rows, int d, int P, QuantileProbs probs,
                                                                 const long long* __restrict__ count,
                                                                 const qkey_t* __restrict__ kmin, const qkey_t* __restrict__ kmax,
                                                                 int* __restrict__ low, qkey_t* __restrict__ prefix,
                                                                 unsigned* __restrict__ rem, int* __restrict__ owner,
                                                                 int* __restrict__ max_low) {
  const long rw = (long)blockIdx.x * kQBlock + threadIdx.x;
  if (rw >= rows) return;
  const long long n = count[rw / d];
  const int R = 2 * P;
  int lw = 0;
  if (n > 0) {
    const qkey_t x = kmax[rw] - kmin[rw];
    lw = x ? 64 - __clzll((long long)x) : 0;
  }
  for (int p = 0; p < P; ++p) {
    long long lo = 0, hi = 0;
    double g;
    if (n > 0) quantile_rank(n, probs.p[p], lo, hi, g);
    prefix[rw * R + 2 * p] = prefix[rw * R + 2 * p + 1] = 0ull;
    rem[rw * R + 2 * p] = (unsigned)lo;
    rem[rw * R + 2 * p + 1] = (unsigned)hi;
    owner[rw * R + 2 * p] = owner[rw * R + 2 * p + 1] = 0;
  }
  low[rw] = lw;
  if (lw > 0) atomicMax(max_low, lw);
}

// One digit pass, histogram half: grid (row, chunk).  A lane takes the next min(low, 8) bits of the offset key of its included values as the
// digit and counts it in the LDS histogram of every owner rank whose prefix the key carries; the workgroup then adds its
// non-zero bins to the row's histograms.
__global__ __launch_bounds__(kQBlock) void quantile_hist_kernel(const double* __restrict__ mean /* slab: [T][D][N] */,
                                                                const qkey_t* __restrict__ mask, long N, int d, int D, int W,
                                                                int n_chunk, int iters, int R, const qkey_t* __restrict__ kmin,
                                                                const int* __restrict__ low,
                                                                const qkey_t* __restrict__ prefix, const int* __restrict__ owner,
                                                                unsigned* __restrict__ hist) {
  __shared__ unsigned sh_hist[kQMaxRanks * kQBins];
  __shared__ qkey_t sh_pref[kQMaxRanks];
  __shared__ int sh_own[kQMaxRanks];
  __shared__ int sh_nown;
  const int t = threadIdx.x;
  const long rw = blockIdx.x / n_chunk;
  const int lw = low[rw];
  if (lw == 0) return;  // the row is finished (uniform over the workgroup)
  const int w = lw < 8 ? lw : 8, sh = lw - w;
  const long ts = rw / d;
  const int a = (int)(rw % d);
  const long base = (long)(blockIdx.x % n_chunk) * iters * kQBlock;
  for (int r = 0; r < R; ++r) sh_hist[r * kQBins + t] = 0u;
  if (t == 0) {
    int n = 0;
    for (int r = 0; r < R; ++r)
      if (owner[rw * R + r] == r) {
        sh_own[n] = r;
        sh_pref[n] = lw == 64 ? 0ull : prefix[rw * R + r] >> lw;
        ++n;
      }
    sh_nown = n;
  }
  __syncthreads();
  const int n_own = sh_nown;
  const double* row = mean + ((size_t)ts * D + a) * N;
  const qkey_t k0 = kmin[rw];
  for (int j = 0; j < iters; ++j) {
    const long i = base + (long)j * kQBlock + t;
    if (i >= N) break;
    if (!(mask[(size_t)ts * W + i / kQWave] >> (i % kQWave) & 1ull)) continue;
    const qkey_t k = quantile_key(row[i]) - k0;
    const qkey_t high = lw == 64 ? 0ull : k >> lw;
    const unsigned digit = (unsigned)(k >> sh) & ((1u << w) - 1u);
    for (int o = 0; o < n_own; ++o)
      if (high == sh_pref[o]) atomicAdd(&sh_hist[sh_own[o] * kQBins + digit], 1u);
  }
  __syncthreads();
  for (int o = 0; o < n_own; ++o) {
    const int r = sh_own[o];
    const unsigned c = sh_hist[r * kQBins + t];
    if (c) atomicAdd(&hist[((size_t)rw * R + r) * kQBins + t], c);
  }
}

// One digit pass, selection half: one workgroup per row, lane t owns bin t.  Prefix sum over the 256 bins of every rank's
// histogram (that of its owner), the bin that holds the remaining rank extends the prefix, the histograms are cleared.
__global__ __launch_bounds__(kQBlock) void quantile_select_kernel(int R, int* __restrict__ low, qkey_t* __restrict__ prefix,
                                                                  unsigned* __restrict__ rem, int* __restrict__ owner,
                                                                  unsigned* __restrict__ hist) {
  __shared__ unsigned sh_sum[2][kQMaxRanks * kQBins];
  __shared__ qkey_t sh_pref[kQMaxRanks];
  __shared__ unsigned sh_rem[kQMaxRanks];
  const int t = threadIdx.x;
  const long rw = blockIdx.x;
  const int lw = low[rw];
  if (lw == 0) return;
  const int w = lw < 8 ? lw : 8, sh = lw - w;
  for (int r = 0; r < R; ++r) sh_sum[0][r * kQBins + t] = hist[((size_t)rw * R + owner[rw * R + r]) * kQBins + t];
  if (t < R) {
    sh_pref[t] = prefix[rw * R + t];
    sh_rem[t] = rem[rw * R + t];
  }
  __syncthreads();
  int src = 0;
  for (int off = 1; off < kQBins; off <<= 1) {  // inclusive prefix sums of all ranks, one barrier per step
    for (int r = 0; r < R; ++r) {
      unsigned v = sh_sum[src][r * kQBins + t];
      if (t >= off) v += sh_sum[src][r * kQBins + t - off];
      sh_sum[src ^ 1][r * kQBins + t] = v;
    }
    __syncthreads();
    src ^= 1;
  }
  for (int r = 0; r < R; ++r) {  // exactly one bin holds the remaining rank (the histogram sums to more than it)
    const unsigned incl = sh_sum[src][r * kQBins + t];
    const unsigned excl = t ? sh_sum[src][r * kQBins + t - 1] : 0u;
    const unsigned k = rem[rw * R + r];
    if (k >= excl && k < incl) {
      sh_pref[r] = prefix[rw * R + r] | (qkey_t)t << sh;
      sh_rem[r] = k - excl;
    }
  }
  __syncthreads();
  for (int r = 0; r < R; ++r) hist[((size_t)rw * R + r) * kQBins + t] = 0u;
  if (t < R) {
    int own = t;
    for (int r = t - 1; r >= 0; --r)
      if (sh_pref[r] == sh_pref[t]) own = r;
    prefix[rw * R + t] = sh_pref[t];
    rem[rw * R + t] = sh_rem[t];
    owner[rw * R + t] = own;
  }
  if (t == 0) low[rw] = sh;
}

// Turns the keys back into doubles and forms Q: one lane per (row, probability).
__global__ __launch_bounds__(kQBlock) void quantile_finish_kernel(long rows, int d, int P, QuantileProbs probs,
                                                                  const long long* __restrict__ count,
                                                                  const qkey_t* __restrict__ kmin,
                                                                  const qkey_t* __restrict__ prefix,
                                                                  double* __restrict__ q /* slab: [T][P][d] */) {
  const long idx = (long)blockIdx.x * kQBlock + threadIdx.x;
  if (idx >= rows * P) return;
  const long rw = idx / P;
  const int p = (int)(idx % P);
  const long ts = rw / d;
  const int a = (int)(rw % d);
  const long long n = count[ts];
  double out = __builtin_nan("");
  if (n > 0) {
    long long lo, hi;
    double g;
    quantile_rank(n, probs.p[p], lo, hi, g);
    const qkey_t k0 = kmin[rw];
    out = quantile_mix(quantile_value(k0 + prefix[rw * 2 * P + 2 * p]), quantile_value(k0 + prefix[rw * 2 * P + 2 * p + 1]), g);
  }
  q[((size_t)ts * P + p) * d + a] = out;
}

}  // namespace odef
