// Device source of the per-trajectory solution errors (errors.hip and errors_field.h launch it; tests/emul/emul_errors.cpp builds
// the same text for the host to check it without a GPU).  Includes nothing: the including file provides the HIP
// runtime.
//
//   errors_partial_kernel<DR, Truth>  one lane per trajectory and time chunk: walks the chunk's saves, e = u - u*, and keeps
//                                     sum e^2, max |e|, sum e' Sigma^+ e, mean |e| of the last save, and the two counts
//   errors_fold_kernel                one lane per trajectory: folds the chunks in chunk order -> FINAL, L2, LINF, CHI2, NUSED
//   errors_truth_kernel<Truth>        writes u* at the trajectory's own save times (U_ANALYTIC), when asked for
//
// DR > 0: d == DR is a compile-time constant and the d x d block lives in registers; DR == 0: any d <= 32, the block lives in the
// lane's own column of an LDS tile [tri(d) + d][lanes] (no lane reads another's column: no barrier).
#pragma once

#ifndef ODEF_ERRORS_TILE
#define ODEF_ERRORS_TILE extern __shared__ double err_tile[]
#endif

#ifdef __clang__  // (DR == 0: the loops over d have a run-time bound, `#pragma unroll` then only warns)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
#endif

namespace odef {

constexpr int kErrBlock = 256;     // lanes per workgroup (register path)
constexpr int kErrRegD = 8;        // largest d whose block is kept in registers (tri(8) + 8 = 44 doubles)
constexpr int kErrMaxSplit = 64;   // most chunks of the time axis
constexpr int kErrMinChunk = 8;    // fewest saves per chunk
constexpr int kErrPartRows = 4;    // rows of a chunk's partial: sum e^2, max |e|, sum chi, mean |e| of its last used save

// lanes of a workgroup that carry a trajectory: 256 on the register path, else the largest power of two <= 64 whose tile stays
// within 64 KiB (d <= 14: 64, <= 21: 32, <= 30: 16, above: 8); the workgroup then has 64 threads
inline int errors_lanes(int d) {
  if (d <= kErrRegD) return kErrBlock;
  const long col = (long)d * (d + 1) / 2 + d;
  int L = 64;
  while (L > 8 && col * L * 8 > 65536) L /= 2;
  return L;
}
// chunks of the time axis: doubled until the grid holds 1 024 workgroups (four per compute unit) or a chunk would fall below
// kErrMinChunk saves
inline int errors_split(long N, long n_save, int lanes) {
  const long nb = (N + lanes - 1) / lanes;
  int S = 1;
  while (S < kErrMaxSplit && nb * S < 1024 && n_save >= (long)kErrMinChunk * (S * 2)) S *= 2;
  return S;
}

struct ErrArgs {
  const double* mean;    // [n_save][D][N]
  const double* cov;     // [n_save][TRI][N]
  const double* tsave;   // adaptive: [n_save][N], else nullptr
  const int* nsaved;     // adaptive: [N], else nullptr
  long N, n_save, chunk;
  int d, D, TRI, lanes, n_split;
  double* part;          // [n_split][kErrPartRows][N]
  int* part_cnt;         // [n_split][2][N]: used saves, saves with a non-zero block
};

// the truth from a buffer [n_save][d][N] (a bound reference, or a materialised U_ANALYTIC)
struct TruthBuffer {
  struct Args {
    const double* ref;
    long N;
    int d;
  };
  Args a;
  const double* row;
  __device__ explicit TruthBuffer(const Args& args) : a(args), row(args.ref) {}
  __device__ void init(long) {}
  __device__ void at(long k, long i) { row = a.ref + (size_t)k * a.d * a.N + i; }
  __device__ double get(int c) const { return row[(size_t)c * a.N]; }
};

// the truth from the vector field's own `analytic(u0, p, t, out)`
struct AnalyticArgs {
  const double* u0;  // [d][N]
  const double* p;   // [np] or [np][N]
  const double* t;   // time of save k of trajectory i at t[k t_sk + i t_si]
  long N, t_sk, t_si;
  int p_shared;
};
// ... whose solution depends on the initial time: `analytic(u0, p, t0, t, out)`; t0 is the time of save 0
template <class...>
using err_void_t = void;
template <class RHS, class = void>
struct AnalyticTakesT0 { static constexpr bool value = false; };
template <class RHS>
struct AnalyticTakesT0<RHS, err_void_t<decltype(RHS::analytic(*(const double (*)[RHS::d])nullptr, (const double*)nullptr, 0.0, 0.0,
                                                              *(double (*)[RHS::d])nullptr))>> {
  static constexpr bool value = true;
};
template <class RHS>
struct TruthAnalytic {
  using Args = AnalyticArgs;
  Args a;
  double u0l[RHS::d], pl[RHS::np > 0 ? RHS::np : 1], out[RHS::d], t0;
  __device__ explicit TruthAnalytic(const Args& args) : a(args) {}
  __device__ void init(long i) {
    for (int c = 0; c < RHS::d; ++c) u0l[c] = a.u0[(size_t)c * a.N + i];
    for (int c = 0; c < RHS::np; ++c) pl[c] = a.p_shared ? a.p[c] : a.p[(size_t)c * a.N + i];
    if constexpr (AnalyticTakesT0<RHS>::value) t0 = a.t[i * a.t_si];
  }
  __device__ void at(long k, long i) {
    if constexpr (AnalyticTakesT0<RHS>::value) RHS::analytic(u0l, pl, t0, a.t[k * a.t_sk + i * a.t_si], out);
    else RHS::analytic(u0l, pl, a.t[k * a.t_sk + i * a.t_si], out);
  }
  __device__ double get(int c) const { return out[c]; }
};

namespace {

// the lane's copy of one save: tri(d) packed block entries, then the d entries of e
template <int DR>
struct ErrColumn {
  double v[DR * (DR + 1) / 2 + DR];
  __device__ __forceinline__ ErrColumn(double*, int) {}
  __device__ __forceinline__ double& operator[](int k) { return v[k]; }
};
template <>
struct ErrColumn<0> {
  double* base;
  int stride;
  __device__ __forceinline__ ErrColumn(double* b, int s) : base(b), stride(s) {}
  __device__ __forceinline__ double& operator[](int k) { return base[(size_t)k * stride]; }
};

// max that keeps a NaN once it has one
__device__ __forceinline__ double nan_max(double m, double v) { return (m != m) ? m : (!(v <= m) ? v : m); }

// e' Sigma^+ e by elimination (Sigma = L D L', e' Sigma^+ e = sum_k y_k^2 / D_k with L y = e), in place.  A non-positive pivot
// drops its direction (column zeroed, reciprocal taken as 0: the semi-definite rule of ek_math.h); a NaN pivot propagates.
template <int DR>
__device__ __forceinline__ double err_quad(ErrColumn<DR>& c, int d) {
  const int tri = d * (d + 1) / 2;
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < d; ++k) {
    const double piv = c[k * (k + 1) / 2 + k];
    const double inv = (piv <= 0.0) ? 0.0 : 1.0 / piv;
    const double y = c[tri + k];
    q += y * y * inv;
#pragma unroll
    for (int i = k + 1; i < d; ++i) {
      const double l = c[i * (i + 1) / 2 + k] * inv;
      c[tri + i] -= l * y;
#pragma unroll
      for (int j = k + 1; j <= i; ++j) c[i * (i + 1) / 2 + j] -= l * c[j * (j + 1) / 2 + k];
    }
  }
  return q;
}

}  // namespace

template <int DR, class Truth>
__global__ __launch_bounds__(kErrBlock) void errors_partial_kernel(ErrArgs a, typename Truth::Args ta) {
  const int d = DR ? DR : a.d;
  const int tri = d * (d + 1) / 2;
  const long n_block = (a.N + a.lanes - 1) / a.lanes;
  const long blk = blockIdx.x % n_block;
  const int split = (int)(blockIdx.x / n_block);
  const long i = blk * a.lanes + threadIdx.x;
  if ((int)threadIdx.x >= a.lanes || i >= a.N) return;
  double* colbase = nullptr;
  if constexpr (DR == 0) {
    ODEF_ERRORS_TILE;
    colbase = err_tile + threadIdx.x;
  }
  ErrColumn<DR> c(colbase, a.lanes);
  Truth tr(ta);
  tr.init(i);
  const long N = a.N;
  const long k0 = (long)split * a.chunk;
  long k1 = k0 + a.chunk < a.n_save ? k0 + a.chunk : a.n_save;
  if (a.nsaved) {  // a lane drops out at its own record count
    const long ns = a.nsaved[i];
    k1 = ns < k1 ? ns : k1;
  }
  double sumsq = 0.0, linf = 0.0, chisum = 0.0, fin = 0.0;
  int nused = 0, nchi = 0;
  double tprev = (a.tsave && k0 > 0 && k0 < k1) ? a.tsave[(size_t)(k0 - 1) * N + i] : 0.0;
  for (long k = k0; k < k1; ++k) {
    if (a.tsave) {  // a rejected attempt repeats the record at the unchanged time: not a save of the solution
      const double t = a.tsave[(size_t)k * N + i];
      const bool repeat = k > 0 && t == tprev;
      tprev = t;
      if (repeat) continue;
    }
    tr.at(k, i);
    const double* m = a.mean + (size_t)k * a.D * N + i;
    const double* s = a.cov + (size_t)k * a.TRI * N + i;
    double fk = 0.0;
#pragma unroll
    for (int r = 0; r < d; ++r) {
      const double e = m[(size_t)r * N] - tr.get(r);
      const double ae = __builtin_fabs(e);
      c[tri + r] = e;
      fk += ae;
      sumsq += e * e;
      linf = nan_max(linf, ae);
    }
    fin = fk / d;
    ++nused;
    bool zero = true;
#pragma unroll
    for (int p = 0; p < tri; ++p) {
      const double v = s[(size_t)p * N];
      c[p] = v;
      zero = zero && v == 0.0;
    }
    if (!zero) {  // the initial record, and u' = 0, have no uncertainty to calibrate against
      chisum += err_quad<DR>(c, d);
      ++nchi;
    }
  }
  double* out = a.part + (size_t)split * kErrPartRows * N + i;
  out[0] = sumsq;
  out[(size_t)N] = linf;
  out[(size_t)2 * N] = chisum;
  out[(size_t)3 * N] = fin;
  int* cnt = a.part_cnt + (size_t)split * 2 * N + i;
  cnt[0] = nused;
  cnt[(size_t)N] = nchi;
}

// Folds the chunks of a trajectory in chunk order: sums and counts add, the maximum combines, FINAL is that of the last chunk that
// used a save.  out: final, l2, linf, chi2 [N] each; nused [N] int64.  (A template, so that only errors.hip emits it.)
template <class = void>
__global__ void errors_fold_kernel(const double* __restrict__ part, const int* __restrict__ part_cnt, int n_split, long N, int d,
                                   double* __restrict__ fin, double* __restrict__ l2, double* __restrict__ linf,
                                   double* __restrict__ chi2, long long* __restrict__ nused) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double sumsq = 0.0, mx = 0.0, chi = 0.0, f = __builtin_nan("");
  long long nu = 0, nc = 0;
  for (int s = 0; s < n_split; ++s) {
    const double* p = part + (size_t)s * kErrPartRows * N + i;
    const int* c = part_cnt + (size_t)s * 2 * N + i;
    const int u = c[0];
    if (u == 0) continue;
    sumsq += p[0];
    mx = nan_max(mx, p[(size_t)N]);
    chi += p[(size_t)2 * N];
    f = p[(size_t)3 * N];
    nu += u;
    nc += c[(size_t)N];
  }
  const double nan = __builtin_nan("");
  fin[i] = f;
  l2[i] = nu > 0 ? __builtin_sqrt(sumsq / ((double)nu * d)) : nan;
  linf[i] = nu > 0 ? mx : nan;
  chi2[i] = nc > 0 ? chi / (double)nc / d : nan;
  nused[i] = nu;
}

// u* of every save slot of every trajectory, [n_save][d][N]; slots past a trajectory's record count get 0
template <class Truth>
__global__ __launch_bounds__(kErrBlock) void errors_truth_kernel(typename Truth::Args ta, const int* __restrict__ nsaved, long N,
                                                                 long n_save, int d, double* __restrict__ out) {
  const long n_block = (N + blockDim.x - 1) / blockDim.x;
  const long i = (long)(blockIdx.x % n_block) * blockDim.x + threadIdx.x;
  const long k = blockIdx.x / n_block;
  if (i >= N || k >= n_save) return;
  Truth tr(ta);
  tr.init(i);
  const bool live = !nsaved || k < nsaved[i];
  if (live) tr.at(k, i);
  for (int r = 0; r < d; ++r) out[((size_t)k * d + r) * N + i] = live ? tr.get(r) : 0.0;
}

}  // namespace odef

#ifdef __clang__
#pragma clang diagnostic pop
#endif
