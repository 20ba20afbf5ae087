// Device source of the data log-likelihood pass (datalik.hip launches it; tests/emul/emul_datalik.cpp builds the same text for the
// host to check it without a GPU).
//
//   data_loglik_kernel<d, q>   one lane per trajectory: walks the filter records of a fixed grid from the last save down to the
//                              first observed one.  The carried Gaussian xi starts as the last filter record; every save below
//                              takes one RTS step against it (rts_step_core, smooth_lane.h: the smoother's arithmetic, registers
//                              left to the compiler), every observed save then conditions it on y_j = H x + N(0, diag r) and adds
//                              that observation's Gaussian log-density to the sum.  H is rows of the identity on the first d
//                              coordinates and is never formed: the components are an index list, kept as one slot per state
//                              component, so that every register array is indexed by compile-time constants only.
//
// Reads each record once (512 contiguous bytes per wavefront and row), writes two doubles per trajectory.  The pass needs no
// vector field: the kernels depend on (d, q) alone.
#pragma once
#include "smooth_lane.h"

namespace odef {

constexpr int kDataLikWave = 64;
constexpr int kDataLikMaxD = 4;        // state components
constexpr int kDataLikMaxState = 20;   // d (q + 1)

struct DataLikArgs {
  PriorConsts pc;
  long N, n_save;
  const double* ptab;          // preconditioner tables of the grid (precond_fill, ek_math.h)
  const int* tab_idx;          // [n_save - 1]
  const double* hs;            // [n_save - 1]: t_{k+1} - t_k
  const double* mean;          // filter records [n_save][D][N]
  const double* cov;           // [n_save][TRI][N]
  const double* diff;          // [n_save][N]: slot k + 1 holds the diffusion of the step k -> k + 1
  const long long* obs_save;   // [M] strictly increasing, in 0 .. n_save - 1
  const long long* obs_comp;   // [o] strictly increasing, in 0 .. d - 1
  const double* obs_val;       // [M][o], or per trajectory [M][o][N]
  const double* obs_noise;     // [o] variances
  int M, o, per_traj;
  double* loglik;              // [N]
  double* maha;                // [N]
};

// Conditions xi = (xm, xP) on the observation yv of the components with slot[c] >= 0 (noise variances rn) and adds its Gaussian
// log-density terms: S = H P H' + R lives in the d x d packed triangle of the observed components -- rows and columns of the
// others are zero and skipped, which is the o x o packed matrix in place --, factored S = L D L'.  `bad`: a pivot that is not
// positive.
template <int d, int D>
__device__ inline void datalik_update(double (&xm)[D], double (&xP)[D * (D + 1) / 2], const int (&slot)[d], const double (&rn)[d],
                                      const double (&yv)[d], double& quad, double& logdet, bool& bad) {
  constexpr int td = d * (d + 1) / 2;
  double S[td], v[d], dinv[d];
#pragma unroll
  for (int a = 0; a < d; ++a) {
    const bool oa = slot[a] >= 0;
    v[a] = oa ? yv[a] - xm[a] : 0.0;
#pragma unroll
    for (int b = 0; b <= a; ++b) S[tri(a, b)] = (oa && slot[b] >= 0) ? xP[tri(a, b)] : 0.0;
    S[tri(a, a)] += oa ? rn[a] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < d; ++k) {
    const bool ok_ = slot[k] >= 0;
    const double piv = S[tri(k, k)];
    const bool pos = piv > 0.0;
    bad = bad || (ok_ && !pos);
    const double inv = (ok_ && pos) ? 1.0 / piv : 0.0;
    dinv[k] = inv;
    logdet += (ok_ && pos) ? log(piv) : 0.0;
    double vc[d];
#pragma unroll
    for (int i = k + 1; i < d; ++i) {
      vc[i] = S[tri(i, k)];
      S[tri(i, k)] = vc[i] * inv;
    }
#pragma unroll
    for (int j = k + 1; j < d; ++j)
#pragma unroll
      for (int i = j; i < d; ++i) S[tri(i, j)] -= S[tri(i, k)] * vc[j];
  }
  // w = L^-1 v;  v' S^-1 v = sum w_k^2 / D_k;  x = S^-1 v
  double x[d];
#pragma unroll
  for (int k = 0; k < d; ++k) {
    double t = v[k];
#pragma unroll
    for (int c = 0; c < k; ++c) t -= S[tri(k, c)] * x[c];
    x[k] = t;
  }
#pragma unroll
  for (int k = 0; k < d; ++k) {
    quad += x[k] * x[k] * dinv[k];
    x[k] *= dinv[k];
  }
#pragma unroll
  for (int k = d - 1; k >= 0; --k) {
    double t = x[k];
#pragma unroll
    for (int c = k + 1; c < d; ++c) t -= S[tri(c, k)] * x[c];
    x[k] = t;
  }
  // U = L^-1 (H P), one column per state coordinate;  m += P H' x;  P -= U' D^-1 U  ( = K S K' )
  double U[d][D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < d; ++k) {
      double u = slot[k] >= 0 ? xP[symidx(i, k)] : 0.0;
      t += u * x[k];
#pragma unroll
      for (int c = 0; c < k; ++c) u -= S[tri(k, c)] * U[c][i];
      U[k][i] = u;
    }
    xm[i] += t;
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double t = xP[tri(i, j)];
#pragma unroll
      for (int k = 0; k < d; ++k) t -= (U[k][i] * dinv[k]) * U[k][j];
      xP[tri(i, j)] = t;
    }
}

// One record into registers: every load of the record in flight before anything is done with it.  D <= 12 goes through the buffer
// descriptors of the lane smoother (RowLoad: the row offset a running scalar, no address arithmetic per load); above, the running
// scalars of two descriptors no longer fit beside the step's own, and the rows are read through the lane's pointer -- the same 512
// contiguous bytes per wavefront and row.
template <int D>
__device__ inline void datalik_load(const double* __restrict__ mean, const double* __restrict__ cov, size_t k, size_t N, long i0,
                                    unsigned lane, double (&m)[D], double (&C)[D * (D + 1) / 2]) {
  constexpr int TRI = D * (D + 1) / 2;
  if constexpr (D <= 12) {
    RowLoad lc(cov + (k * TRI) * N + i0, N, TRI, lane), lm(mean + (k * D) * N + i0, N, D, lane);
#pragma unroll
    for (int e = 0; e < TRI; ++e) C[e] = lc.get();
#pragma unroll
    for (int e = 0; e < D; ++e) m[e] = lm.get();
  } else {
    const double* pc = cov + (k * TRI) * N + i0 + lane;
    const double* pm = mean + (k * D) * N + i0 + lane;
#pragma unroll
    for (int e = 0; e < TRI; ++e) {
      C[e] = *pc;
      pc += N;
    }
#pragma unroll
    for (int e = 0; e < D; ++e) {
      m[e] = *pm;
      pm += N;
    }
  }
}

template <int d, int q>
__device__ ODEF_FORCE_INLINE void data_loglik_lane(const DataLikArgs& P, long i0, unsigned lane, const LaneMem& xl) {
  constexpr int NB = q + 1, D = d * NB, TRI = D * (D + 1) / 2;
  static_assert(d <= kDataLikMaxD && D <= kDataLikMaxState, "data log-likelihood: d <= 4, d (q + 1) <= 20");
  const long i = i0 + lane;
  const size_t N = (size_t)P.N;
  const long n = P.n_save;
  // the observed components, one slot per state component (wave-uniform)
  int slot[d];
  double rn[d];
#pragma unroll
  for (int c = 0; c < d; ++c) slot[c] = -1;
  for (int a = 0; a < P.o; ++a) {
    const long long cc = uniform_load(P.obs_comp + a);
#pragma unroll
    for (int c = 0; c < d; ++c) slot[c] = (cc == c) ? a : slot[c];
  }
#pragma unroll
  for (int c = 0; c < d; ++c) rn[c] = uniform_load(P.obs_noise + (slot[c] >= 0 ? slot[c] : 0));
  bool bad = false;
  double xm[D], xP[TRI];
  datalik_load<D>(P.mean, P.cov, (size_t)(n - 1), N, i0, lane, xm, xP);
#pragma unroll
  for (int k = 0; k < TRI; ++k) bad = bad || !(xP[k] == xP[k]);
#pragma unroll
  for (int k = 0; k < D; ++k) bad = bad || !(xm[k] == xm[k]);
  double quad = 0.0, logdet = 0.0;
  int j = P.M - 1;
  long next = (long)uniform_load(P.obs_save + j);
  const long k_first = (long)uniform_load(P.obs_save);
  for (long k = n - 1; k >= k_first; --k) {
    const double h = k < n - 1 ? uniform_load(P.hs + k) : 0.0;
    if (h != 0.0) {  // (h == 0: xi unchanged, the copy branch of src/smoothing.jl:13-16)
      double pj[NB], pij[NB];
      const GlobalTab tab{P.ptab + (size_t)uniform_load(P.tab_idx + k) * kTabStride};
#pragma unroll
      for (int J = 0; J < NB; ++J) {
        pj[J] = tab[kTabPJ + J];
        pij[J] = tab[kTabPIJ + J];
      }
      const double sigma2 = P.diff[(size_t)(k + 1) * N + i];
      double mt[D], B[TRI];
      datalik_load<D>(P.mean, P.cov, (size_t)k, N, i0, lane, mt, B);
      ODEF_SCHED_FENCE();
      bad = bad || !(sigma2 == sigma2);
#pragma unroll
      for (int e = 0; e < TRI; ++e) bad = bad || !(B[e] == B[e]);
#pragma unroll
      for (int e = 0; e < D; ++e) bad = bad || !(mt[e] == mt[e]);
      double msn[D], Cs[TRI], mo[D];
#pragma unroll
      for (int e = 0; e < D; ++e) {
        mt[e] *= pj[e / d];
        msn[e] = pj[e / d] * xm[e];
      }
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          const double s = pj[a / d] * pj[b / d];
          const double x = B[tri(a, b)] * s;
          xl.set(tri(a, b), x);
          B[tri(a, b)] = x;
          Cs[tri(a, b)] = xP[tri(a, b)] * s;
        }
      // B is dead inside the core once the covariance rows are being produced: it receives them (as in sample_lane.h)
      auto sink = [&](int e, double v) { B[e] = v; };
      // (forced in line: left to its cost model the compiler keeps the core of the largest states as a function of its own, and no
      // kernel of this library calls one)
      ODEF_INLINE_CALL rts_step_core<d, NB>(P.pc, pij, mt, B, Cs, msn, sigma2, xl, mo, sink);
#pragma unroll
      for (int e = 0; e < D; ++e) xm[e] = mo[e];
#pragma unroll
      for (int e = 0; e < TRI; ++e) xP[e] = B[e];
    }
    if (k == next) {
      double yv[d];
#pragma unroll
      for (int c = 0; c < d; ++c) {
        const size_t e = (size_t)j * P.o + (slot[c] >= 0 ? slot[c] : 0);
        yv[c] = P.per_traj ? P.obs_val[e * N + i] : uniform_load(P.obs_val + e);
        bad = bad || (slot[c] >= 0 && !(yv[c] == yv[c]));
      }
      datalik_update<d, D>(xm, xP, slot, rn, yv, quad, logdet, bad);
      --j;
      next = j >= 0 ? (long)uniform_load(P.obs_save + j) : -1;
    }
  }
  const double nan = __builtin_nan("");
  const double cnt = (double)P.M * (double)P.o;
  P.loglik[i] = bad ? nan : -0.5 * (quad + logdet + cnt * 1.8378770664093453);
  P.maha[i] = bad ? nan : quad;
}

#ifndef ODEF_HOST_EMUL
// One wavefront per workgroup; the lane-private copy of the step's filter covariance sits in LDS (TRI x 64 doubles), like the lane
// smoother's.
template <int d, int q>
__global__ __launch_bounds__(kDataLikWave) void data_loglik_kernel(const DataLikArgs P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kDataLikWave];
  const long i0 = (long)blockIdx.x * kDataLikWave;
  const LaneMem xl{lds + threadIdx.x, kDataLikWave};
  if (i0 + threadIdx.x < P.N) data_loglik_lane<d, q>(P, i0, threadIdx.x, xl);
}
#endif

}  // namespace odef
