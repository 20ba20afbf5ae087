// Device source of the data log-likelihood at arbitrary observation times (datalik_times.hip launches it;
// tests/emul/emul_datalik_times.cpp builds the same text for the host to check it without a GPU).
//
//   data_loglik_times_kernel<d, q>   one lane per trajectory: the backward sweep of data_loglik_kernel (datalik_kernels.h) over the
//                                    AUGMENTED chain of the trajectory -- its filter records, on a fixed or on its own adaptive grid,
//                                    plus one node per observation time that is no save time.  A node inside the step k -> k + 1 is
//                                    the filter's prediction from record k over h1 = tau - t_k in the coordinates of P(h1) with
//                                    DIFFUSION[k + 1] (what event_eval, events_kernels.h, forms for the filter source); it takes one
//                                    RTS step against the carried Gaussian xi with h2 = t(xi) - tau in the coordinates of P(h2), and
//                                    is then observed (datalik_update).  The steps per unit come from precond_from_h per lane.
//
// The save index k is wave-uniform and runs from the wavefront's largest record count down; a lane joins at its own last record.
// Every lane of the wavefront reads row k of the records at the same time (512 contiguous bytes per row), lanes differ only in the
// number of nodes they handle between two saves.  One loop body -- load record k, (predict to the node,) one RTS step, (observe) --
// serves the step onto a node and the step onto a save, so that the step is inlined once.  The step is rts_step_core's arithmetic
// cut in two (smooth_lane.h's pieces, unedited): a node is carried in the form the first half produces and the second half is run
// at saves only, so that no step factors the near-singular prediction of a node shortly above a save (see the step).  The record
// is read again for every node of a step (from cache) instead of being kept: a fourth packed matrix does not fit the registers.
//
// Bounds: k stays in 0 .. min(NSAVED, capacity) - 1, the observation index in 0 .. M - 1, the node loop of one save runs at most
// M + 1 times, and a lane at or beyond N does nothing: at most n_i + M steps per lane, whatever the inputs hold.
#pragma once
#include "datalik_kernels.h"
#include "dense_lane.h"

namespace odef {

constexpr int kDataLikTimesMaxState = 12;  // d (q + 1): what the lane dense output serves

struct DataLikTimesArgs {
  PriorConsts pc;
  long N, n_save;              // fixed grid: number of saves; adaptive: capacity of the records
  int adaptive;
  const double* tgrid;         // fixed: [n_save]
  const double* tsave;         // adaptive: [n_save][N]
  const int* nsaved;           // adaptive: [N]
  const double* mean;          // filter records [n_save][D][N]
  const double* cov;           // [n_save][TRI][N]
  const double* diff;          // [n_save][N]: slot k + 1 holds the diffusion of the step k -> k + 1
  const double* obs_time;      // [M] strictly increasing
  const long long* obs_comp;   // [o] strictly increasing, in 0 .. d - 1
  const double* obs_val;       // [M][o], or per trajectory [M][o][N]
  const double* obs_noise;     // [o] variances
  int M, o, per_traj;
  double* loglik;              // [N]
  double* maha;                // [N]
  long host_n_hi;              // host build only: the largest record count of the emulated wavefront (0: the lane's own)
};

// true when any lane of the wavefront holds b (every lane of the wavefront calls it)
__device__ ODEF_FORCE_INLINE bool datalik_wave_any(bool b) {
#ifdef ODEF_HOST_EMUL
  return b;
#else
  return __any((int)b) != 0;
#endif
}

// The observation of a NODE whose Gaussian is held relative to its own prediction (m, X) -- the node's filter mean and covariance in
// the coordinates of the step, X in the lane's LDS column -- as  mean = m + X w,  cov = X + X W X  (data_loglik_times_lane says why).
// In that form  cov H' = X U  with  U = (I + W X) H',  so conditioning on y is  w += U S^-1 v,  W -= U S^-1 U'  and no inverse of X is
// taken.  H = s0 times rows of the identity on the first d coordinates (s0: the un-preconditioning of derivative block 0).  Sums and
// pivot rule as in datalik_update.
template <int d, int D>
__device__ ODEF_FORCE_INLINE void datalik_update_node(double (&w)[D], double (&W)[D * (D + 1) / 2], const double (&m)[D], const LaneMem& xl,
                                                      double s0, const int (&slot)[d], const double (&rn)[d], const double (&yv)[d],
                                                      double& quad, double& logdet, bool& bad) {
  constexpr int td = d * (d + 1) / 2;
  double U[d][D], S[td], v[d], dinv[d];
#pragma unroll
  for (int c = 0; c < d; ++c) {
    const bool oc = slot[c] >= 0;
    double xh[D];  // X H' / s0, column c
#pragma unroll
    for (int i = 0; i < D; ++i) xh[i] = oc ? xl.get(symidx(i, c)) : 0.0;
    double hm = m[c];
#pragma unroll
    for (int i = 0; i < D; ++i) hm += xh[i] * w[i];
    v[c] = oc ? yv[c] - s0 * hm : 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) t += W[symidx(i, k)] * xh[k];
      U[c][i] = oc ? t + (i == c ? 1.0 : 0.0) : 0.0;  // U / s0
    }
  }
  // S = H cov H' + R = s0^2 H0 X U / s0 + R: entry (a, b) is row a of X times column b of U
#pragma unroll
  for (int a = 0; a < d; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) t += xl.get(symidx(a, i)) * U[b][i];
      S[tri(a, b)] = (slot[a] >= 0 && slot[b] >= 0) ? (s0 * s0) * t : 0.0;
      if (a == b) S[tri(a, a)] += slot[a] >= 0 ? rn[a] : 0.0;
    }
#pragma unroll
  for (int c = 0; c < d; ++c)
#pragma unroll
    for (int i = 0; i < D; ++i) U[c][i] *= s0;
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
  // w += U' x;  U <- L^-1 U;  W -= U' D^-1 U
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < d; ++k) {
      double u = U[k][i];
      t += u * x[k];
#pragma unroll
      for (int c = 0; c < k; ++c) u -= S[tri(k, c)] * U[c][i];
      U[k][i] = u;
    }
    w[i] += t;
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double t = W[tri(i, j)];
#pragma unroll
      for (int k = 0; k < d; ++k) t -= (U[k][i] * dinv[k]) * U[k][j];
      W[tri(i, j)] = t;
    }
}

// The sweep of the wavefront's lane `lane` (trajectory i0 + lane).  Every lane of the wavefront calls it, `valid` or not: the save
// index and the votes are wave-uniform.  A lane that is not valid reads and writes nothing.
template <int d, int q>
__device__ ODEF_FORCE_INLINE void data_loglik_times_lane(const DataLikTimesArgs& P, long i0, unsigned lane, bool valid,
                                                         const LaneMem& xl) {
  constexpr int NB = q + 1, D = d * NB, TRI = D * (D + 1) / 2;
  static_assert(d <= kDataLikMaxD && D <= kDataLikTimesMaxState, "data log-likelihood at times: d <= 4, d (q + 1) <= 12");
  const long i = i0 + lane;
  const size_t N = (size_t)P.N;
  const long cap = P.n_save;
  const int M = P.M;
  // the lane's own record count, clamped to the records the context holds before it indexes anything
  long n = 0;
  if (valid) {
    n = P.adaptive ? (long)P.nsaved[i] : cap;
    n = n < 0 ? 0 : n > cap ? cap : n;
  }
  long n_hi = P.adaptive ? wave_uniform_max(n, valid) : cap;
#ifdef ODEF_HOST_EMUL
  if (P.adaptive && P.host_n_hi > n_hi) n_hi = P.host_n_hi < cap ? P.host_n_hi : cap;  // the lane joins below the wavefront's start
#endif
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
  bool bad = n < 1;            // no record: nothing covers the times
  bool done = !valid || n < 1;
  double xm[D], xP[TRI];
#pragma unroll
  for (int e = 0; e < D; ++e) xm[e] = 0.0;
#pragma unroll
  for (int e = 0; e < TRI; ++e) xP[e] = 0.0;
  double quad = 0.0, logdet = 0.0;
  double txi = 0.0;            // the time of xi
  bool wform = false;          // xi is a node held as (w, W) in xm, xP (see the step below)
  int j = M - 1;               // the next observation, from the last down
  double tau = uniform_load(P.obs_time + j);
  for (long k = n_hi - 1; k >= 0; --k) {
    if (!datalik_wave_any(!done)) break;  // every lane has met its first observation: the sweep ends there
    if (!done && k <= n - 1) {
      const bool join = k == n - 1;         // the lane's last record: xi starts as it
      const double tk = P.adaptive ? P.tsave[(size_t)k * N + i] : uniform_load(P.tgrid + k);
      const double sigma2 = join ? 0.0 : P.diff[(size_t)(k + 1) * N + i];
      // the records end before the last observation time: NaN for this trajectory only
      if (join && !(tau <= tk)) bad = done = true;
      // The nodes of the step k -> k + 1 from the right to the left, then save k itself: at most M + 1 turns.
      for (int it = 0; it <= M && !done; ++it) {
        const bool node = !join && j >= 0 && tau > tk;
        const double tt = node ? tau : tk;
        const double h2 = txi - tt;
        const bool step = !join && (node || h2 != 0.0);  // (h2 == 0 at a save: xi unchanged)
        if (join || step) {
          double mt[D], B[TRI];
          datalik_load<D>(P.mean, P.cov, (size_t)k, N, i0, lane, mt, B);
          ODEF_SCHED_FENCE();
          bad = bad || (step && !(sigma2 == sigma2));
#pragma unroll
          for (int e = 0; e < TRI; ++e) bad = bad || !(B[e] == B[e]);
#pragma unroll
          for (int e = 0; e < D; ++e) bad = bad || !(mt[e] == mt[e]);
          if (join) {
#pragma unroll
            for (int e = 0; e < D; ++e) xm[e] = mt[e];
#pragma unroll
            for (int e = 0; e < TRI; ++e) xP[e] = B[e];
          } else {
            double pj[NB], pij[NB];
            precond_from_h<q>(h2, pj, pij);
            if (node) {
              // the filter's prediction from record k at tau in the coordinates of P(h1), handed on un-preconditioned
              double pj1[NB], pij1[NB];
              precond_from_h<q>(tau - tk, pj1, pij1);
              double mp[D];
#pragma unroll
              for (int e = 0; e < D; ++e) mp[e] = pj1[e / d] * mt[e];
#pragma unroll
              for (int J = 0; J < NB; ++J)
#pragma unroll
                for (int a = 0; a < d; ++a) {
                  double s = mp[J * d + a];
#pragma unroll
                  for (int jj = J + 1; jj < NB; ++jj) s += P.pc.At[J][jj] * mp[jj * d + a];
                  mt[J * d + a] = pij1[J] * s;
                }
#pragma unroll
              for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) B[tri(a, b)] *= pj1[a / d] * pj1[b / d];
              predict_cov_inplace<d, NB>(P.pc, B, sigma2);
#pragma unroll
              for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) B[tri(a, b)] *= pij1[a / d] * pij1[b / d];
            }
            // The step in two halves, rts_step_core's arithmetic operation by operation.  RECOVER: (w, W) with
            //   xi.m = m^- + B w,  xi.P = B + B W B,   B = A X A' + sigma2 Q the prediction of this entry at the time of xi,
            // then  w <- A' w,  W <- A' W A, so that this entry's smoothed Gaussian is  m + X w,  X + X W X.  APPLY forms it.
            // A node is not applied: it keeps (w, W) -- its own X is the B of the entry below it, because predictions from record k
            // compose --, is observed in that form (datalik_update_node), and the entry below starts at the congruence.  So the
            // step from a node onto the save shortly below it never factors its B, which is the rank-deficient filter covariance
            // of the save plus a Q below its rounding: factoring it (the core called per entry) gave wrong numbers and NaN there.
            double wv[D], Cs[TRI];
#pragma unroll
            for (int e = 0; e < D; ++e) mt[e] *= pj[e / d];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
              for (int b = 0; b <= a; ++b) {
                const double s = pj[a / d] * pj[b / d];
                const double x = B[tri(a, b)] * s;
                xl.set(tri(a, b), x);
                B[tri(a, b)] = x;
                Cs[tri(a, b)] = wform ? xP[tri(a, b)] * (pij[a / d] * pij[b / d]) : xP[tri(a, b)] * s;
              }
            double dl[D];
            if (wform) {
#pragma unroll
              for (int e = 0; e < D; ++e) dl[e] = xm[e] * pij[e / d];
            } else {
#pragma unroll
              for (int J = 0; J < NB; ++J)
#pragma unroll
                for (int a = 0; a < d; ++a) {
                  double t = mt[J * d + a];
#pragma unroll
                  for (int jj = J + 1; jj < NB; ++jj) t += P.pc.At[J][jj] * mt[jj * d + a];
                  dl[J * d + a] = pj[J] * xm[J * d + a] - t;  // m^s_+ - m^-
                }
              ODEF_SCHED_FENCE();
              predict_cov_inplace<d, NB>(P.pc, B, sigma2);
              ODEF_SCHED_FENCE();
#pragma unroll
              for (int e = 0; e < TRI; ++e) Cs[e] -= B[e];
              int fixes = 0;
              double dinv[D];
              chol_packed<D>(B, fixes, dinv);
              ODEF_SCHED_FENCE();
#pragma unroll
              for (int a = 0; a < D; ++a) {
                double t = dl[a];
#pragma unroll
                for (int c = 0; c < a; ++c) t -= B[tri(a, c)] * dl[c];
                dl[a] = t * dinv[a];
              }
#pragma unroll
              for (int a = D - 1; a >= 0; --a) {
                double t = dl[a];
#pragma unroll
                for (int c = a + 1; c < D; ++c) t -= B[tri(c, a)] * dl[c];
                dl[a] = t * dinv[a];
              }
              ODEF_SCHED_FENCE();
              two_sided_inverse<D>(Cs, B, dinv);
            }
#pragma unroll
            for (int K = 0; K < NB; ++K)
#pragma unroll
              for (int b = 0; b < d; ++b) {
                double t = dl[K * d + b];
#pragma unroll
                for (int jj = 0; jj < K; ++jj) t += P.pc.At[jj][K] * dl[jj * d + b];
                wv[K * d + b] = t;
              }
            ODEF_SCHED_FENCE();
            congruence_At_inplace<d, NB>(P.pc, Cs);
            ODEF_SCHED_FENCE();
            if (node) {  // observed as (w, W), kept un-preconditioned
              double yv[d];
#pragma unroll
              for (int c = 0; c < d; ++c) {
                const size_t e = (size_t)j * P.o + (slot[c] >= 0 ? slot[c] : 0);
                yv[c] = P.per_traj ? P.obs_val[e * N + i] : P.obs_val[e];
                bad = bad || (slot[c] >= 0 && !(yv[c] == yv[c]));
              }
              datalik_update_node<d, D>(wv, Cs, mt, xl, pij[0], slot, rn, yv, quad, logdet, bad);
#pragma unroll
              for (int e = 0; e < D; ++e) xm[e] = wv[e] * pj[e / d];
#pragma unroll
              for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) xP[tri(a, b)] = Cs[tri(a, b)] * (pj[a / d] * pj[b / d]);
              wform = true;
            } else {
              static_for<0, D>([&](auto ac) {
                constexpr int a = decltype(ac)::value;
                double xa[D], u[D];
#pragma unroll
                for (int c = 0; c < D; ++c) xa[c] = xl.get(symidx(a, c));
                double mnew = mt[a];
#pragma unroll
                for (int c = 0; c < D; ++c) mnew += xa[c] * wv[c];
                xm[a] = mnew * pij[a / d];
#pragma unroll
                for (int c = 0; c < D; ++c) {
                  double t = 0.0;
#pragma unroll
                  for (int kk = 0; kk < D; ++kk) t += xa[kk] * Cs[symidx(kk, c)];
                  u[c] = t;
                }
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                  double t = xa[b];
#pragma unroll
                  for (int kk = 0; kk < D; ++kk) t += u[kk] * xl.get(symidx(kk, b));
                  xP[tri(a, b)] = t * (pij[a / d] * pij[b / d]);
                }
                ODEF_SCHED_FENCE();
              });
              wform = false;
            }
          }
          txi = tt;
        }
        if (j >= 0 && tau == tt) {  // the node (observed in its step), or a save that is an observation time
          if (!node) {
            double yv[d];
#pragma unroll
            for (int c = 0; c < d; ++c) {
              const size_t e = (size_t)j * P.o + (slot[c] >= 0 ? slot[c] : 0);
              yv[c] = P.per_traj ? P.obs_val[e * N + i] : P.obs_val[e];
              bad = bad || (slot[c] >= 0 && !(yv[c] == yv[c]));
            }
            datalik_update<d, D>(xm, xP, slot, rn, yv, quad, logdet, bad);
          }
          --j;
          tau = j >= 0 ? P.obs_time[j] : tau;
          done = j < 0;
        }
        if (!node || done) break;
      }
    }
  }
  if (!valid) return;
  bad = bad || j >= 0;  // observation times below the trajectory's first record
  const double nan = __builtin_nan("");
  const double cnt = (double)M * (double)P.o;
  P.loglik[i] = bad ? nan : -0.5 * (quad + logdet + cnt * 1.8378770664093453);
  P.maha[i] = bad ? nan : quad;
}

#ifndef ODEF_HOST_EMUL
// One wavefront per workgroup; the lane-private copy of the step's filter covariance sits in LDS (TRI x 64 doubles), like
// data_loglik_kernel's.
template <int d, int q>
__global__ __launch_bounds__(kDataLikWave) void data_loglik_times_kernel(const DataLikTimesArgs P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kDataLikWave];
  const long i0 = (long)blockIdx.x * kDataLikWave;
  const LaneMem xl{lds + threadIdx.x, kDataLikWave};
  data_loglik_times_lane<d, q>(P, i0, threadIdx.x, i0 + threadIdx.x < P.N, xl);
}
#endif

}  // namespace odef
