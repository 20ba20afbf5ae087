// Device source of the event location pass (events.hip launches it; tests/emul/emul_events.cpp builds the same text for the host to
// check it without a GPU): the times at which component c of the posterior mean crosses a level, per trajectory.
//
//   event_scan_kernel          one lane per trajectory, not templated: walks row c of the mean records forward, counts the sign
//                              changes of g_k = m_c[k] - level (the brackets) and keeps the left save and the direction of the
//                              first K.  Reads 8 bytes per trajectory and save (16 after an adaptive solve: the save times), never
//                              a covariance.  The walk is a pure stream -- a save's test needs its predecessor only --, so
//                              kEventScanAhead rows are loaded before the first of them is compared.
//   event_refine_kernel<d, q>  blockIdx.y = slot, one lane per trajectory: the root of E[u_c(t)] - level inside the bracket by
//                              bracketed Newton on the dense posterior mean.  The state carries u', so the slope is entry d + c of
//                              the same evaluation.  The evaluation at a per-lane time (event_eval) follows dense_lane
//                              (dense_lane.h) operation by operation and returns in registers.
//
// The pass needs no vector field: the kernels depend on (d, q) alone.
#pragma once
#include "dense_lane.h"

namespace odef {

constexpr int kEventWave = 64;
constexpr int kEventMaxD = 4;        // state components
constexpr int kEventMaxState = 12;   // d (q + 1): what the lane dense output serves
constexpr int kEventMaxEval = 64;    // dense evaluations per event; at the cap the current iterate is returned
constexpr int kEventScanAhead = 8;   // rows in flight per lane in the scan
constexpr double kEventStepTol = 0x1p-40;  // Newton stops at a step of this share of the bracket

struct EventArgs {
  PriorConsts pc;
  long N, n_save;          // fixed grid: number of saves; adaptive: capacity
  int adaptive, source;    // source 0: filter posterior, 1: smoothed
  int comp, dir, K;        // component 0 .. d - 1, direction -1 / 0 / +1, slots per trajectory
  int D;                   // d (q + 1): the row stride of the mean records (the scan is not templated)
  int level_per_traj;
  const double* tgrid;     // fixed: [n_save]
  const double* tsave;     // adaptive: [n_save][N]
  const int* nsaved;       // adaptive: [N]
  const double* mean;      // filter records, ABI layout
  const double* cov;
  const double* diff;
  const double* smean;     // smoothed records (source 1)
  const double* scov;
  const double* level;     // [1] or [N]
  int* count;              // [N]
  double* time;            // [K][N]
  double* tvar;            // [K][N]
  double* u;               // [K][d][N]
  int* direction;          // [K][N]
  int* save;               // [K][N]
  int* neval;              // [K][N]
};

// The scan of one trajectory.  `n_hi`: wave-uniform upper bound of the record counts of the wavefront (fixed grid: n_save), so that
// every load of a row is the same save for all lanes: 512 contiguous bytes.
__device__ ODEF_FORCE_INLINE void event_scan_lane(const EventArgs& P, long i, long n_hi) {
  const size_t N = (size_t)P.N;
  const long n = P.adaptive ? (long)P.nsaved[i] : P.n_save;
  const double* row = (P.source ? P.smean : P.mean) + (size_t)P.comp * N + (size_t)i;  // save k at row[k D N]
  const size_t rs = (size_t)P.D * N;
  const double lvl = P.level_per_traj ? P.level[i] : uniform_load(P.level);
  const int K = P.K, dir = P.dir;
  int cnt = 0;
  double gp = 0.0, tp = 0.0;  // save k - 1
  bool have = false;
  auto test = [&](long k, double m, double t) {
    const double g = m - lvl;
    if (have && k < n && t > tp) {  // (a NaN makes every comparison false: no event)
      const bool up = gp < 0.0 && g >= 0.0, down = gp > 0.0 && g <= 0.0;
      if ((up && dir >= 0) || (down && dir <= 0)) {
        if (cnt < K) {
          P.save[(size_t)cnt * N + i] = (int)(k - 1);
          P.direction[(size_t)cnt * N + i] = up ? 1 : -1;
        }
        ++cnt;
      }
    }
    if (k < n) {
      gp = g;
      tp = t;
      have = true;
    }
  };
  long k = 0;
  for (; k + kEventScanAhead <= n_hi; k += kEventScanAhead) {
    double m[kEventScanAhead], t[kEventScanAhead];
#pragma unroll
    for (int a = 0; a < kEventScanAhead; ++a) {  // every load of the chunk in flight before the first compare
      m[a] = row[(size_t)(k + a) * rs];
      t[a] = P.adaptive ? P.tsave[(size_t)(k + a) * N + i] : uniform_load(P.tgrid + k + a);
    }
    ODEF_SCHED_FENCE();
#pragma unroll
    for (int a = 0; a < kEventScanAhead; ++a) test(k + a, m[a], t[a]);
  }
  for (; k < n_hi; ++k) test(k, row[(size_t)k * rs], P.adaptive ? P.tsave[(size_t)k * N + i] : uniform_load(P.tgrid + k));
  P.count[i] = cnt;
  for (int s = cnt; s < K; ++s) {  // unused slots
    P.save[(size_t)s * N + i] = -1;
    P.direction[(size_t)s * N + i] = 0;
  }
}

// entry `c` (a run-time index) of a register array, by selection: every index stays a compile-time constant
template <int n, int lo, int cnt>
__device__ ODEF_FORCE_INLINE double event_pick(const double (&v)[n], int c) {
  double r = v[lo];
#pragma unroll
  for (int a = 1; a < cnt; ++a) r = (a == c) ? v[lo + a] : r;
  return r;
}

// The dense posterior of trajectory i at its own time t inside the step k -> k + 1 (t_k <= t <= t_{k+1}), with the semantics and the
// arithmetic of dense_lane: a stored time gives the stored record; otherwise predict from the left filter record with P(h1) and,
// for source 1, one RTS step against the right smoothed record with P(h2).  Out: the mean m (un-preconditioned) and var = Sigma_cc.
// `with_cov` false (source 0 only): the mean alone -- P(h)^-1 A P(h) m_k, no covariance is read or formed -- and var is left as it is.
// `limit` (source 0, mean alone): the prediction itself at t = t_{k+1}, i.e. the left limit of the filter's interpolant at the save,
// not the stored record -- the two differ by the measurement update.
template <int d, int q>
__device__ ODEF_FORCE_INLINE void event_eval(const EventArgs& P, long i, long k, double tk, double tk1, double t, bool with_cov,
                                             bool limit, const LaneMem& xl, double (&m)[d * (q + 1)], double& var) {
  constexpr int NB = q + 1, D = d * NB, TRI = D * (D + 1) / 2;
  const size_t N = (size_t)P.N;
  const int c = P.comp;
  const bool sm = P.source != 0;
  if ((t == tk || t == tk1) && !limit) {  // exactly a stored time (src/solution.jl:172-176)
    const size_t s = t == tk1 ? (size_t)(k + 1) : (size_t)k;
    const double* pm = (sm ? P.smean : P.mean) + (s * D) * N + i;
    const double* pc = (sm ? P.scov : P.cov) + (s * TRI) * N + i;
#pragma unroll
    for (int e = 0; e < D; ++e) m[e] = pm[(size_t)e * N];
    if (with_cov) {
      double v = pc[(size_t)tri(0, 0) * N];
#pragma unroll
      for (int a = 1; a < d; ++a) v = (a == c) ? pc[(size_t)tri(a, a) * N] : v;
      var = v;
    }
    return;
  }
  const double h1 = t - tk;
  double pj1[NB], pij1[NB];
  precond_from_h<q>(h1, pj1, pij1);
  double mt[D];
#pragma unroll
  for (int e = 0; e < D; ++e) mt[e] = pj1[e / d] * P.mean[((size_t)k * D + e) * N + i];
  double mp[D];
#pragma unroll
  for (int J = 0; J < NB; ++J)
#pragma unroll
    for (int a = 0; a < d; ++a) {
      double s = mt[J * d + a];
#pragma unroll
      for (int j = J + 1; j < NB; ++j) s += P.pc.At[J][j] * mt[j * d + a];
      mp[J * d + a] = s;
    }
  if (!with_cov || limit) {
#pragma unroll
    for (int e = 0; e < D; ++e) m[e] = pij1[e / d] * mp[e];
    return;
  }
  // diffusions[min(idx, end)] (src/solution.jl:181): slot k + 1 holds the diffusion of the step k -> k + 1
  const double sigma2 = load_sig<d, false>(P.diff, (size_t)(k + 1), N, (size_t)i);
  double B[TRI];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) B[tri(a, b)] = P.cov[((size_t)k * TRI + tri(a, b)) * N + i] * (pj1[a / d] * pj1[b / d]);
  predict_cov_inplace<d, NB>(P.pc, B, sigma2);
  if (!sm) {
#pragma unroll
    for (int e = 0; e < D; ++e) m[e] = pij1[e / d] * mp[e];
    double v = B[tri(0, 0)];
#pragma unroll
    for (int a = 1; a < d; ++a) v = (a == c) ? B[tri(a, a)] : v;
    var = v * (pij1[0] * pij1[0]);
    return;
  }
  // smooth against the smoothed record k + 1 with P(h2)  (src/solution.jl:199-209)
  const double h2 = tk1 - t;
  double pj2[NB], pij2[NB];
  precond_from_h<q>(h2, pj2, pij2);
  double msn[D], Cs[TRI];
#pragma unroll
  for (int e = 0; e < D; ++e) {
    mt[e] = pj2[e / d] * (pij1[e / d] * mp[e]);
    msn[e] = pj2[e / d] * P.smean[((size_t)(k + 1) * D + e) * N + i];
  }
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const double x = (B[tri(a, b)] * (pij1[a / d] * pij1[b / d])) * (pj2[a / d] * pj2[b / d]);
      B[tri(a, b)] = x;
      xl.set(tri(a, b), x);
      Cs[tri(a, b)] = P.scov[((size_t)(k + 1) * TRI + tri(a, b)) * N + i] * (pj2[a / d] * pj2[b / d]);
    }
  double dv[d];  // the diagonal of the d x d solution block, entry by entry as the core hands the covariance out
#pragma unroll
  for (int a = 0; a < d; ++a) dv[a] = 0.0;
  auto sink = [&](int e, double v) {
#pragma unroll
    for (int a = 0; a < d; ++a)
      if (e == tri(a, a)) dv[a] = v;
  };
  ODEF_INLINE_CALL rts_step_core<d, NB>(P.pc, pij2, mt, B, Cs, msn, sigma2, xl, m, sink);
  var = event_pick<d, 0, d>(dv, c);
}

// One slot of one trajectory: fill values without an event, the stored record for an exact hit or a crossing inside the update, else
// the root.  One call site of event_eval serves all of it (the step core at D = 12 is inlined once): `stage` says what the next
// evaluation is.
//   source 0 only, first: the LEFT LIMIT of the interpolant at t_{k+1}.  The filter's dense mean is the prediction from save k; at
//   t_{k+1} it jumps by the measurement update to the stored record.  A bracket of the stored means whose prediction has not passed
//   the level by t_{k+1} has no root inside: the crossing happens in the update, the event is the save t_{k+1} and the outputs are
//   its stored record.  Otherwise the left limit, not the stored mean, is the right end of the secant.  (The smoothed interpolant is
//   continuous at the saves.)
template <int d, int q>
__device__ ODEF_FORCE_INLINE void event_refine_lane(const EventArgs& P, long i, long slot, const LaneMem& xl) {
  constexpr int NB = q + 1, D = d * NB;
  static_assert(d <= kEventMaxD && D <= kEventMaxState, "event location: d <= 4, d (q + 1) <= 12");
  const size_t N = (size_t)P.N, o = (size_t)slot * N + (size_t)i;
  const int c = P.comp;
  const double nan = __builtin_nan("");
  double* uo = P.u + ((size_t)slot * d) * N + i;
  const long k = (long)P.save[o];
  if (k < 0) {
    P.time[o] = nan;
    P.tvar[o] = nan;
#pragma unroll
    for (int a = 0; a < d; ++a) uo[(size_t)a * N] = nan;
    P.neval[o] = 0;
    return;
  }
  const double tk = P.adaptive ? P.tsave[(size_t)k * N + i] : P.tgrid[k];
  const double tk1 = P.adaptive ? P.tsave[(size_t)(k + 1) * N + i] : P.tgrid[k + 1];
  const double lvl = P.level_per_traj ? P.level[i] : uniform_load(P.level);
  const double* row = (P.source ? P.smean : P.mean) + (size_t)c * N + (size_t)i;
  const double ga0 = row[(size_t)k * D * N] - lvl;
  const double gb0 = row[(size_t)(k + 1) * D * N] - lvl;
  const bool src1 = P.source != 0;
  const bool neg = ga0 < 0.0;  // the sign of g at the left end
  const double tol = kEventStepTol * (tk1 - tk);
  enum { kLimit, kIterate, kOutputs };
  double m[D], var = nan;
  double a = tk, b = tk1, x;
  int neval = 0, last_counts = 0, stage;
  if (gb0 == 0.0) {  // the crossing is the save itself: every output is the stored record
    stage = kOutputs;
    x = tk1;
  } else if (src1) {
    stage = kIterate;
    x = a - ga0 * ((b - a) / (gb0 - ga0));  // the secant point of the bracket's ends
    if (!(x >= a && x <= b)) x = 0.5 * (a + b);
  } else {
    stage = kLimit;
    x = tk1;
  }
  for (;;) {
    // source 0 iterates on the mean alone; its covariance is formed once, at the accepted time
    event_eval<d, q>(P, i, k, tk, tk1, x, stage == kOutputs || (src1 && stage == kIterate), stage == kLimit, xl, m, var);
    if (stage == kOutputs) {
      neval += last_counts;
      break;
    }
    ++neval;
    const double g = event_pick<D, 0, d>(m, c) - lvl;
    const double s = event_pick<D, d, d>(m, c);
    if (stage == kLimit) {
      if (!(neg ? g > 0.0 : g < 0.0)) {  // not passed by t_{k+1}: the crossing is inside the update, the stored record answers
        stage = kOutputs;
        continue;
      }
      x = a - ga0 * ((b - a) / (g - ga0));
      if (!(x >= a && x <= b)) x = 0.5 * (a + b);
      stage = kIterate;
      continue;
    }
    if (g == 0.0 || neval >= kEventMaxEval) {
      if (src1) break;
      stage = kOutputs;  // the same time once more, with the covariance: no new evaluation point
      continue;
    }
    if ((g < 0.0) == neg) a = x;
    else b = x;
    double xn = x - g / s;
    // a zero or non-finite slope, or an iterate outside the CLOSED bracket (a converged iterate may equal an end): the midpoint
    if (!(s != 0.0 && s - s == 0.0) || !(xn >= a && xn <= b)) xn = 0.5 * (a + b);
    if (__builtin_fabs(xn - x) <= tol) {  // converged: accepted before any interior test; the outputs come from this time
      stage = kOutputs;
      last_counts = 1;
    }
    x = xn;
  }
  const double s = event_pick<D, d, d>(m, c);
  P.time[o] = x;
  P.tvar[o] = var / (s * s);  // plain IEEE: a zero slope gives inf
#pragma unroll
  for (int a_ = 0; a_ < d; ++a_) uo[(size_t)a_ * N] = m[a_];
  P.neval[o] = neval;
}

#ifndef ODEF_HOST_EMUL
__global__ __launch_bounds__(kEventWave) void event_scan_kernel(const EventArgs P) {
  const long i = (long)blockIdx.x * kEventWave + threadIdx.x;
  const bool valid = i < P.N;
  long n_hi = P.n_save;
  if (P.adaptive) n_hi = wave_uniform_max(valid ? (long)P.nsaved[i] : 0, valid);
  if (valid) event_scan_lane(P, i, n_hi);
}

// One wavefront per workgroup; the lane-private copy of the interpolated filter covariance sits in LDS (TRI x 64 doubles), like the
// dense output's.
template <int d, int q>
__global__ __launch_bounds__(kEventWave) void event_refine_kernel(const EventArgs P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kEventWave];
  const long i = (long)blockIdx.x * kEventWave + threadIdx.x;
  const LaneMem xl{lds + threadIdx.x, kEventWave};
  if (i < P.N) event_refine_lane<d, q>(P, i, (long)blockIdx.y, xl);
}
#endif

}  // namespace odef
