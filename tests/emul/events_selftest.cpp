// TEST INFRASTRUCTURE: stand-alone run of the host build of the event location kernels (emul_events.cpp) for the CPU sanitisers.
// Synthetic records of five shapes -- a sine in every component with its derivatives in the higher blocks, positive definite
// covariances, a zero first record, a repeated time, fixed and adaptive grids with ragged record counts, both sources, all three
// directions, K below and above the count, shared and per-trajectory levels --, every buffer of its exact size, so that
// AddressSanitizer sees any access past one.  Build and run:
//   g++ -O1 -g -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas
//       tests/emul/events_selftest.cpp -o events_selftest && ./events_selftest
// Exit status 0 and "events selftest: ok" when every located time lies in its bracket, no event spent more than 64 evaluations, the
// unused slots hold their fill values and two runs agree bit for bit.  Not part of the product.
#include "emul_events.cpp"

#include <cmath>
#include <cstdio>

namespace {

unsigned long long g_state = 0x9E3779B97F4A7C15ull;
double uniform() {  // in (-1, 1)
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

void prior(int q, double* At, double* Qt, double* QLt) {
  const int nb = q + 1;
  auto fact = [](int n) { double f = 1.0; for (int k = 2; k <= n; ++k) f *= k; return f; };
  for (int k = 0; k < MAXNB * MAXNB; ++k) At[k] = Qt[k] = QLt[k] = 0.0;
  for (int J = 0; J < nb; ++J)
    for (int K = J; K < nb; ++K) At[J * MAXNB + K] = 1.0 / fact(K - J);
  for (int r = 0; r < nb; ++r)
    for (int c = 0; c < nb; ++c) Qt[r * MAXNB + c] = 1.0 / ((2 * q + 1 - r - c) * fact(q - r) * fact(q - c));
  for (int j = 0; j < nb; ++j) {
    double s = Qt[j * MAXNB + j];
    for (int k = 0; k < j; ++k) s -= QLt[j * MAXNB + k] * QLt[j * MAXNB + k];
    QLt[j * MAXNB + j] = std::sqrt(s);
    for (int i = j + 1; i < nb; ++i) {
      double t = Qt[i * MAXNB + j];
      for (int k = 0; k < j; ++k) t -= QLt[i * MAXNB + k] * QLt[j * MAXNB + k];
      QLt[i * MAXNB + j] = t / QLt[j * MAXNB + j];
    }
  }
}

struct Out {
  std::vector<int> count, direction, save, neval;
  std::vector<double> time, tvar, u;
};

bool run_shape(int d, int q, long N, long n_save, bool adaptive, int source, int comp, int dir, int K, bool per_traj, long repeat_at) {
  const int D = d * (q + 1), TRI = D * (D + 1) / 2;
  const double w = 5.0, h = 0.0625;
  std::vector<double> t(adaptive ? (size_t)n_save * N : (size_t)n_save);
  std::vector<int> nsaved(N);
  for (long i = 0; i < N; ++i) nsaved[i] = adaptive ? (int)(n_save - (i % 5)) : (int)n_save;  // ragged record counts
  for (long i = 0; i < (adaptive ? N : 1); ++i) {
    double tt = 0.0;
    for (long k = 0; k < n_save; ++k) {
      if (k > 0 && k != repeat_at) tt += adaptive ? h * (1.0 + 0.3 * uniform()) : h;
      t[adaptive ? (size_t)k * N + i : (size_t)k] = tt;
    }
  }
  std::vector<double> mean[2], cov[2], diff((size_t)n_save * N), F((size_t)D * D);
  for (int s = 0; s < 2; ++s) {
    mean[s].resize((size_t)n_save * D * N);
    cov[s].resize((size_t)n_save * TRI * N);
  }
  for (long i = 0; i < N; ++i) {
    const double phase = 0.3 + 0.01 * (double)i;
    for (long k = 0; k < n_save; ++k) {
      const double tt = t[adaptive ? (size_t)k * N + i : (size_t)k];
      for (int s = 0; s < 2; ++s) {
        for (int J = 0; J <= q; ++J)
          for (int a = 0; a < d; ++a)  // the J-th derivative of sin(w t + phase + a)
            mean[s][((size_t)k * D + J * d + a) * N + i] = std::pow(w, J) * std::sin(w * tt + phase + a + J * 1.5707963267948966) +
                                                            (s ? 1e-4 * uniform() : 0.0);
        for (double& f : F) f = 1e-2 * uniform();
        for (int a = 0; a < D; ++a)
          for (int b = 0; b <= a; ++b) {
            double v = a == b ? 1e-5 : 0.0;
            for (int c = 0; c < D; ++c) v += F[a * D + c] * F[b * D + c];
            cov[s][((size_t)k * TRI + a * (a + 1) / 2 + b) * N + i] = k == 0 ? 0.0 : v;  // the first record: zero covariance
          }
      }
      diff[(size_t)k * N + i] = k == 0 ? 0.0 : 0.5 + 0.4 * uniform();
    }
  }
  std::vector<double> level(per_traj ? N : 1);
  for (double& l : level) l = 0.3 * uniform();
  double At[MAXNB * MAXNB], Qt[MAXNB * MAXNB], QLt[MAXNB * MAXNB];
  prior(q, At, Qt, QLt);
  Out o[2];
  const size_t KN = (size_t)K * N;
  for (Out& r : o) {
    r.count.assign(N, -7);
    r.direction.assign(KN, -7);
    r.save.assign(KN, -7);
    r.neval.assign(KN, -7);
    r.time.assign(KN, -7.0);
    r.tvar.assign(KN, -7.0);
    r.u.assign(KN * d, -7.0);
    if (emul_events(d, q, At, Qt, QLt, mean[0].data(), cov[0].data(), diff.data(), mean[1].data(), cov[1].data(), t.data(), nsaved.data(),
                    adaptive, N, n_save, source, comp, dir, K, level.data(), per_traj, r.count.data(), r.time.data(), r.tvar.data(),
                    r.u.data(), r.direction.data(), r.save.data(), r.neval.data()))
      return false;
  }
  bool ok = true;
  long total = 0, worst = 0;
  for (long i = 0; i < N; ++i) {
    ok = ok && o[0].count[i] >= 0 && o[0].count[i] < nsaved[i];
    total += o[0].count[i];
    for (int s = 0; s < K; ++s) {
      const size_t e = (size_t)s * N + i;
      if (s < o[0].count[i]) {
        const long k = o[0].save[e];
        ok = ok && k >= 0 && k + 1 < nsaved[i];
        if (!ok) break;
        const double ta = t[adaptive ? (size_t)k * N + i : (size_t)k], tb = t[adaptive ? (size_t)(k + 1) * N + i : (size_t)(k + 1)];
        ok = ok && tb > ta && o[0].time[e] >= ta && o[0].time[e] <= tb && o[0].neval[e] >= 0 && o[0].neval[e] <= kEventMaxEval &&
             (o[0].direction[e] == 1 || o[0].direction[e] == -1) && (dir == 0 || o[0].direction[e] == dir) && !(o[0].tvar[e] < 0.0);
        worst = std::max(worst, (long)o[0].neval[e]);
        for (int a = 0; a < d; ++a) ok = ok && std::isfinite(o[0].u[((size_t)s * d + a) * N + i]);
      } else {
        ok = ok && o[0].save[e] == -1 && o[0].direction[e] == 0 && o[0].neval[e] == 0 && std::isnan(o[0].time[e]) &&
             std::isnan(o[0].tvar[e]);
        for (int a = 0; a < d; ++a) ok = ok && std::isnan(o[0].u[((size_t)s * d + a) * N + i]);
      }
    }
  }
  ok = ok && o[0].count == o[1].count && o[0].direction == o[1].direction && o[0].save == o[1].save && o[0].neval == o[1].neval &&
       std::memcmp(o[0].time.data(), o[1].time.data(), KN * 8) == 0 && std::memcmp(o[0].tvar.data(), o[1].tvar.data(), KN * 8) == 0 &&
       std::memcmp(o[0].u.data(), o[1].u.data(), KN * d * 8) == 0;
  std::printf("(d, q) = (%d, %d) N = %ld n_save = %ld %s source %d c = %d dir = %d K = %d %s: %ld brackets, most evaluations %ld %s\n", d,
              q, N, n_save, adaptive ? "adaptive" : "fixed", source, comp, dir, K, per_traj ? "per trajectory" : "shared", total, worst,
              ok && total > 0 ? "ok" : "FAILED");
  return ok && total > 0;
}

}  // namespace

int main() {
  bool ok = true;
  ok = run_shape(1, 1, 1, 40, false, 0, 0, 0, 2, false, -1) && ok;
  ok = run_shape(2, 3, 65, 33, false, 1, 1, 1, 1, true, 7) && ok;
  ok = run_shape(3, 3, 130, 29, true, 1, 2, -1, 4, false, 5) && ok;
  ok = run_shape(2, 5, 3, 21, true, 0, 0, 0, 6, true, -1) && ok;
  ok = run_shape(4, 2, 67, 19, false, 0, 3, 0, 3, false, 2) && ok;
  std::printf("events selftest: %s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
