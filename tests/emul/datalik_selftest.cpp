// TEST INFRASTRUCTURE: stand-alone run of the host build of the data log-likelihood kernel (emul_datalik.cpp) for the CPU
// sanitisers.  Synthetic records of a few shapes -- positive definite covariances, a zero first record, a repeated time, shared and
// per-trajectory values, o < d and o = d, observations at the first, last and interior saves --, every buffer of its exact size, so
// that AddressSanitizer sees any access past one.  Build and run:
//   g++ -O1 -g -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas
//       tests/emul/datalik_selftest.cpp -o datalik_selftest && ./datalik_selftest
// Exit status 0 and "datalik selftest: ok" when every result is finite and two runs agree bit for bit.  Not part of the product.
#include "emul_datalik.cpp"

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

bool run_shape(int d, int q, long N, long n_save, const std::vector<long long>& saves, const std::vector<long long>& comps, bool per_traj,
               long repeat_at) {
  const int D = d * (q + 1), TRI = D * (D + 1) / 2;
  const int M = (int)saves.size(), o = (int)comps.size();
  std::vector<double> mean((size_t)n_save * D * N), cov((size_t)n_save * TRI * N), diff((size_t)n_save * N), t(n_save);
  for (long k = 0; k < n_save; ++k) t[k] = k == 0 ? 0.0 : t[k - 1] + (k == repeat_at ? 0.0 : 0.0625);
  std::vector<double> F((size_t)D * D);
  for (long k = 0; k < n_save; ++k)
    for (long i = 0; i < N; ++i) {
      for (int a = 0; a < D; ++a) mean[((size_t)k * D + a) * N + i] = uniform();
      for (double& f : F) f = 1e-2 * uniform();
      for (int a = 0; a < D; ++a)
        for (int b = 0; b <= a; ++b) {
          double s = a == b ? 1e-5 : 0.0;
          for (int c = 0; c < D; ++c) s += F[a * D + c] * F[b * D + c];
          cov[((size_t)k * TRI + a * (a + 1) / 2 + b) * N + i] = k == 0 ? 0.0 : s;  // the first record: zero covariance
        }
      diff[(size_t)k * N + i] = k == 0 ? 0.0 : 0.5 + 0.4 * uniform();
    }
  std::vector<double> val((size_t)M * o * (per_traj ? N : 1)), noise(o);
  for (double& v : val) v = uniform();
  for (double& r : noise) r = 1e-3 * (1.5 + uniform());
  double At[MAXNB * MAXNB], Qt[MAXNB * MAXNB], QLt[MAXNB * MAXNB];
  prior(q, At, Qt, QLt);
  std::vector<double> ll[2], mq[2];
  for (int rep = 0; rep < 2; ++rep) {
    ll[rep].assign(N, -7.0);
    mq[rep].assign(N, -7.0);
    if (emul_datalik(d, q, At, Qt, QLt, mean.data(), cov.data(), diff.data(), t.data(), N, n_save, saves.data(), M, comps.data(), o,
                     val.data(), per_traj, noise.data(), ll[rep].data(), mq[rep].data()))
      return false;
  }
  bool ok = true;
  for (long i = 0; i < N; ++i)
    ok = ok && std::isfinite(ll[0][i]) && mq[0][i] >= 0.0 && std::isfinite(mq[0][i]) &&
         std::memcmp(&ll[0][i], &ll[1][i], 8) == 0 && std::memcmp(&mq[0][i], &mq[1][i], 8) == 0;
  std::printf("(d, q) = (%d, %d) N = %ld n_save = %ld M = %d o = %d %s: loglik[0] = %.15g %s\n", d, q, N, n_save, M, o,
              per_traj ? "per trajectory" : "shared", ll[0][0], ok ? "ok" : "FAILED");
  return ok;
}

}  // namespace

int main() {
  bool ok = true;
  ok = run_shape(1, 1, 1, 5, {0, 1, 2, 3, 4}, {0}, false, -1) && ok;
  ok = run_shape(2, 3, 65, 9, {0, 4, 8}, {0, 1}, true, 3) && ok;
  ok = run_shape(3, 3, 130, 12, {5}, {0, 2}, false, -1) && ok;
  ok = run_shape(3, 5, 3, 6, {5}, {0, 1, 2}, true, -1) && ok;
  ok = run_shape(4, 4, 2, 5, {0, 2, 4}, {1, 3}, false, 2) && ok;
  std::printf("datalik selftest: %s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
