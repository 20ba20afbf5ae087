// TEST INFRASTRUCTURE: stand-alone run of the host build of the kernel of the data log-likelihood at arbitrary times
// (emul_datalik_times.cpp) for the CPU sanitisers.  Synthetic records of five shapes -- N = 1, 63, 65, fixed and ragged grids with
// a repeated time, record counts of 0, of 1 and above the capacity, shared and per-trajectory values, o < d and o = d, times on
// saves, between them, several in one step and above a lane's last record --, every buffer of its exact size, so that
// AddressSanitizer sees any access past one.  Build and run:
//   g++ -O1 -g -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas
//       tests/emul/datalik_times_selftest.cpp -o datalik_times_selftest && ./datalik_times_selftest
// Exit status 0 and "datalik times selftest: ok" when every lane whose records cover the times gives a finite result, every other
// lane NaN, and two runs -- every lane its own wavefront, and wavefronts of 64 with lanes that join later -- agree bit for bit.  Not part of the product.
#include "emul_datalik_times.cpp"

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

// ragged: lane i holds n_save - (i % 4) records, lane 1 none, lane 2 one, lane 3 claims more than the capacity; its times are its own
bool run_shape(int d, int q, long N, long n_save, const std::vector<double>& frac, const std::vector<long long>& comps, bool per_traj,
               bool ragged, long repeat_at) {
  const int D = d * (q + 1), TRI = D * (D + 1) / 2;
  const int M = (int)frac.size(), o = (int)comps.size();
  std::vector<double> mean((size_t)n_save * D * N), cov((size_t)n_save * TRI * N), diff((size_t)n_save * N);
  std::vector<double> tgrid(ragged ? 0 : n_save), tsave(ragged ? (size_t)n_save * N : 0);
  std::vector<int> nsaved(ragged ? N : 0);
  const double t_end = 0.0625 * (n_save - 1 - (repeat_at > 0 ? 1 : 0));
  std::vector<bool> covered(N, true);
  std::vector<double> times(M);
  for (int j = 0; j < M; ++j) times[j] = frac[j] * t_end;  // frac 1: the last save of the full grid
  for (long i = 0; i < N; ++i) {
    long n = n_save;
    double scale = 1.0;
    if (ragged) {
      n = i == 1 ? 0 : i == 2 ? 1 : n_save - (i % 4);
      nsaved[i] = i == 3 ? (int)n_save + 5 : (int)n;  // (clamped to the capacity by the kernel)
      scale = i % 4 == 0 || i == 3 ? 1.0 : 1.0 + 0.01 * (double)(i % 7);  // its own step size; lanes 0, 4, .. and 3 keep the grid
    }
    double t = 0.0;
    for (long k = 0; k < n_save; ++k) {
      if (k > 0) t += k == repeat_at ? 0.0 : 0.0625 * scale;
      if (ragged) tsave[(size_t)k * N + i] = t;
      else tgrid[k] = t;
      if (k == (ragged && i != 3 ? n : n_save) - 1) covered[i] = t >= times[M - 1];
    }
    if (ragged && n < 1) covered[i] = false;
  }
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
    if (emul_datalik_times(d, q, At, Qt, QLt, mean.data(), cov.data(), diff.data(), ragged, ragged ? nullptr : tgrid.data(),
                           ragged ? tsave.data() : nullptr, ragged ? nsaved.data() : nullptr, N, n_save, times.data(), M, comps.data(), o,
                           val.data(), per_traj, noise.data(), rep ? 64 : 1, ll[rep].data(), mq[rep].data()))
      return false;
  }
  bool ok = true;
  long n_nan = 0;
  for (long i = 0; i < N; ++i) {
    const bool fin = std::isfinite(ll[0][i]) && std::isfinite(mq[0][i]) && mq[0][i] >= 0.0;
    const bool nan = std::isnan(ll[0][i]) && std::isnan(mq[0][i]);
    n_nan += nan;
    ok = ok && (covered[i] ? fin : nan) && std::memcmp(&ll[0][i], &ll[1][i], 8) == 0 && std::memcmp(&mq[0][i], &mq[1][i], 8) == 0;
  }
  std::printf("(d, q) = (%d, %d) N = %ld n_save = %ld M = %d o = %d %s %s: loglik[0] = %.15g, %ld lanes NaN %s\n", d, q, N, n_save, M, o,
              per_traj ? "per trajectory" : "shared", ragged ? "ragged" : "fixed", ll[0][0], n_nan, ok ? "ok" : "FAILED");
  return ok;
}

}  // namespace

int main() {
  bool ok = true;
  ok = run_shape(1, 1, 1, 5, {0.0, 0.3, 0.35, 0.5, 1.0}, {0}, false, false, -1) && ok;
  ok = run_shape(2, 3, 63, 9, {0.0, 0.26, 0.27, 0.28, 0.9}, {0, 1}, true, true, 3) && ok;
  ok = run_shape(3, 3, 65, 12, {0.41, 0.42, 1.0}, {0, 2}, false, true, -1) && ok;
  ok = run_shape(2, 5, 65, 6, {0.999, 1.0}, {1}, true, false, 2) && ok;
  ok = run_shape(4, 2, 63, 7, {0.01, 0.02, 0.03}, {1, 3}, false, true, -1) && ok;
  std::printf("datalik times selftest: %s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
