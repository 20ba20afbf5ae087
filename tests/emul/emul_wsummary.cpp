// TEST INFRASTRUCTURE: host build of the weighted ensemble-summary reduction (csrc/wsummary_kernels.h, the text the GPU runs) in
// the launch sequence of wsummary.hip, so that its indexing, its inclusion rule and its arithmetic can be checked against
// tests/_wsummary_reference.py without a GPU.  One host thread per lane of a wavefront; __shfl_xor is an exchange through a
// 64-slot array between two barriers, so the butterfly adds in the order of the device.  Wavefronts run one after the other (the
// kernels have no workgroup barrier and no lane reads another lane's LDS column), so the one atomicMax is a plain maximum.  With
// -DODEF_EMUL_MAIN the file has its own main(): the stand-alone program of the sanitizer run.  Not part of the product.
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__

namespace {
struct Idx { unsigned x; };
thread_local Idx threadIdx, blockIdx, blockDim, gridDim;
double* g_lds;
std::barrier<>* g_bar;
double g_xd[64];
int g_xi[64];
double __shfl_xor(double v, int m, int) {
  const int l = threadIdx.x % 64;
  g_xd[l] = v;
  g_bar->arrive_and_wait();
  const double r = g_xd[l ^ m];
  g_bar->arrive_and_wait();
  return r;
}
int __shfl_xor(int v, int m, int) {
  const int l = threadIdx.x % 64;
  g_xi[l] = v;
  g_bar->arrive_and_wait();
  const int r = g_xi[l ^ m];
  g_bar->arrive_and_wait();
  return r;
}
int __popc(unsigned x) { return __builtin_popcount(x); }
// one lane of a wavefront calls it, and the wavefronts run one after the other
unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
  const unsigned long long old = *p;
  if (v > old) *p = v;
  return old;
}
}  // namespace

#define ODEF_WSUMMARY_TILE double* tile = g_lds
#include "../../odefilters.jl_amd/csrc/wsummary_kernels.h"

using namespace odef;

namespace {
template <class F>
void run_grid(unsigned n_blocks, F f) {
  for (unsigned b = 0; b < n_blocks; ++b)
    for (unsigned w = 0; w < 256 / 64; ++w) {
      std::barrier<> bar(64);
      g_bar = &bar;
      std::vector<std::thread> lanes;
      for (unsigned l = 0; l < 64; ++l)
        lanes.emplace_back([=] {
          threadIdx.x = w * 64 + l;
          blockIdx.x = b;
          blockDim.x = 256;
          gridDim.x = n_blocks;
          f();
        });
      for (auto& t : lanes) t.join();
    }
}

// kernels whose lanes are independent: no thread per lane needed
template <class F>
void run_flat(unsigned n_blocks, unsigned block, F f) {
  for (unsigned b = 0; b < n_blocks; ++b)
    for (unsigned t = 0; t < block; ++t) {
      threadIdx.x = t;
      blockIdx.x = b;
      blockDim.x = block;
      gridDim.x = n_blocks;
      f();
    }
}

template <int K>
void run(const double* mean, const double* cov, const int* rc, const double* logw, long N, long n_t, int d, int D, int TRI,
         int max_blocks, long long* count, double* m, double* within, double* between, double* logev, double* ess) {
  const int tri = d * (d + 1) / 2, R = 2 + d + tri;
  const int n_block = (int)((N + 256L * K - 1) / (256L * K)), n_wave = n_block * 4;
  const long n_flat = (N + 255) / 256;
  // exact-size buffers: the sanitiser build sees any access past the tile, the partials, the weights or the records
  std::vector<double> part((size_t)n_t * n_wave * R), lds((size_t)d * K * 256), v((size_t)N), zsum((size_t)n_t);
  std::vector<int> part_cnt((size_t)n_t * n_wave);
  std::vector<unsigned long long> key(1, 0ull);
  g_lds = lds.data();
  run_grid((unsigned)(n_flat < max_blocks ? n_flat : max_blocks), [&] { wsummary_max_kernel(logw, rc, N, key.data()); });
  run_flat((unsigned)n_flat, 256, [&] { wsummary_weights_kernel(logw, rc, N, key.data(), v.data()); });
  run_grid(n_block * n_t,
           [&] { wsummary_sums_kernel<K>(mean, cov, rc, v.data(), N, d, D, TRI, n_wave, part.data(), part_cnt.data()); });
  run_flat((unsigned)n_t, 64, [&] {
    wsummary_fold_kernel(part.data(), part_cnt.data(), n_wave, d, tri, key.data(), count, zsum.data(), m, within, logev, ess);
  });
  part.assign((size_t)n_t * n_wave * tri, 0.0);
  run_grid(n_block * n_t, [&] { wsummary_centred_kernel<K>(mean, rc, v.data(), m, N, d, D, n_wave, part.data()); });
  run_flat((unsigned)n_t, 64, [&] { wsummary_fold_centred_kernel(part.data(), n_wave, tri, zsum.data(), between); });
}
}  // namespace

// records mean [n_t][D][N], cov [n_t][TRI][N], retcode [N], log-weights [N] -> count [n_t], m [n_t][d], within / between
// [n_t][tri(d)], log evidence and ess [n_t].  max_blocks: the cap on the grid of the maximum kernel (1024 in wsummary.hip; a
// small one makes its lanes stride).
extern "C" int emul_wsummary(int K, const double* mean, const double* cov, const int* rc, const double* logw, long N, long n_t, int d,
                             int D, int TRI, int max_blocks, long long* count, double* m, double* within, double* between,
                             double* logev, double* ess) {
  switch (K) {
    case 8: run<8>(mean, cov, rc, logw, N, n_t, d, D, TRI, max_blocks, count, m, within, between, logev, ess); return 0;
    case 4: run<4>(mean, cov, rc, logw, N, n_t, d, D, TRI, max_blocks, count, m, within, between, logev, ess); return 0;
    case 2: run<2>(mean, cov, rc, logw, N, n_t, d, D, TRI, max_blocks, count, m, within, between, logev, ess); return 0;
    case 1: run<1>(mean, cov, rc, logw, N, n_t, d, D, TRI, max_blocks, count, m, within, between, logev, ess); return 0;
    default: return -1;
  }
}

#ifdef ODEF_EMUL_MAIN
// Stand-alone run for the sanitizers: every K on ragged shapes with dropped trajectories, non-finite weights, underflowing
// weights and an empty time; checks only what needs no reference (counts, NaN rows, sum of weights) and prints "clean".
namespace {
unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
double uniform() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_seed >> 11) * 0x1.0p-53;
}

int one(int K, long N, long n_t, int d, int D) {
  const int TRI = D * (D + 1) / 2, tri = d * (d + 1) / 2;
  std::vector<double> mean((size_t)n_t * D * N), cov((size_t)n_t * TRI * N), logw((size_t)N);
  std::vector<int> rc((size_t)N, 0);
  for (double& x : mean) x = 2.0 * uniform() - 1.0;
  for (double& x : cov) x = uniform();
  for (double& x : logw) x = -900.0 * uniform();
  long dropped = 0;
  if (N > 10) {
    rc[7] = 3;
    logw[2] = std::numeric_limits<double>::quiet_NaN();
    logw[5] = std::numeric_limits<double>::infinity();
    logw[9] = -std::numeric_limits<double>::infinity();
    dropped = 4;
  }
  if (n_t > 1)
    for (long i = 0; i < N; ++i) mean[((size_t)(n_t - 1) * D + (d - 1)) * N + i] = std::numeric_limits<double>::quiet_NaN();
  std::vector<long long> count((size_t)n_t, -7);
  std::vector<double> m((size_t)n_t * d), within((size_t)n_t * tri), between((size_t)n_t * tri), logev((size_t)n_t), ess((size_t)n_t);
  if (emul_wsummary(K, mean.data(), cov.data(), rc.data(), logw.data(), N, n_t, d, D, TRI, 2, count.data(), m.data(), within.data(),
                    between.data(), logev.data(), ess.data()))
    return 1;
  for (long s = 0; s < n_t; ++s) {
    const bool empty = n_t > 1 && s == n_t - 1;
    if (count[s] != (empty ? 0 : N - dropped)) return 2;
    if (empty != std::isnan(m[(size_t)s * d]) || empty != std::isnan(ess[s]) || empty != std::isnan(logev[s])) return 3;
    if (!empty && !(ess[s] >= 1.0 - 1e-12 && ess[s] <= (double)count[s] * (1.0 + 1e-12))) return 4;
    for (int a = 0; !empty && a < d; ++a)
      if (!(std::fabs(m[(size_t)s * d + a]) <= 1.0)) return 5;  // a convex combination of values in [-1, 1]
  }
  return 0;
}
}  // namespace

int main() {
  const struct { int K; long N, n_t; int d, D; } cases[] = {
      {1, 1, 1, 2, 4}, {1, 65, 2, 28, 28}, {2, 513, 2, 16, 32}, {2, 300, 3, 10, 20}, {4, 1030, 2, 3, 12}, {8, 2500, 2, 2, 4}, {8, 63, 3, 3, 3},
  };
  for (const auto& c : cases)
    if (const int r = one(c.K, c.N, c.n_t, c.d, c.D)) {
      std::printf("FAILED K=%d N=%ld d=%d: %d\n", c.K, c.N, c.d, r);
      return 1;
    }
  std::printf("clean\n");
  return 0;
}
#endif
