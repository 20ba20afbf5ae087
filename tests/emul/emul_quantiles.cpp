// TEST INFRASTRUCTURE: host build of the ensemble-quantile kernels (csrc/quantile_kernels.h, the text the GPU runs), so that the
// key transform, the inclusion rule, the digit passes and the tie rule can be checked against tests/_quantile_reference.py
// without a GPU.  One host thread per lane of a workgroup: __syncthreads is a std::barrier over the 256 lanes, __shfl_xor and
// __ballot exchange through a per-wavefront array between two per-wavefront barriers, LDS is a static array, LDS and global
// atomics are __atomic builtins.  Workgroups run one after the other and launches run in order, in the sequence of
// quantiles.hip.  Every buffer has its exact size, so a sanitiser build sees any access past one.  With -DODEF_EMUL_MAIN the
// file is a stand-alone program that runs a fixed set of cases on generated data and prints "clean".  Not part of the product.
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static

namespace {
struct Idx { unsigned x; };
thread_local Idx threadIdx, blockIdx, blockDim;
std::barrier<>* g_block_bar;
std::barrier<>* g_wave_bar[4];
unsigned long long g_xq[4][64];
int g_xi[4][64];

void __syncthreads() { g_block_bar->arrive_and_wait(); }
unsigned long long __shfl_xor(unsigned long long v, int m, int) {
  const int w = threadIdx.x / 64, l = threadIdx.x % 64;
  g_xq[w][l] = v;
  g_wave_bar[w]->arrive_and_wait();
  const unsigned long long r = g_xq[w][l ^ m];
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
int __shfl_xor(int v, int m, int) {
  const int w = threadIdx.x / 64, l = threadIdx.x % 64;
  g_xi[w][l] = v;
  g_wave_bar[w]->arrive_and_wait();
  const int r = g_xi[w][l ^ m];
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
unsigned long long __ballot(bool pred) {
  const int w = threadIdx.x / 64, l = threadIdx.x % 64;
  g_xi[w][l] = pred ? 1 : 0;
  g_wave_bar[w]->arrive_and_wait();
  unsigned long long r = 0;
  for (int k = 0; k < 64; ++k) r |= (unsigned long long)(g_xi[w][k] & 1) << k;
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
int __popc(unsigned x) { return __builtin_popcount(x); }
int __clzll(long long x) { return __builtin_clzll((unsigned long long)x); }
unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
}
unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
  unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
}
int atomicMax(int* p, int v) {
  int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
}
}  // namespace

#include "../../odefilters.jl_amd/csrc/quantile_kernels.h"

using namespace odef;

namespace {
// The 256 lane threads of the emulated device, kept for all launches of one run.  One launch: the lanes walk the workgroups in
// order, a barrier between two workgroups; the launching thread waits for the last one.
struct Lanes {
  std::barrier<> block_bar{kQBlock}, w0{64}, w1{64}, w2{64}, w3{64}, go{kQBlock + 1}, done{kQBlock + 1};
  std::function<void()> job;
  long n_blocks = 0;
  bool quit = false;
  std::vector<std::thread> lanes;

  Lanes() {
    g_block_bar = &block_bar;
    g_wave_bar[0] = &w0, g_wave_bar[1] = &w1, g_wave_bar[2] = &w2, g_wave_bar[3] = &w3;
    for (unsigned t = 0; t < (unsigned)kQBlock; ++t)
      lanes.emplace_back([this, t] {
        threadIdx.x = t;
        blockDim.x = kQBlock;
        for (;;) {
          go.arrive_and_wait();
          if (quit) return;
          for (long b = 0; b < n_blocks; ++b) {
            blockIdx.x = (unsigned)b;
            job();
            block_bar.arrive_and_wait();
          }
          done.arrive_and_wait();
        }
      });
  }
  ~Lanes() {
    quit = true;
    go.arrive_and_wait();
    for (auto& t : lanes) t.join();
  }
  template <class F>
  void launch(long blocks, F f) {
    job = f;
    n_blocks = blocks;
    go.arrive_and_wait();
    done.arrive_and_wait();
  }
};

int run(const double* mean_all, const int* rc, long N, long n_t, int d, int D, int P, const double* pr, int iters, long T,
        long long* count_all, double* q_all, int* passes_out) {
  if (d < 1 || d > kQMaxDim || P < 1 || P > kQMaxProbs || iters < 1 || iters > kQMaxIters || T < 1 || N < 1 || n_t < 1) return -1;
  const int R = 2 * P, W = (int)((N + kQWave - 1) / kQWave);
  const long n_chunk = (N + (long)kQBlock * iters - 1) / ((long)kQBlock * iters);
  QuantileProbs probs{};
  for (int p = 0; p < P; ++p) probs.p[p] = pr[p];
  int passes_total = 0;
  Lanes dev;
  for (long s0 = 0; s0 < n_t; s0 += T) {
    const long Ts = n_t - s0 < T ? n_t - s0 : T, rows = Ts * d;
    std::vector<qkey_t> mask((size_t)Ts * W), kmin(rows), kmax(rows), prefix((size_t)rows * R);
    std::vector<int> low(rows), owner((size_t)rows * R), max_low(1);
    std::vector<unsigned> rem((size_t)rows * R), hist((size_t)rows * R * kQBins, 0xDEADu);
    const double* mean = mean_all + (size_t)s0 * D * N;
    long long* count = count_all + s0;
    dev.launch(rows, [&] { quantile_init_kernel(d, R, count, kmin.data(), kmax.data(), hist.data(), max_low.data()); });
    dev.launch(Ts * n_chunk, [&] {
      quantile_mask_kernel(mean, rc, N, d, D, W, (int)n_chunk, iters, mask.data(), count, kmin.data(), kmax.data());
    });
    dev.launch((rows + kQBlock - 1) / kQBlock, [&] {
      quantile_start_kernel(rows, d, P, probs, count, kmin.data(), kmax.data(), low.data(), prefix.data(), rem.data(), owner.data(),
                            max_low.data());
    });
    const int passes = (max_low[0] + 7) / 8;
    for (int k = 0; k < passes; ++k) {
      dev.launch(rows * n_chunk, [&] {
        quantile_hist_kernel(mean, mask.data(), N, d, D, W, (int)n_chunk, iters, R, kmin.data(), low.data(), prefix.data(), owner.data(),
                             hist.data());
      });
      dev.launch(rows, [&] { quantile_select_kernel(R, low.data(), prefix.data(), rem.data(), owner.data(), hist.data()); });
    }
    dev.launch((rows * P + kQBlock - 1) / kQBlock,
             [&] { quantile_finish_kernel(rows, d, P, probs, count, kmin.data(), prefix.data(), q_all + (size_t)s0 * P * d); });
    passes_total += passes;
  }
  if (passes_out) *passes_out = passes_total;
  return 0;
}
}  // namespace

// records mean [n_t][D][N], retcode [N], probabilities [P] -> count [n_t], q [n_t][P][d]; iters: 256-trajectory steps of a
// lane per chunk, slab: times per slab; passes: digit passes run, summed over the slabs
extern "C" int emul_quantiles(const double* mean, const int* rc, long N, long n_t, int d, int D, int P, const double* probs,
                              int iters, long slab, long long* count, double* q, int* passes) {
  return run(mean, rc, N, n_t, d, D, P, probs, iters, slab, count, q, passes);
}

#ifdef ODEF_EMUL_MAIN
namespace {
unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
double uniform() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_rng >> 11) * 0x1.0p-53;
}

// the definition with std::sort, for the program's own check
bool check(long N, long n_t, int d, int D, int P, const double* probs, int iters, long slab, int kind) {
  std::vector<double> mean((size_t)n_t * D * N);
  std::vector<int> rc(N, 0);
  for (size_t k = 0; k < mean.size(); ++k) {
    const double u = uniform();
    mean[k] = kind == 0   ? 27.0 + 1e-6 * u
              : kind == 1 ? (u < 0.5 ? -1.0 : 1.0) * std::pow(10.0, 600.0 * uniform() - 300.0)
              : kind == 2 ? (u < 0.9 ? 1.5 : u)
                          : (u < 0.3 ? -0.0 : u < 0.6 ? 0.0 : 4.9e-324 * (double)(k % 7));
  }
  if (N > 2) rc[1] = 3;
  if (N > 3) mean[((size_t)0 * D + (d - 1)) * N + 2] = INFINITY;
  if (N > 4 && n_t > 1) mean[((size_t)1 * D + 0) * N + 4] = NAN;
  std::vector<long long> count(n_t);
  std::vector<double> q((size_t)n_t * P * d);
  if (run(mean.data(), rc.data(), N, n_t, d, D, P, probs, iters, slab, count.data(), q.data(), nullptr)) return false;
  for (long s = 0; s < n_t; ++s) {
    std::vector<long> in;
    for (long i = 0; i < N; ++i) {
      bool ok = rc[i] == 0;
      for (int a = 0; a < d; ++a) ok = ok && std::isfinite(mean[((size_t)s * D + a) * N + i]);
      if (ok) in.push_back(i);
    }
    const long long n = (long long)in.size();
    if (count[s] != n) return false;
    for (int a = 0; a < d; ++a) {
      std::vector<double> x;
      for (long i : in) x.push_back(mean[((size_t)s * D + a) * N + i]);
      std::sort(x.begin(), x.end());
      for (int p = 0; p < P; ++p) {
        const double got = q[((size_t)s * P + p) * d + a];
        if (n == 0) {
          if (!std::isnan(got)) return false;
          continue;
        }
        const double h = (double)(n - 1) * probs[p];
        long long lo = (long long)std::floor(h);
        if (lo > n - 1) lo = n - 1;
        const long long hi = lo + 1 < n ? lo + 1 : n - 1;
        const double g = h - (double)lo, diff = x[hi] - x[lo], prod = g * diff;
        const double want = g == 0.0 ? x[lo] : x[lo] + prod;
        if (!(got == want) && !(std::isnan(got) && std::isnan(want))) return false;
      }
    }
  }
  return true;
}
}  // namespace

int main() {
  const double probs[8] = {0.95, 0.0, 0.5, 1.0 / 3.0, 0.05, 1.0, 0.25, 0.5};
  struct Case { long N, n_t; int d, D, P, iters; long slab; int kind; };
  const Case cases[] = {
      {1, 2, 2, 4, 1, 1, 1, 0},    {2, 2, 3, 6, 3, 1, 2, 1},    {63, 2, 2, 4, 8, 1, 2, 2},  {64, 2, 3, 3, 3, 2, 1, 3},
      {65, 1, 16, 32, 3, 1, 1, 1}, {257, 1, 28, 28, 1, 1, 1, 0}, {1001, 2, 3, 12, 8, 2, 1, 1}, {700, 3, 2, 4, 3, 1, 2, 2},
  };
  for (const Case& c : cases)
    if (!check(c.N, c.n_t, c.d, c.D, c.P, probs, c.iters, c.slab, c.kind)) {
      std::printf("mismatch at N=%ld d=%d P=%d kind=%d\n", c.N, c.d, c.P, c.kind);
      return 1;
    }
  std::printf("clean\n");
  return 0;
}
#endif
