// TEST INFRASTRUCTURE: host build of the ensemble-summary reduction (csrc/summary_kernels.h, the text the GPU runs), so that
// its indexing, its inclusion rule and its arithmetic can be checked against tests/_summary_reference.py without a GPU.  One
// host thread per lane of a wavefront; __shfl_xor is an exchange through a 64-slot array between two barriers, so the butterfly
// adds in the order of the device.  Wavefronts run one after the other (the kernels have no workgroup barrier and no lane reads
// another lane's LDS column).  Not part of the product.
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__

namespace {
struct Idx { unsigned x; };
thread_local Idx threadIdx, blockIdx, blockDim;
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
}  // namespace

#define ODEF_SUMMARY_TILE double* tile = g_lds
#include "../../odefilters.jl_amd/csrc/summary_kernels.h"

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
          f();
        });
      for (auto& t : lanes) t.join();
    }
}

template <class F>
void run_fold(long n_t, F f) {
  for (long s = 0; s < n_t; ++s)
    for (unsigned t = 0; t < 64; ++t) {  // (the fold's lanes are independent)
      threadIdx.x = t;
      blockIdx.x = (unsigned)s;
      blockDim.x = 64;
      f();
    }
}

template <int K>
void run(const double* mean, const double* cov, const int* rc, long N, long n_t, int d, int D, int TRI, long long* count, double* m,
         double* within, double* between) {
  const int tri = d * (d + 1) / 2, R = d + tri;
  const int n_block = (int)((N + 256L * K - 1) / (256L * K)), n_wave = n_block * 4;
  // exact-size buffers: the sanitiser build sees any access past the tile, the partials or the records
  std::vector<double> part((size_t)n_t * n_wave * R), lds((size_t)d * K * 256);
  std::vector<int> part_cnt((size_t)n_t * n_wave);
  g_lds = lds.data();
  run_grid(n_block * n_t, [&] { summary_sums_kernel<K>(mean, cov, rc, N, d, D, TRI, n_wave, part.data(), part_cnt.data()); });
  run_fold(n_t, [&] { summary_fold_kernel(part.data(), part_cnt.data(), n_wave, R, d, count, m, within); });
  part.assign((size_t)n_t * n_wave * tri, 0.0);
  run_grid(n_block * n_t, [&] { summary_centred_kernel<K>(mean, rc, m, N, d, D, n_wave, part.data()); });
  run_fold(n_t, [&] { summary_fold_kernel(part.data(), nullptr, n_wave, tri, tri, count, between, nullptr); });
}
}  // namespace

// records mean [n_t][D][N], cov [n_t][TRI][N], retcode [N] -> count [n_t], m [n_t][d], within / between [n_t][tri(d)]
extern "C" int emul_summary(int K, const double* mean, const double* cov, const int* rc, long N, long n_t, int d, int D, int TRI,
                            long long* count, double* m, double* within, double* between) {
  switch (K) {
    case 8: run<8>(mean, cov, rc, N, n_t, d, D, TRI, count, m, within, between); return 0;
    case 4: run<4>(mean, cov, rc, N, n_t, d, D, TRI, count, m, within, between); return 0;
    case 2: run<2>(mean, cov, rc, N, n_t, d, D, TRI, count, m, within, between); return 0;
    case 1: run<1>(mean, cov, rc, N, n_t, d, D, TRI, count, m, within, between); return 0;
    default: return -1;
  }
}
