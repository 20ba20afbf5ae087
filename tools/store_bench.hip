// Microbenchmark: what HBM write rate does the filter kernel's store shape reach on its own?
// `waves` wavefronts, each storing field rows of 512 B (8 B/lane) or 1 KiB (16 B/lane) per step into a
// [nsteps][rows][N] array -- no arithmetic.  Variants: nontemporal stores, more waves per SIMD.
// `store_bench stream [rounds]`: the address stream of the headline filter kernel itself (k_stream below) under the two
// wave -> trajectory maps of csrc/wave_map.h, timed alternately.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "wave_map.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

template <int W, int NT>
__global__ __launch_bounds__(64) void k_store(double* out, long N, int rows, int nsteps, int split) {
  // `split` blocks share one 64-trajectory column group, each writing rows/split of the rows
  const long grp = blockIdx.x / split, part = blockIdx.x % split;
  const long i0 = grp * 64;
  const unsigned lane = threadIdx.x;
  double v = (double)lane;
  const int r0 = (int)part * (rows / split), r1 = r0 + rows / split;
  for (int n = 0; n < nsteps; ++n) {
    double* base = out + ((size_t)n * rows * N + (size_t)r0 * N + i0 * W);
    for (int k = r0; k < r1; k += W) {
      if (W == 1) { if (NT) __builtin_nontemporal_store(v, base + lane); else base[lane] = v; }
      else {
        typedef double d2 __attribute__((ext_vector_type(2)));
        d2 t = {v, v + 1.0};
        if (NT) __builtin_nontemporal_store(t, (d2*)base + lane); else ((d2*)base)[lane] = t;
      }
      base += N * W;
    }
    v += 1.0;
  }
}

// Blocked layout [nsteps][N/64][rows][64]: the record of one wavefront (rows x 512 B) is one contiguous block.
template <int NT>
__global__ __launch_bounds__(64) void k_store_blocked(double* out, long N, int rows, int nsteps) {
  const long grp = blockIdx.x, G = N / 64;
  const unsigned lane = threadIdx.x;
  double v = (double)lane;
  for (int n = 0; n < nsteps; ++n) {
    double* base = out + (((size_t)n * G + grp) * rows) * 64;
    for (int k = 0; k < rows; ++k) {
      if (NT) __builtin_nontemporal_store(v, base + lane); else base[lane] = v;
      base += 64;
    }
    v += 1.0;
  }
}
template <int NT>
float run_blocked(double* d, long N, int rows, int nsteps) {
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  float best = 1e9;
  for (int rep = 0; rep < 4; ++rep) {
    CK(hipEventRecord(a));
    hipLaunchKernelGGL((k_store_blocked<NT>), dim3(N / 64), dim3(64), 0, 0, d, N, rows, nsteps);
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b)); if (ms < best) best = ms;
  }
  return best;
}

template <int W, int NT>
float run(double* d, long N, int rows, int nsteps, int split) {
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  float best = 1e9;
  for (int rep = 0; rep < 4; ++rep) {
    CK(hipEventRecord(a));
    hipLaunchKernelGGL((k_store<W, NT>), dim3(N / 64 * split), dim3(64), 0, 0, d, N, rows, nsteps, split);
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b)); if (ms < best) best = ms;
  }
  return best;
}

// The record stream of ek_filter_fixed_kernel<RhsLorenz63, 3, true, true> at 65 536 trajectories: one single-wave workgroup per
// 64 trajectories; per step 12 mean rows, 78 covariance rows and 1 diffusion row of 8 B/lane, non-temporal buffer stores with
// the row offset in an SGPR (RowStore, csrc/ek_lane.h), rows N * 8 bytes apart, into record-sized arrays [n_rec][rows][N].
// A chain of FPS dependent FP64 FMAs in front of every store paces the stream like the step's arithmetic does (91 x 20 = 1 820
// against the step's 1 831 FP64 instructions), so that the records do not leave as one burst.  `mode`: wave_map.h.
struct RowPut {
  __amdgpu_buffer_rsrc_t rs;
  unsigned voff, soff, step;
  __device__ RowPut(double* base, size_t N, size_t rows, unsigned lane)
      : rs(__builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)(rows * N * sizeof(double)), 0x00020000)),
        voff(lane * 8u), soff(0u), step((unsigned)(N * sizeof(double))) {}
  __device__ void put(double v) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rs, voff, soff, 2 /* nt */);
    soff += step;
    asm volatile("" : "+s"(soff));
  }
};
template <int FPS>
__global__ __launch_bounds__(64) void k_stream(double* mean, double* cov, double* diff, long N, long n_rec, int mode, double a, double b) {
  constexpr int D = 12, TRI = 78;
  const long i0 = odef::wave_first_trajectory(blockIdx.x, gridDim.x, mode);
  const unsigned lane = threadIdx.x;
  if (i0 + lane >= N) return;
  double v = (double)lane;
  const size_t Nn = (size_t)N;
  for (long n = 0; n < n_rec; ++n) {
    RowPut sm(mean + ((size_t)n * D * Nn + i0), Nn, D, lane), sc(cov + ((size_t)n * TRI * Nn + i0), Nn, TRI, lane),
        sd(diff + ((size_t)n * Nn + i0), Nn, 1, lane);
#pragma unroll
    for (int k = 0; k < D + TRI + 1; ++k) {
#pragma unroll
      for (int j = 0; j < FPS; ++j) v = __builtin_fma(v, a, b);
      if (k < D) sm.put(v);
      else if (k < D + TRI) sc.put(v);
      else sd.put(v);
    }
  }
}
static int stream_main(int rounds) {
  const long N = 65536, n_rec = 1025;
  const size_t per_rec = (size_t)N * 8, bm = n_rec * 12 * per_rec, bc = n_rec * 78 * per_rec, bd = n_rec * per_rec;
  double *mean, *cov, *diff;
  CK(hipMalloc((void**)&mean, bm)); CK(hipMalloc((void**)&cov, bc)); CK(hipMalloc((void**)&diff, bd));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  auto once = [&](int mode) {
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_stream<20>), dim3((unsigned)(N / 64)), dim3(64), 0, 0, mean, cov, diff, N, n_rec, mode, 1.0, 0.0);
    CK(hipGetLastError());
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  };
  const double gb = (double)(bm + bc + bd) / 1e9;
  printf("# record stream of the headline filter kernel: %ld waves, %ld records of 12 + 78 + 1 rows, %.2f GB per launch\n", N / 64, n_rec, gb);
  printf("# warm-up (first touch): map 0 %.3f ms, map 1 %.3f ms\n", once(0), once(1));
  // per round: identity, XCD-contiguous, identity again (the pair of identity runs is the noise floor)
  std::vector<float> t[3];
  const int modes[3] = {0, 1, 0};
  for (int r = 0; r < rounds; ++r) {
    float ms[3];
    for (int k = 0; k < 3; ++k) { ms[k] = once(modes[k]); t[k].push_back(ms[k]); }
    printf("round %2d  map0 %.3f ms  map1 %.3f ms  map0 again %.3f ms\n", r, ms[0], ms[1], ms[2]);
  }
  const char* names[3] = {"(A) identity          ", "(B) XCD-contiguous    ", "(A') identity, repeat "};
  for (int k = 0; k < 3; ++k) {
    std::sort(t[k].begin(), t[k].end());
    const float med = 0.5f * (t[k][(rounds - 1) / 2] + t[k][rounds / 2]), mn = t[k][0];
    printf("%s median %.3f ms %.2f TB/s   min %.3f ms %.2f TB/s\n", names[k], med, gb / med, mn, gb / mn);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "stream")) return stream_main(argc > 2 ? std::max(1, atoi(argv[2])) : 12);
  const long N = 65536; const int rows = 96, nsteps = argc > 1 ? atoi(argv[1]) : 512;
  double* d; size_t bytes = (size_t)nsteps * rows * N * 8;
  CK(hipMalloc((void**)&d, bytes));
  {
    float t;
    t = run_blocked<0>(d, N, rows, nsteps); printf("blocked layout, 1 wave/SIMD, 8 B/lane plain  %.3f ms %.2f TB/s\n", t, bytes / (t * 1e-3) / 1e12);
    t = run_blocked<1>(d, N, rows, nsteps); printf("blocked layout, 1 wave/SIMD, 8 B/lane nt     %.3f ms %.2f TB/s\n", t, bytes / (t * 1e-3) / 1e12);
  }
  for (int split : {1, 2, 4, 8}) {
    float t;
    t = run<1, 0>(d, N, rows, nsteps, split); printf("waves/SIMD=%d  8 B/lane plain  %.3f ms %.2f TB/s\n", split, t, bytes / (t * 1e-3) / 1e12);
    t = run<1, 1>(d, N, rows, nsteps, split); printf("waves/SIMD=%d  8 B/lane nt     %.3f ms %.2f TB/s\n", split, t, bytes / (t * 1e-3) / 1e12);
    t = run<2, 0>(d, N, rows, nsteps, split); printf("waves/SIMD=%d 16 B/lane plain  %.3f ms %.2f TB/s\n", split, t, bytes / (t * 1e-3) / 1e12);
    t = run<2, 1>(d, N, rows, nsteps, split); printf("waves/SIMD=%d 16 B/lane nt     %.3f ms %.2f TB/s\n", split, t, bytes / (t * 1e-3) / 1e12);
  }
  return 0;
}
