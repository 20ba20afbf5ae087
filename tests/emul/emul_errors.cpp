// TEST INFRASTRUCTURE: host build of the solution-error kernels (csrc/errors_kernels.h, the text the GPU runs), so that their
// indexing, their skipping rules and their arithmetic can be checked against tests/_errors_reference.py without a GPU.  The
// kernels have no barrier, no shuffle and no lane reads another lane's LDS column, so the lanes of a grid run one after the other.
// The set-up (lanes per workgroup, chunks of the time axis, grid, tile size) repeats errors_run of csrc/errors.hip; buffers have
// their exact size, so that the sanitiser build sees any access past the tile, the partials or the records.  Not part of the product.
#define ODEF_HOST_EMUL 1
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__

namespace {
struct Idx { unsigned x; };
Idx threadIdx, blockIdx, blockDim;
double* g_lds;
}  // namespace

#define ODEF_ERRORS_TILE double* err_tile = g_lds
#include "../../odefilters.jl_amd/csrc/rhs.h"
#include "../../odefilters.jl_amd/csrc/errors_kernels.h"

using namespace odef;

namespace {
template <class F>
void run_grid(unsigned n_blocks, unsigned block, F f) {
  for (unsigned b = 0; b < n_blocks; ++b)
    for (unsigned t = 0; t < block; ++t) {
      threadIdx.x = t;
      blockIdx.x = b;
      blockDim.x = block;
      f();
    }
}

// FixedD > 0: the truth has a dimension of its own (a vector field's analytic), only that instantiation exists
template <class Truth, int FixedD = 0>
int run(int n_split, ErrArgs a, const typename Truth::Args& ta, double* fin, double* l2, double* linf, double* chi2, long long* nused) {
  const int d = a.d, tri = d * (d + 1) / 2;
  a.lanes = errors_lanes(d);
  a.n_split = n_split > 0 ? n_split : errors_split(a.N, a.n_save, a.lanes);
  a.chunk = (a.n_save + a.n_split - 1) / a.n_split;
  const long n_block = (a.N + a.lanes - 1) / a.lanes;
  const bool regs = d <= kErrRegD;
  const unsigned grid = (unsigned)(n_block * a.n_split), block = regs ? kErrBlock : 64;
  std::vector<double> part((size_t)a.n_split * kErrPartRows * a.N), lds(regs ? 0 : (size_t)(tri + d) * a.lanes);
  std::vector<int> cnt((size_t)a.n_split * 2 * a.N);
  a.part = part.data();
  a.part_cnt = cnt.data();
  g_lds = lds.data();
  if constexpr (FixedD > 0) {
    run_grid(grid, block, [&] { errors_partial_kernel<(FixedD <= kErrRegD ? FixedD : 0), Truth>(a, ta); });
  } else
  switch (regs ? d : 0) {
    case 1: run_grid(grid, block, [&] { errors_partial_kernel<1, Truth>(a, ta); }); break;
    case 2: run_grid(grid, block, [&] { errors_partial_kernel<2, Truth>(a, ta); }); break;
    case 3: run_grid(grid, block, [&] { errors_partial_kernel<3, Truth>(a, ta); }); break;
    case 4: run_grid(grid, block, [&] { errors_partial_kernel<4, Truth>(a, ta); }); break;
    case 5: run_grid(grid, block, [&] { errors_partial_kernel<5, Truth>(a, ta); }); break;
    case 6: run_grid(grid, block, [&] { errors_partial_kernel<6, Truth>(a, ta); }); break;
    case 7: run_grid(grid, block, [&] { errors_partial_kernel<7, Truth>(a, ta); }); break;
    case 8: run_grid(grid, block, [&] { errors_partial_kernel<8, Truth>(a, ta); }); break;
    default: run_grid(grid, block, [&] { errors_partial_kernel<0, Truth>(a, ta); }); break;
  }
  run_grid((unsigned)((a.N + 255) / 256), 256,
           [&] { errors_fold_kernel<>(part.data(), cnt.data(), a.n_split, a.N, d, fin, l2, linf, chi2, nused); });
  return a.n_split;
}

ErrArgs args(const double* mean, const double* cov, const double* tsave, const int* nsaved, long N, long n_save, int d, int D, int TRI) {
  ErrArgs a;
  std::memset(&a, 0, sizeof a);
  a.mean = mean;
  a.cov = cov;
  a.tsave = tsave;
  a.nsaved = nsaved;
  a.N = N;
  a.n_save = n_save;
  a.d = d;
  a.D = D;
  a.TRI = TRI;
  return a;
}
}  // namespace

extern "C" int emul_errors_lanes(int d) { return errors_lanes(d); }
extern "C" int emul_errors_split(long N, long n_save, int d) { return errors_split(N, n_save, errors_lanes(d)); }

// records mean [n_save][D][N], cov [n_save][TRI][N]; adaptive: tsave [n_save][N] and nsaved [N], else null; truth ref [n_save][d][N]
// -> fin, l2, linf, chi2 [N], nused [N].  n_split = 0: the launcher's choice.  Returns the number of chunks used.
extern "C" int emul_errors(int n_split, const double* mean, const double* cov, const double* tsave, const int* nsaved, const double* ref,
                           long N, long n_save, int d, int D, int TRI, double* fin, double* l2, double* linf, double* chi2,
                           long long* nused) {
  const TruthBuffer::Args t{ref, N, d};
  return run<TruthBuffer>(n_split, args(mean, cov, tsave, nsaved, N, n_save, d, D, TRI), t, fin, l2, linf, chi2, nused);
}

// the same with the truth from RhsLinear::analytic (d = 2): u0 [2][N], p [2] (shared) or [2][N], time of save k of trajectory i at
// t[k t_sk + i t_si]
extern "C" int emul_errors_linear(int n_split, const double* mean, const double* cov, const double* tsave, const int* nsaved,
                                  const double* u0, const double* p, int p_shared, const double* t, long t_sk, long t_si, long N,
                                  long n_save, int D, int TRI, double* fin, double* l2, double* linf, double* chi2, long long* nused) {
  const AnalyticArgs ta{u0, p, t, N, t_sk, t_si, p_shared};
  return run<TruthAnalytic<RhsLinear>, 2>(n_split, args(mean, cov, tsave, nsaved, N, n_save, 2, D, TRI), ta, fin, l2, linf, chi2, nused);
}

// u* of every save slot from RhsLinear::analytic, [n_save][2][N]
extern "C" void emul_truth_linear(const int* nsaved, const double* u0, const double* p, int p_shared, const double* t, long t_sk, long t_si,
                                  long N, long n_save, double* out) {
  const AnalyticArgs ta{u0, p, t, N, t_sk, t_si, p_shared};
  const long n_block = (N + kErrBlock - 1) / kErrBlock;
  run_grid((unsigned)(n_block * n_save), kErrBlock, [&] { errors_truth_kernel<TruthAnalytic<RhsLinear>>(ta, nsaved, N, n_save, 2, out); });
}
