// TEST INFRASTRUCTURE: host build of the data log-likelihood kernel's lane function (csrc/datalik_kernels.h, the text the GPU runs),
// so that its indexing, its skipping rules and its arithmetic can be checked against tests/_datalik_reference.py without a GPU.  A
// lane reads no other lane's memory, so the lanes run one after the other; the lane-private LDS column is a plain array.  The grid's
// step sizes and preconditioner tables are built as odef_solve_fixed builds them (csrc/api.hip).  Buffers have their exact size, so
// that a sanitiser build sees any access past the records, the observations or the outputs.  Not part of the product.
#define ODEF_HOST_EMUL 1
#include "../../odefilters.jl_amd/csrc/datalik_kernels.h"
#include "../../odefilters.jl_amd/csrc/dispatch_dq.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace odef;

namespace {

template <int d, int q>
void run_lanes(const DataLikArgs& a) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  std::vector<double> x(TRI);
  for (long i = 0; i < a.N; ++i) data_loglik_lane<d, q>(a, i, 0, LaneMem{x.data(), 1});
}

}  // namespace

// records mean [n_save][D][N], cov [n_save][TRI][N], diff [n_save][N], grid t [n_save] (a repeated time gives h = 0); prior tables
// At, Qt, QLt [MAXNB][MAXNB]; observations saves [M], comps [o], val [M][o] or [M][o][N], noise [o] -> loglik, maha [N].
// Returns 0, or -1 for a (d, q) without an instance.
extern "C" int emul_datalik(int d, int q, const double* At, const double* Qt, const double* QLt, const double* mean, const double* cov,
                            const double* diff, const double* t, long N, long n_save, const long long* saves, int M,
                            const long long* comps, int o, const double* val, int per_traj, const double* noise, double* loglik,
                            double* maha) {
  DataLikArgs a;
  std::memset(&a, 0, sizeof a);
  std::memcpy(a.pc.At, At, sizeof a.pc.At);
  std::memcpy(a.pc.Qt, Qt, sizeof a.pc.Qt);
  std::memcpy(a.pc.QLt, QLt, sizeof a.pc.QLt);
  const long nsteps = n_save - 1;
  std::vector<double> hs(nsteps), tabs;
  std::vector<int> idx(nsteps);
  std::vector<double> distinct;
  for (long n = 0; n < nsteps; ++n) {
    hs[n] = t[n + 1] - t[n];
    int k = -1;
    for (size_t j = distinct.size(); j-- > 0;)
      if (distinct[j] == hs[n]) { k = (int)j; break; }
    if (k < 0) {
      k = (int)distinct.size();
      distinct.push_back(hs[n]);
      tabs.resize(distinct.size() * kTabStride, 0.0);
      double* tb = tabs.data() + (size_t)k * kTabStride;
      if (hs[n] != 0.0) {
        const double pval = std::pow(hs[n], -q - 0.5);
        switch (q) {
          case 1: precond_fill<2>(hs[n], pval, tb); break;
          case 2: precond_fill<3>(hs[n], pval, tb); break;
          case 3: precond_fill<4>(hs[n], pval, tb); break;
          case 4: precond_fill<5>(hs[n], pval, tb); break;
          default: precond_fill<6>(hs[n], pval, tb); break;
        }
      }
    }
    idx[n] = k;
  }
  a.N = N;
  a.n_save = n_save;
  a.ptab = tabs.data();
  a.tab_idx = idx.data();
  a.hs = hs.data();
  a.mean = mean;
  a.cov = cov;
  a.diff = diff;
  a.obs_save = saves;
  a.obs_comp = comps;
  a.obs_val = val;
  a.obs_noise = noise;
  a.M = M;
  a.o = o;
  a.per_traj = per_traj;
  a.loglik = loglik;
  a.maha = maha;
  const bool ok = dispatch_dq<kDataLikMaxD, kDataLikMaxState>(d, q, [&]<int dd, int qq>() { run_lanes<dd, qq>(a); });
  return ok ? 0 : -1;
}
