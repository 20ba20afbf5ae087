// TEST INFRASTRUCTURE: host build of the lane function of the data log-likelihood at arbitrary times
// (csrc/datalik_times_kernels.h, the text the GPU runs), so that its walk over ragged grids, its nodes, its skipping rules and its
// arithmetic can be checked against tests/_datalik_times_reference.py without a GPU.  A lane reads no other lane's memory, so the
// lanes run one after the other; the lane-private LDS column is a plain array.  `wave` > 1 walks the lanes in wavefronts of that
// many: the wave-uniform save index then starts at the largest record count of the lane's wavefront, so that a lane joins later,
// as on the device (wave <= 1: at the lane's own last record).  Buffers have their exact size, so that a sanitiser build sees any access past the
// records, the observations or the outputs.  Not part of the product.
#define ODEF_HOST_EMUL 1
#include "../../odefilters.jl_amd/csrc/datalik_times_kernels.h"
#include "../../odefilters.jl_amd/csrc/dispatch_dq.h"

#include <cstring>
#include <vector>

using namespace odef;

namespace {

template <int d, int q>
void run_lanes(DataLikTimesArgs a, int wave) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  std::vector<double> x(TRI);
  for (long i = 0; i < a.N; ++i) {
    a.host_n_hi = 0;
    if (wave > 1 && a.adaptive)
      for (long l = i / wave * wave; l < a.N && l < (i / wave + 1) * wave; ++l)
        if (a.nsaved[l] > a.host_n_hi) a.host_n_hi = a.nsaved[l];
    data_loglik_times_lane<d, q>(a, i, 0, true, LaneMem{x.data(), 1});
  }
}

}  // namespace

// records mean [n_save][D][N], cov [n_save][TRI][N], diff [n_save][N]; adaptive: tsave [n_save][N] and nsaved [N], else tgrid
// [n_save]; prior tables At, Qt, QLt [MAXNB][MAXNB]; observations times [M], comps [o], val [M][o] or [M][o][N], noise [o]
// -> loglik, maha [N].  Returns 0, or -1 for a (d, q) without an instance.
extern "C" int emul_datalik_times(int d, int q, const double* At, const double* Qt, const double* QLt, const double* mean,
                                  const double* cov, const double* diff, int adaptive, const double* tgrid, const double* tsave,
                                  const int* nsaved, long N, long n_save, const double* times, int M, const long long* comps, int o,
                                  const double* val, int per_traj, const double* noise, int wave, double* loglik, double* maha) {
  DataLikTimesArgs a;
  std::memset(&a, 0, sizeof a);
  std::memcpy(a.pc.At, At, sizeof a.pc.At);
  std::memcpy(a.pc.Qt, Qt, sizeof a.pc.Qt);
  std::memcpy(a.pc.QLt, QLt, sizeof a.pc.QLt);
  a.N = N;
  a.n_save = n_save;
  a.adaptive = adaptive;
  a.tgrid = tgrid;
  a.tsave = tsave;
  a.nsaved = nsaved;
  a.mean = mean;
  a.cov = cov;
  a.diff = diff;
  a.obs_time = times;
  a.obs_comp = comps;
  a.obs_val = val;
  a.obs_noise = noise;
  a.M = M;
  a.o = o;
  a.per_traj = per_traj;
  a.loglik = loglik;
  a.maha = maha;
  const bool ok = dispatch_dq<kDataLikMaxD, kDataLikTimesMaxState>(d, q, [&]<int dd, int qq>() { run_lanes<dd, qq>(a, wave); });
  return ok ? 0 : -1;
}
