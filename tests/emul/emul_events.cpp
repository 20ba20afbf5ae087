// TEST INFRASTRUCTURE: host build of the event location kernels' lane functions (csrc/events_kernels.h, the text the GPU runs), so that
// their indexing, the bracket rule and the Newton iteration can be checked against tests/_events_reference.py without a GPU.  A lane
// reads no other lane's memory, so the lanes run one after the other; the lane-private LDS column is a plain array.  The scan gets
// the record count of its group of 64 lanes as the wave-uniform bound, as the kernel does.  Buffers have their exact size, so that a
// sanitiser build sees any access past the records, the inputs or the outputs.  Not part of the product.
#define ODEF_HOST_EMUL 1
#include "../../odefilters.jl_amd/csrc/dispatch_dq.h"
#include "../../odefilters.jl_amd/csrc/events_kernels.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace odef;

namespace {

template <int d, int q>
void refine_lanes(const EventArgs& a) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  std::vector<double> x(TRI);
  for (long s = 0; s < a.K; ++s)
    for (long i = 0; i < a.N; ++i) event_refine_lane<d, q>(a, i, s, LaneMem{x.data(), 1});
}

}  // namespace

// Records mean [n_save][D][N], cov [n_save][TRI][N], diff [n_save][N] and, for source 1, smean / scov; times t [n_save] (fixed grid) or
// [n_save][N] with nsaved [N] (adaptive); prior tables At, Qt, QLt [MAXNB][MAXNB]; level [1] or [N].  Outputs as the ABI lays them
// out: count [N], time / tvar [K][N], u [K][d][N], direction / save / neval [K][N].  Returns 0, or -1 for a (d, q) without an instance.
extern "C" int emul_events(int d, int q, const double* At, const double* Qt, const double* QLt, const double* mean, const double* cov,
                           const double* diff, const double* smean, const double* scov, const double* t, const int* nsaved, int adaptive,
                           long N, long n_save, int source, int comp, int dir, int K, const double* level, int level_per_traj, int* count,
                           double* time, double* tvar, double* u, int* direction, int* save, int* neval) {
  if (!has_dq<kEventMaxD, kEventMaxState>(d, q)) return -1;
  EventArgs a;
  std::memset(&a, 0, sizeof a);
  std::memcpy(a.pc.At, At, sizeof a.pc.At);
  std::memcpy(a.pc.Qt, Qt, sizeof a.pc.Qt);
  std::memcpy(a.pc.QLt, QLt, sizeof a.pc.QLt);
  a.N = N;
  a.n_save = n_save;
  a.adaptive = adaptive;
  a.source = source;
  a.comp = comp;
  a.dir = dir;
  a.K = K;
  a.D = d * (q + 1);
  a.level_per_traj = level_per_traj;
  a.tgrid = adaptive ? nullptr : t;
  a.tsave = adaptive ? t : nullptr;
  a.nsaved = nsaved;
  a.mean = mean;
  a.cov = cov;
  a.diff = diff;
  a.smean = smean;
  a.scov = scov;
  a.level = level;
  a.count = count;
  a.time = time;
  a.tvar = tvar;
  a.u = u;
  a.direction = direction;
  a.save = save;
  a.neval = neval;
  for (long i0 = 0; i0 < N; i0 += kEventWave) {
    const long i1 = std::min(N, i0 + kEventWave);
    long n_hi = n_save;
    if (adaptive) {
      n_hi = 0;
      for (long i = i0; i < i1; ++i) n_hi = std::max(n_hi, (long)nsaved[i]);
    }
    for (long i = i0; i < i1; ++i) event_scan_lane(a, i, n_hi);
  }
  const bool ok = dispatch_dq<kEventMaxD, kEventMaxState>(d, q, [&]<int dd, int qq>() { refine_lanes<dd, qq>(a); });
  return ok ? 0 : -1;
}
