// Event location per trajectory (events.h).  Two launches: the scan of one row of the mean records for sign changes
// (not templated), and the refinement of the first K brackets by bracketed Newton on the dense posterior, one slot per blockIdx.y.
// The refinement depends on (d, q) only and is instantiated here once, for the compiled-in and the run-time compiled fields alike.
#include "events.h"

#include <cstdint>
#include <cstdio>

#include "dispatch_dq.h"
#include "events_kernels.h"

namespace odef {
namespace {

template <class T>
bool alloc(T*& p, size_t n) {
  if (hipMalloc((void**)&p, sizeof(T) * n) == hipSuccess) return true;
  (void)hipGetLastError();
  p = nullptr;
  return false;
}

void release(EventsCache& ec) {
  free_device(ec.count, ec.direction, ec.save, ec.neval);
  free_device(ec.time, ec.tvar, ec.u);
  ec = EventsCache{};
}

}  // namespace

bool events_has(int d, int q) { return has_dq<kEventMaxD, kEventMaxState>(d, q); }

int events_run(EventsState& st, EventsCache& ec, const EventsRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname,
               size_t kname_n, std::string& err) {
  ec.valid = false;
  if (!events_has(r.d, r.q)) return pass_fail(err, "event location: no kernel for (d, q) = (%d, %d)", r.d, r.q);
  if (r.spec_bytes != 24)
    return pass_fail(err, "event location: ODEF_EV_SPEC holds %zu bytes, it is [3] int64 {component, direction, K} = 24", r.spec_bytes);
  if (r.level_bytes != 8 && r.level_bytes != (size_t)r.N * 8)
    return pass_fail(err, "event location: ODEF_EV_LEVEL holds %zu bytes, it is one double (8) or one per trajectory (%zu)",
                     r.level_bytes, (size_t)r.N * 8);
  if (r.N < 1 || r.n_save < 2) return pass_fail(err, "event location: needs at least two saves");
  long long spec[3];
  hipError_t e = hipMemcpyAsync(spec, r.spec, sizeof spec, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return pass_fail(err, "event location: %s", hipGetErrorString(e));
  if (spec[0] < 0 || spec[0] >= r.d)
    return pass_fail(err, "event location: component %lld outside 0 .. d - 1 = %d", spec[0], r.d - 1);
  if (spec[1] < -1 || spec[1] > 1) return pass_fail(err, "event location: direction %lld outside {-1, 0, 1}", spec[1]);
  const size_t per_slot = (size_t)r.N * (size_t)(r.d > 1 ? r.d : 1) * 8;
  if (spec[2] < 1 || spec[2] >= (1ll << 31) || (unsigned long long)spec[2] * per_slot >= (1ull << 31))
    return pass_fail(err, "event location: K = %lld: need K >= 1 and K * N * max(d, 1) * 8 bytes below 2 GiB", spec[2]);
  const long K = (long)spec[2];
  if (K > 65535) return pass_fail(err, "event location: K = %ld exceeds the 65535 slots of one launch", K);
  const size_t slots = (size_t)K * (size_t)r.N;
  if (ec.slots < slots || !ec.count) {
    release(ec);
    if (!alloc(ec.count, (size_t)r.N) || !alloc(ec.time, slots) || !alloc(ec.tvar, slots) || !alloc(ec.u, slots * r.d) ||
        !alloc(ec.direction, slots) || !alloc(ec.save, slots) || !alloc(ec.neval, slots)) {
      release(ec);
      return pass_fail(err, "event location: out of device memory");
    }
    ec.slots = slots;
  }
  EventArgs a;
  a.pc = *r.pc;
  a.N = r.N;
  a.n_save = r.n_save;
  a.adaptive = r.adaptive;
  a.source = r.source;
  a.comp = (int)spec[0];
  a.dir = (int)spec[1];
  a.K = (int)K;
  a.D = r.d * (r.q + 1);
  a.level_per_traj = r.level_bytes != 8;
  a.tgrid = r.tgrid;
  a.tsave = r.tsave;
  a.nsaved = r.nsaved;
  a.mean = r.mean;
  a.cov = r.cov;
  a.diff = r.diff;
  a.smean = r.smean;
  a.scov = r.scov;
  a.level = r.level;
  a.count = ec.count;
  a.time = ec.time;
  a.tvar = ec.tvar;
  a.u = ec.u;
  a.direction = ec.direction;
  a.save = ec.save;
  a.neval = ec.neval;
  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "event location: hipEventCreate failed");
  hipLaunchKernelGGL(event_scan_kernel, dim3((unsigned)((a.N + kEventWave - 1) / kEventWave)), dim3(kEventWave), 0, stream, a);
  auto refine = [&]<int d, int q>() {
    hipLaunchKernelGGL((event_refine_kernel<d, q>), dim3((unsigned)((a.N + kEventWave - 1) / kEventWave), (unsigned)a.K), dim3(kEventWave),
                       0, stream, a);
  };
  if (!dispatch_dq<kEventMaxD, kEventMaxState>(r.d, r.q, refine)) return pass_fail(err, "event location: no kernel");
  if (kname) std::snprintf(kname, kname_n, "odef::event_refine_kernel<%d, %d>", r.d, r.q);
  if (e = st.timer.end(stream, ms); e != hipSuccess) return pass_fail(err, "event location: %s", hipGetErrorString(e));
  if (n_launches) *n_launches += 2;  // a running count: a request served from the cache leaves it unchanged
  ec.K = K;
  ec.valid = true;
  return 0;
}

void events_free(EventsState& st) {
  for (EventsCache& ec : st.src) release(ec);
  st.timer.destroy();
}

}  // namespace odef
