// Event location per trajectory on the device (include/odefilter.h, odef_event_field): the times at which one
// component of the posterior mean crosses a level, found on the records by a scan for sign changes and a bracketed Newton iteration
// on the dense posterior.  Host-side interface of events.hip; this header includes none of the step headers, so that no filter /
// smoother kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "pass_host.h"

namespace odef {

struct PriorConsts;  // ek_math.h

// the cached outputs of one source, device memory owned by the context
struct EventsCache {
  int* count = nullptr;      // [N]
  double* time = nullptr;    // [K][N]
  double* tvar = nullptr;    // [K][N]
  double* u = nullptr;       // [K][d][N]
  int* direction = nullptr;  // [K][N]
  int* save = nullptr;       // [K][N]
  int* neval = nullptr;      // [K][N]
  size_t slots = 0;          // K N the arrays were allocated for
  long K = 0;                // of the cached result
  bool valid = false;
};

struct EventsState {
  EventsCache src[2];  // filter / smoothed posterior
  PassTimer timer;
};

struct EventsRequest {
  const PriorConsts* pc;
  long N, n_save;
  int d, q, adaptive, source;
  const double* tgrid;   // fixed: [n_save] (device)
  const double* tsave;   // adaptive: [n_save][N]
  const int* nsaved;     // adaptive: [N]
  const double* mean;    // filter records, ABI layout
  const double* cov;
  const double* diff;
  const double* smean;   // smoothed records (source 1)
  const double* scov;
  const void* spec;      // ODEF_EV_SPEC: [3] int64 {component, direction, K} (device)
  const double* level;   // ODEF_EV_LEVEL: [1] or [N] (device)
  size_t spec_bytes, level_bytes;
};

// true when event_refine_kernel<d, q> is instantiated (d <= 4, q <= 5, d (q + 1) <= 12)
bool events_has(int d, int q);
// Copies the three spec words to the host and validates them, runs the pass on `stream` (two launches) into `ec` and waits.
// Returns 0, or -1 with `err` set.
int events_run(EventsState& st, EventsCache& ec, const EventsRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname,
               size_t kname_n, std::string& err);
void events_free(EventsState& st);

}  // namespace odef
