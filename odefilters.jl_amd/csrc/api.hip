// C-ABI layer of libodefilter_hip.so (see include/odefilter.h for the contract and the
// reference interfaces each entry point replaces).  Owns device buffers, builds the prior
// tables (src/priors.jl:7-59) and the per-step preconditioner seeds
// (src/preconditioning.jl:9) on the host, launches the gfx950 kernels, times them with
// hipEvents on the launch stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "../../include/odefilter.h"
#include "jit.h"
#include "launch.h"
#include "summary.h"
#include "errors.h"
#include "datalik.h"
#include "events.h"
#include "quantiles.h"
#include "wsummary.h"

using namespace odef;

namespace {

thread_local std::string g_create_error;

struct Buf {
  void* ptr = nullptr;
  size_t bytes = 0;     // capacity
  size_t valid = 0;     // bytes holding results
  bool owned = false;
  bool bound = false;
};

struct RhsInfo { int d, np; };
const RhsInfo kRhs[] = {{2, 3}, {3, 3}, {2, 4}, {2, 1}, {2, 2}, {28, 0}, {16, 1}, {2, 3}};

// the passes a context times and names: `which` of odef_kernel_time_ms / odef_kernel_name
enum Pass { kPassFilter = 0, kPassSmooth = 1, kPassSummary = 2, kPassErrors = 3, kPassDataLik = 4, kPassEvents = 5, kPassQuantiles = 6, kPassWSummary = 7, kPassCount };

}  // namespace

struct odef_ctx {
  odef_config cfg{};
  int d = 0, q = 0, D = 0, TRI = 0, np = 0;
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  PriorConsts pc{};
  double* d_u0 = nullptr;
  double* d_p = nullptr;
  bool have_problem = false;
  double t0 = 0.0;
  // time grid of the last fixed solve
  std::vector<double> tgrid;
  double* d_hs = nullptr;
  double* d_tgrid = nullptr;
  bool grid_on_device = false;  // d_hs / d_ptab / d_tab_idx / d_tgrid hold the tables of `tgrid`
  double* d_tq = nullptr;
  size_t tq_cap = 0;
  long n_q = 0;
  long n_samples = 0;
  bool smoothed_done = false;
  double* d_ptab = nullptr;
  int* d_tab_idx = nullptr;
  size_t grid_cap = 0;
  long n_save = 0;
  bool adaptive = false;
  bool solved = false;
  const FieldLaunch* field = nullptr;  // launch functions of the vector field (compiled-in, or owned by the registry in jit.hip)
  double* d_ws = nullptr;   // per-trajectory workspace of the team kernels
  double* d_stage = nullptr;  // trajectory-major stage of the covariance records (D = 168 smoother, record_stage.h)
  long stage_filter_recs = 0; // > 0: the stage holds this many filter records (record r at r N ld); reset by records_changed
  size_t stage_cap = 0;     // doubles
  size_t ws_cap = 0;
  Buf f[ODEF_F_COUNT_];
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float ms[kPassCount] = {};
  int nl[kPassCount] = {};
  char kname[kPassCount][192] = {};  // kernel of the last pass of each kind (odef_kernel_name)
  SummaryState summary;  // cached ensemble summaries of the filter, smoothed and dense records (odef_summary_field)
  ErrorsState errors;    // cached solution errors of the filter and smoothed records (odef_errors_field)
  const double* err_ref = nullptr;  // ODEF_E_REFERENCE: the bound truth [n_save][d][N] (caller memory, read only)
  size_t err_ref_bytes = 0;
  DataLikState datalik;  // cached data log-likelihood of the filter records (odef_data_field)
  Buf obs[5];            // ODEF_L_OBS_SAVE / COMPONENT / VALUE / NOISE / TIME: caller memory, read only
  EventsState events;    // cached event times of the filter and smoothed posterior (odef_event_field)
  Buf evin[2];           // ODEF_EV_SPEC / ODEF_EV_LEVEL: caller memory, read only
  QuantileState quantiles;  // cached ensemble quantiles of the filter, smoothed and dense records (odef_quantile_field)
  Buf qprobs;            // ODEF_Q_PROBS: caller memory, read only
  WSummaryState wsummary;  // cached weighted ensemble summaries of the filter, smoothed and dense records (odef_wsummary_field)
  Buf wlogw;             // ODEF_W_LOGWEIGHT: caller memory, read only
  // odef_group runs its shards concurrently: with `defer` set, odef_solve_* / odef_smooth return after the launch and
  // complete_pending() does the wait + timing (pending: 1 = filter, 2 = smoother)
  bool defer = false;
  int pending = 0;
  // IEKS: ODEF_F_LINEARIZE_AT was filled by odef_smooth (an owned buffer) from the fixed-grid solve on `lin_grid`
  bool lin_set = false;
  std::vector<double> lin_grid;
  mutable std::string err;
};

namespace {

// the field runs on the workgroup-per-trajectory kernels (large state dimension)
bool team_path(const odef_ctx* c) { return c->field->smooth_staged != nullptr; }
// the MV diffusion models :dynamicMV / :fixedMV: d diffusions per record
bool is_mv(int diffusion) { return diffusion == ODEF_DIFFUSION_DYNAMIC_MV || diffusion == ODEF_DIFFUSION_FIXED_MV; }
// the EK1 step: EK1, and IEKS (whose step is EK1 while ODEF_F_LINEARIZE_AT is empty)
bool is_ek1(int alg) { return alg == ODEF_EK1 || alg == ODEF_IEKS; }
// IEKS: ODEF_F_LINEARIZE_AT is bound by the caller or set by odef_smooth (else the step is EK1)
bool lin_active(const odef_ctx* c) { return c->f[ODEF_F_LINEARIZE_AT].bound || c->lin_set; }
// empties ODEF_F_LINEARIZE_AT: a bound buffer is let go, an owned one is kept for the next odef_smooth
void clear_lin(odef_ctx* c) {
  Buf& b = c->f[ODEF_F_LINEARIZE_AT];
  if (b.bound) b = Buf{};
  b.valid = 0;
  c->lin_set = false;
  c->lin_grid.clear();
}

int fail(const odef_ctx* c, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  else g_create_error = buf;
  return -1;
}

#define HIPCHK(c, call)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) return fail((c), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// ibm(d,q) reduced to its (q+1)x(q+1) scalar blocks (src/priors.jl:15-56).
void build_prior(int q, PriorConsts& pc) {
  std::memset(&pc, 0, sizeof pc);
  const int nb = q + 1;
  for (int J = 0; J < nb; ++J) {
    pc.At[J][J] = 1.0;
  }
  {
    double val = 1.0;
    for (int i = 1; i <= q; ++i) {  // A[j, j+d*i] = 1/i!  by the reference's running division
      val = val / i;
      for (int J = 0; J + i < nb; ++J) pc.At[J][J + i] = val;
    }
  }
  auto fact = [](int n) { double f = 1.0; for (int k = 2; k <= n; ++k) f *= k; return f; };
  for (int c = 0; c < nb; ++c)
    for (int r = c; r < nb; ++r) {
      const double idx = 2 * q + 1 - r - c;
      const double v = 1.0 / (idx * fact(q - r) * fact(q - c));
      pc.Qt[r][c] = v;
      pc.Qt[c][r] = v;
    }
  // QLt = cholesky(Qt).L   (chol(Qt (x) I) == chol(Qt) (x) I)
  for (int j = 0; j < nb; ++j) {
    double s = pc.Qt[j][j];
    for (int k = 0; k < j; ++k) s -= pc.QLt[j][k] * pc.QLt[j][k];
    pc.QLt[j][j] = std::sqrt(s);
    for (int i = j + 1; i < nb; ++i) {
      double t = pc.Qt[i][j];
      for (int k = 0; k < j; ++k) t -= pc.QLt[i][k] * pc.QLt[j][k];
      pc.QLt[i][j] = t / pc.QLt[j][j];
    }
  }
}

size_t field_elem(int field) {
  switch (field) {
    case ODEF_F_NACCEPT: case ODEF_F_NREJECT: case ODEF_F_NF: case ODEF_F_NJAC: case ODEF_F_NSAVED: case ODEF_F_RETCODE:
      return sizeof(int32_t);
    default: return sizeof(double);
  }
}

// number of elements of a field for the current solve shape
size_t field_count(const odef_ctx* c, int field, long n_save) {
  const size_t N = (size_t)c->cfg.n_traj;
  switch (field) {
    case ODEF_F_MEAN: case ODEF_F_SMOOTH_MEAN: return (size_t)n_save * c->D * N;
    case ODEF_F_COV_TRIL: case ODEF_F_SMOOTH_COV_TRIL: return (size_t)n_save * c->TRI * N;
    case ODEF_F_DIFFUSION: return (size_t)n_save * (is_mv(c->cfg.diffusion) ? (size_t)c->d : 1) * N;
    case ODEF_F_T: return c->adaptive ? (size_t)n_save * N : (size_t)n_save;
    case ODEF_F_U0: return (size_t)c->d * N;
    case ODEF_F_LINEARIZE_AT: return (size_t)n_save * c->d * N;
    case ODEF_F_DENSE_MEAN: return (size_t)c->n_q * c->D * N;
    case ODEF_F_DENSE_COV_TRIL: return (size_t)c->n_q * c->TRI * N;
    case ODEF_F_SAMPLES: return (size_t)n_save * c->D * (size_t)c->n_samples * N;
    default: return N;
  }
}

int ensure(odef_ctx* c, int field, size_t bytes) {
  Buf& b = c->f[field];
  if (b.bound) {
    if (b.bytes < bytes) return fail(c, "bound buffer for field %d too small: %zu < %zu bytes", field, b.bytes, bytes);
    b.valid = bytes;
    return 0;
  }
  if (b.bytes < bytes) {
    if (b.ptr) HIPCHK(c, hipFree(b.ptr));
    b.ptr = nullptr;
    b.bytes = 0;
    HIPCHK(c, hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
    b.owned = true;
  }
  b.valid = bytes;
  return 0;
}

int ensure_ws(odef_ctx* c, size_t doubles) {
  if (c->ws_cap >= doubles) return 0;
  if (c->d_ws) HIPCHK(c, hipFree(c->d_ws));
  c->d_ws = nullptr;
  c->ws_cap = 0;
  HIPCHK(c, hipMalloc((void**)&c->d_ws, doubles * sizeof(double)));
  c->ws_cap = doubles;
  return 0;
}

// Stage for the covariance records of the workgroup-per-trajectory kernels: as many records as fit in `ODEF_SMOOTH_STAGE_MB`
// (default: a third of the free device memory), at most `want_recs`.  Returns the capacity in doubles (0: work in place).
size_t ensure_stage(odef_ctx* c, long want_recs, size_t per_rec_doubles) {
  if (want_recs < 2) return 0;
  size_t budget;
  if (const char* e = getenv("ODEF_SMOOTH_STAGE_MB")) {
    budget = (size_t)atol(e) << 20;
  } else {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
    budget = (free_b + c->stage_cap * sizeof(double)) / 3;
  }
  size_t recs = budget / (per_rec_doubles * sizeof(double));
  if (recs > (size_t)want_recs) recs = (size_t)want_recs;
  if (recs < 2) return 0;
  const size_t doubles = recs * per_rec_doubles;
  if (c->stage_cap < doubles) {
    if (c->d_stage) (void)hipFree(c->d_stage);
    c->d_stage = nullptr;
    c->stage_cap = 0;
    if (hipMalloc((void**)&c->d_stage, doubles * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    c->stage_cap = doubles;
  }
  return doubles;
}

int set_device(odef_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  return 0;
}

// What an entry point, or a caller holding a writable pointer, may have changed.  Record set k (kFilterRecs << k) is source k of the
// derived outputs.
enum : unsigned {
  kFilterRecs = 1u << 0,    // ODEF_F_MEAN, COV_TRIL, DIFFUSION, T
  kSmoothRecs = 1u << 1,    // ODEF_F_SMOOTH_MEAN, SMOOTH_COV_TRIL
  kDenseRecs = 1u << 2,     // ODEF_F_DENSE_MEAN, DENSE_COV_TRIL
  kAllRecs = kFilterRecs | kSmoothRecs | kDenseRecs,
  kProblem = 1u << 3,       // u0, p, t0
  kTruth = 1u << 4,         // ODEF_E_REFERENCE
  kObservations = 1u << 5,  // ODEF_L_OBS_*
  kEventSpec = 1u << 6,     // ODEF_EV_SPEC, ODEF_EV_LEVEL
  kQuantileProbs = 1u << 7, // ODEF_Q_PROBS
  kLogWeights = 1u << 8,    // ODEF_W_LOGWEIGHT
};

// the record set an ODEF_F_* id belongs to (0: none)
unsigned record_set_of(int field) {
  switch (field) {
    case ODEF_F_MEAN: case ODEF_F_COV_TRIL: case ODEF_F_DIFFUSION: case ODEF_F_T: return kFilterRecs;
    case ODEF_F_SMOOTH_MEAN: case ODEF_F_SMOOTH_COV_TRIL: return kSmoothRecs;
    case ODEF_F_DENSE_MEAN: case ODEF_F_DENSE_COV_TRIL: return kDenseRecs;
    default: return 0;
  }
}

// The one statement of what is computed from what (include/odefilter.h, "Derived outputs and their caches"): everything derived
// from a member of `what` is dropped, and the next request for it runs its pass again.
void records_changed(odef_ctx* c, unsigned what) {
  // summary of source k: record set k -- and the problem, of which it makes no use: the records still on the device answer the
  // problem before, and a summary asked for after odef_set_problem* has always been computed anew
  for (int k = 0; k < 3; ++k)
    if (what & (kFilterRecs << k | kProblem)) c->summary.src[k].valid = false;
  for (int k = 0; k < 2; ++k)  // errors (and the analytic truth) of source k: record set k, the bound truth, the problem
    if (what & (kFilterRecs << k | kTruth | kProblem)) c->errors.src[k].valid = c->errors.src[k].truth_valid = false;
  // data likelihood: the filter records, the observations, the problem
  if (what & (kFilterRecs | kObservations | kProblem)) c->datalik.valid = false;
  for (int k = 0; k < 2; ++k)  // events of source k: record set k, the filter records (both sources predict from them), spec, problem
    if (what & (kFilterRecs << k | kFilterRecs | kEventSpec | kProblem)) c->events.src[k].valid = false;
  for (int k = 0; k < 3; ++k)  // quantiles of source k: record set k, the problem (as for the summary), the bound probabilities
    if (what & (kFilterRecs << k | kProblem | kQuantileProbs)) c->quantiles.src[k].valid = false;
  for (int k = 0; k < 3; ++k)  // weighted summary of source k: record set k, the problem (as for the summary), the bound log-weights
    if (what & (kFilterRecs << k | kProblem | kLogWeights)) c->wsummary.src[k].valid = false;
  // The filter records resident in the stage: the filter records.  odef_smooth works in the stage and leaves the smoothed records
  // (or another block layout) there, so new smoothed records end the residency as well.
  if (what & (kFilterRecs | kSmoothRecs)) c->stage_filter_recs = 0;
}

// One family of derived outputs (odef_summary_field / odef_errors_field / odef_data_field / odef_event_field / odef_quantile_field / odef_wsummary_field).  `check` touches no device; `fetch`
// runs after it and returns the cached device array, running the pass first when the cache is stale.
struct DerivedFamily {
  bool (*owns)(int field);
  int (*check)(const odef_ctx* c, int field, const char* who);  // 0, or -1 with the reason in odef_last_error
  size_t (*bytes)(const odef_ctx* c, int field);
  int (*fetch)(odef_ctx* c, int field, const char* who, void** ptr);
  bool bytes_after_fetch = false;  // the byte count follows from an input in device memory: odef_field_bytes runs the pass as well
};

// odef_summary_field: id = ODEF_S_BASE + 8 source + quantity
bool is_summary_field(int field) {
  return field >= ODEF_S_BASE && field < ODEF_S_BASE + 8 * 3 && (field - ODEF_S_BASE) % 8 < 4;
}

// number of times of a summary source
long summary_times(const odef_ctx* c, int source) { return source == 2 ? c->n_q : c->n_save; }

// what the per-time reductions over the ensemble (summary, quantiles, weighted summary) ask of source 0 / 1 / 2; `what` names the reduction
int ensemble_source_check(const odef_ctx* c, int source, const char* what, const char* who) {
  if (!c->solved) return fail(c, "%s: %s requested before a solve (call odef_solve_* first)", who, what);
  if (source == 2) {
    if (!c->f[ODEF_F_DENSE_MEAN].valid || c->n_q < 1)
      return fail(c, "%s: %s of source 2 needs odef_dense_output (or odef_dense_sample) first", who, what);
    return 0;
  }
  if (c->adaptive)
    return fail(c, "%s: the records of one save index of an adaptive solve lie at different times per trajectory; "
                   "evaluate odef_dense_output at common times and use source 2", who);
  if (source == 1 && !c->smoothed_done) return fail(c, "%s: %s of the smoothed records needs odef_smooth first", who, what);
  return 0;
}

int summary_check(const odef_ctx* c, int field, const char* who) {
  return ensemble_source_check(c, (field - ODEF_S_BASE) / 8, "ensemble summary", who);
}

size_t summary_bytes(const odef_ctx* c, int field) {
  const int source = (field - ODEF_S_BASE) / 8, quantity = (field - ODEF_S_BASE) % 8;
  const size_t tri = (size_t)c->d * (c->d + 1) / 2;
  return (size_t)summary_times(c, source) * 8 * (quantity == 0 ? 1 : quantity == 1 ? (size_t)c->d : tri);
}

// the cached array of a summary field; the first request after the source's records changed runs the reduction
int summary_fetch(odef_ctx* c, int field, const char* who, void** ptr) {
  const int source = (field - ODEF_S_BASE) / 8, quantity = (field - ODEF_S_BASE) % 8;
  const long n_t = summary_times(c, source);
  SummaryCache& sc = c->summary.src[source];
  if (!sc.valid || sc.n_t != n_t) {
    static const int kMean[3] = {ODEF_F_MEAN, ODEF_F_SMOOTH_MEAN, ODEF_F_DENSE_MEAN};
    static const int kCov[3] = {ODEF_F_COV_TRIL, ODEF_F_SMOOTH_COV_TRIL, ODEF_F_DENSE_COV_TRIL};
    SummaryArgs a;
    a.mean = (const double*)c->f[kMean[source]].ptr;
    a.cov = (const double*)c->f[kCov[source]].ptr;
    a.retcode = (const int*)c->f[ODEF_F_RETCODE].ptr;
    a.N = c->cfg.n_traj;
    a.n_t = n_t;
    a.d = c->d;
    a.D = c->D;
    a.TRI = c->TRI;
    if (!a.mean || !a.cov || !a.retcode) return fail(c, "%s: the records of summary source %d hold no data", who, source);
    std::string err;
    int walk = 0;
    if (summary_run(c->summary, sc, a, c->stream, &c->ms[kPassSummary], &c->nl[kPassSummary], &walk, err))
      return fail(c, "%s: %s", who, err.c_str());
    std::snprintf(c->kname[kPassSummary], sizeof c->kname[kPassSummary], "odef::summary_sums_kernel<%d>", walk);
  }
  void* const p[4] = {sc.count, sc.mean, sc.within, sc.between};
  *ptr = p[quantity];
  return 0;
}

// odef_errors_field: id = ODEF_E_BASE + 8 source + quantity (source 0 filter / 1 smoothed records)
bool is_errors_field(int field) {
  return field >= ODEF_E_BASE && field < ODEF_E_BASE + 8 * 2 && (field - ODEF_E_BASE) % 8 <= ODEF_E_U_ANALYTIC - ODEF_E_BASE;
}

size_t errors_bytes(const odef_ctx* c, int field) {
  const size_t N = (size_t)c->cfg.n_traj;
  return (field - ODEF_E_BASE) % 8 == ODEF_E_U_ANALYTIC - ODEF_E_BASE ? (size_t)c->n_save * c->d * N * sizeof(double) : N * 8;
}

int errors_check(const odef_ctx* c, int field, const char* who) {
  const int source = (field - ODEF_E_BASE) / 8;
  if (!c->solved) return fail(c, "%s: solution errors requested before a solve (call odef_solve_* first)", who);
  if (source == 1 && !c->smoothed_done) return fail(c, "%s: solution errors of the smoothed records need odef_smooth first", who);
  if (!c->err_ref && !c->field->errors)
    return fail(c, "%s: nothing to compare with: the vector field (rhs %d) has no `analytic` member and no reference is bound "
                   "(odef_bind_device(ctx, ODEF_E_REFERENCE, [n_save][d][N], bytes))", who, c->cfg.rhs_id);
  if (c->err_ref && c->adaptive)
    return fail(c, "%s: a bound reference [n_save][d][N] belongs to a fixed grid; the saves of an adaptive solve lie at different times "
                   "per trajectory: give the vector field an `analytic` member (and unbind ODEF_E_REFERENCE)", who);
  const size_t need = (size_t)c->n_save * c->d * (size_t)c->cfg.n_traj * sizeof(double);
  if (c->err_ref && c->err_ref_bytes < need)
    return fail(c, "%s: the bound ODEF_E_REFERENCE buffer holds %zu bytes, the records need n_save * d * N * 8 = %zu", who,
                c->err_ref_bytes, need);
  return 0;
}

// the cached array of a solution-error field; the first request after the source's records (or the truth) changed runs the pass
int errors_fetch(odef_ctx* c, int field, const char* who, void** ptr) {
  const int source = (field - ODEF_E_BASE) / 8, quantity = (field - ODEF_E_BASE) % 8;
  ErrorsCache& ec = c->errors.src[source];
  const bool truth = quantity == ODEF_E_U_ANALYTIC - ODEF_E_BASE;
  if (truth && c->err_ref) {  // the truth is the caller's own buffer
    *ptr = const_cast<double*>(c->err_ref);
    return 0;
  }
  if (truth ? !ec.truth_valid : !ec.valid) {
    ErrorsRequest r;
    std::memset(&r, 0, sizeof r);
    r.mean = (const double*)c->f[source ? ODEF_F_SMOOTH_MEAN : ODEF_F_MEAN].ptr;
    r.cov = (const double*)c->f[source ? ODEF_F_SMOOTH_COV_TRIL : ODEF_F_COV_TRIL].ptr;
    r.N = c->cfg.n_traj;
    r.n_save = c->n_save;
    r.d = c->d;
    r.D = c->D;
    r.TRI = c->TRI;
    r.ref = c->err_ref;
    r.field = c->field->errors;
    r.u0 = c->d_u0;
    r.p = c->d_p;
    r.p_shared = c->cfg.params_shared;
    if (c->adaptive) {
      r.tsave = (const double*)c->f[ODEF_F_T].ptr;
      r.nsaved = (const int*)c->f[ODEF_F_NSAVED].ptr;
      r.t = r.tsave;
      r.t_sk = r.N;
      r.t_si = 1;
      if (!r.tsave || !r.nsaved) return fail(c, "%s: the records of source %d hold no data", who, source);
    } else {  // the shared grid; final-save mode keeps the one record of the last time
      r.t = c->d_tgrid + (c->n_save == 1 ? (long)c->tgrid.size() - 1 : 0);
      r.t_sk = 1;
      r.t_si = 0;
    }
    if (!r.mean || !r.cov) return fail(c, "%s: the records of source %d hold no data", who, source);
    std::string err;
    const int rc = truth ? errors_truth(ec, r, c->stream, err)
                         : errors_run(c->errors, ec, r, c->stream, &c->ms[kPassErrors], &c->nl[kPassErrors], c->kname[kPassErrors],
                                      sizeof c->kname[kPassErrors], err);
    if (rc) return fail(c, "%s: %s", who, err.c_str());
  }
  *ptr = truth ? (void*)ec.truth : quantity == ODEF_E_NUSED - ODEF_E_BASE ? (void*)ec.nused : (void*)ec.val[quantity];
  return 0;
}

// odef_data_field: the two outputs, and the five inputs that odef_bind_device alone takes
bool is_datalik_output(int field) { return field == ODEF_L_DATA_LOGLIK || field == ODEF_L_DATA_MAHALANOBIS; }
bool is_datalik_input(int field) { return field >= ODEF_L_OBS_SAVE && field <= ODEF_L_OBS_TIME; }
// the observations are given by time (ODEF_L_OBS_TIME bound: the pass of datalik_times.hip), not by save index
bool datalik_by_time(const odef_ctx* c) { return c->obs[4].ptr != nullptr; }

int datalik_check(const odef_ctx* c, int, const char* who) {
  if (c->obs[0].ptr && c->obs[4].ptr)
    return fail(c, "%s: data log-likelihood: ODEF_L_OBS_SAVE and ODEF_L_OBS_TIME are both bound; the observations are given by save "
                   "index or by time: unbind one of the two (odef_bind_device with NULL)", who);
  if (!c->solved) return fail(c, "%s: data log-likelihood requested before a solve (call odef_solve_* first)", who);
  const bool by_time = datalik_by_time(c);
  if (c->adaptive && !by_time)
    return fail(c, "%s: data log-likelihood after an adaptive solve: the observation times are per ensemble, the grid of an adaptive "
                   "solve is per trajectory; solve on a fixed grid that contains the observation times", who);
  if (is_mv(c->cfg.diffusion))
    return fail(c, "%s: data log-likelihood is built for the scalar diffusion models, not :dynamicMV / :fixedMV", who);
  if (by_time && (team_path(c) || !datalik_times_has(c->d, c->q)))
    return fail(c, "%s: data log-likelihood at observation times has no kernel for (d, q) = (%d, %d); built for d <= 4, q <= 5, "
                   "d (q + 1) <= 12", who, c->d, c->q);
  if (team_path(c) || !datalik_has(c->d, c->q))
    return fail(c, "%s: data log-likelihood has no kernel for (d, q) = (%d, %d); built for d <= 4, q <= 5, d (q + 1) <= 20", who, c->d, c->q);
  if (c->cfg.save_mode != ODEF_SAVE_EVERYSTEP || c->n_save < 2)
    return fail(c, "%s: data log-likelihood needs the records of every step, this context kept only the final state "
                   "(ODEF_SAVE_EVERYSTEP)", who);
  static const char* const kName[4] = {"ODEF_L_OBS_SAVE", "ODEF_L_OBS_COMPONENT", "ODEF_L_OBS_VALUE", "ODEF_L_OBS_NOISE"};
  for (int k = by_time ? 1 : 0; k < 4; ++k)
    if (!c->obs[k].ptr) return fail(c, "%s: data log-likelihood input missing: bind %s with odef_bind_device", who, kName[k]);
  return 0;
}

// the cached array of a data log-likelihood field; the first request after the records or an input changed runs the pass
size_t datalik_bytes(const odef_ctx* c, int) { return (size_t)c->cfg.n_traj * sizeof(double); }

// the part of a request that both data log-likelihood passes take from the context: the filter records and the observed components
int datalik_request(odef_ctx* c, const char* who, DataLikObsRequest& r) {
  r.pc = &c->pc;
  r.N = c->cfg.n_traj;
  r.n_save = c->n_save;
  r.d = c->d;
  r.q = c->q;
  r.mean = (const double*)c->f[ODEF_F_MEAN].ptr;
  r.cov = (const double*)c->f[ODEF_F_COV_TRIL].ptr;
  r.diff = (const double*)c->f[ODEF_F_DIFFUSION].ptr;
  r.obs_comp = c->obs[1].ptr;
  r.obs_val = (const double*)c->obs[2].ptr;
  r.obs_noise = (const double*)c->obs[3].ptr;
  r.comp_bytes = c->obs[1].bytes;
  r.val_bytes = c->obs[2].bytes;
  r.noise_bytes = c->obs[3].bytes;
  if (!r.mean || !r.cov || !r.diff) return fail(c, "%s: the filter records hold no data", who);
  return 0;
}

// the pass over every trajectory's own records with a node per observation time (ODEF_L_OBS_TIME)
int datalik_times_ensure(odef_ctx* c, const char* who) {
  DataLikTimesRequest r{};
  if (datalik_request(c, who, r)) return -1;
  r.adaptive = c->adaptive;
  r.t0 = c->adaptive || c->tgrid.empty() ? c->t0 : c->tgrid.front();
  r.t_last = c->tgrid.empty() ? 0.0 : c->tgrid.back();
  r.tgrid = c->d_tgrid;
  r.tsave = (const double*)c->f[ODEF_F_T].ptr;
  r.nsaved = (const int*)c->f[ODEF_F_NSAVED].ptr;
  if (c->adaptive ? !r.tsave || !r.nsaved : !r.tgrid || (long)c->tgrid.size() != c->n_save)
    return fail(c, "%s: the filter records hold no data", who);
  r.obs_time = (const double*)c->obs[4].ptr;
  r.time_bytes = c->obs[4].bytes;
  std::string err;
  if (datalik_times_run(c->datalik, r, c->stream, &c->ms[kPassDataLik], &c->nl[kPassDataLik], c->kname[kPassDataLik],
                        sizeof c->kname[kPassDataLik], err))
    return fail(c, "%s: %s", who, err.c_str());
  return 0;
}

int datalik_fetch(odef_ctx* c, int field, const char* who, void** ptr) {
  if (!c->datalik.valid && datalik_by_time(c)) {
    if (datalik_times_ensure(c, who)) return -1;
  } else if (!c->datalik.valid) {
    DataLikRequest r{};
    if (datalik_request(c, who, r)) return -1;
    r.ptab = c->d_ptab;
    r.tab_idx = c->d_tab_idx;
    r.hs = c->d_hs;
    if (!r.hs) return fail(c, "%s: the filter records hold no data", who);
    r.obs_save = c->obs[0].ptr;
    r.save_bytes = c->obs[0].bytes;
    std::string err;
    if (datalik_run(c->datalik, r, c->stream, &c->ms[kPassDataLik], &c->nl[kPassDataLik], c->kname[kPassDataLik],
                    sizeof c->kname[kPassDataLik], err))
      return fail(c, "%s: %s", who, err.c_str());
  }
  *ptr = c->datalik.out[field - ODEF_L_BASE];
  return 0;
}

// odef_event_field: id = ODEF_EV_BASE + 8 source + quantity, and the two inputs that odef_bind_device alone takes
bool is_event_output(int field) {
  return field >= ODEF_EV_BASE && field < ODEF_EV_BASE + 8 * 2 && (field - ODEF_EV_BASE) % 8 <= ODEF_EV_NEVAL - ODEF_EV_BASE;
}
bool is_event_input(int field) { return field == ODEF_EV_SPEC || field == ODEF_EV_LEVEL; }

int events_check(const odef_ctx* c, int field, const char* who) {
  const int source = (field - ODEF_EV_BASE) / 8;
  if (!c->solved) return fail(c, "%s: event location requested before a solve (call odef_solve_* first)", who);
  if (source == 1 && !c->smoothed_done) return fail(c, "%s: event location on the smoothed posterior needs odef_smooth first", who);
  if (c->cfg.save_mode != ODEF_SAVE_EVERYSTEP || c->n_save < 2)
    return fail(c, "%s: event location needs the records of every step, this context kept only the final state "
                   "(ODEF_SAVE_EVERYSTEP)", who);
  if (is_mv(c->cfg.diffusion))
    return fail(c, "%s: event location is built for the scalar diffusion models, not :dynamicMV / :fixedMV", who);
  if (!events_has(c->d, c->q))
    return fail(c, "%s: event location has no kernel for (d, q) = (%d, %d); built for d <= 4, q <= 5, d (q + 1) <= 12", who, c->d, c->q);
  static const char* const kName[2] = {"ODEF_EV_SPEC", "ODEF_EV_LEVEL"};
  for (int k = 0; k < 2; ++k)
    if (!c->evin[k].ptr) return fail(c, "%s: event location input missing: bind %s with odef_bind_device", who, kName[k]);
  if (c->evin[0].bytes != 24)
    return fail(c, "%s: event location: ODEF_EV_SPEC holds %zu bytes, it is [3] int64 {component, direction, K} = 24", who,
                c->evin[0].bytes);
  if (c->evin[1].bytes != 8 && c->evin[1].bytes != (size_t)c->cfg.n_traj * 8)
    return fail(c, "%s: event location: ODEF_EV_LEVEL holds %zu bytes, it is one double (8) or one per trajectory (%zu)", who,
                c->evin[1].bytes, (size_t)c->cfg.n_traj * 8);
  return 0;
}

// runs the pass of a source when its cache is stale (the byte counts of all but COUNT depend on K, which the pass validates)
int events_ensure(odef_ctx* c, int source, const char* who) {
  EventsCache& ec = c->events.src[source];
  if (ec.valid) return 0;
  EventsRequest r;
  std::memset(&r, 0, sizeof r);
  r.pc = &c->pc;
  r.N = c->cfg.n_traj;
  r.n_save = c->n_save;
  r.d = c->d;
  r.q = c->q;
  r.adaptive = c->adaptive;
  r.source = source;
  r.tgrid = c->d_tgrid;
  r.tsave = (const double*)c->f[ODEF_F_T].ptr;
  r.nsaved = (const int*)c->f[ODEF_F_NSAVED].ptr;
  r.mean = (const double*)c->f[ODEF_F_MEAN].ptr;
  r.cov = (const double*)c->f[ODEF_F_COV_TRIL].ptr;
  r.diff = (const double*)c->f[ODEF_F_DIFFUSION].ptr;
  r.smean = (const double*)c->f[ODEF_F_SMOOTH_MEAN].ptr;
  r.scov = (const double*)c->f[ODEF_F_SMOOTH_COV_TRIL].ptr;
  if (!r.mean || !r.cov || !r.diff || (c->adaptive ? !r.tsave || !r.nsaved : !r.tgrid) || (source == 1 && (!r.smean || !r.scov)))
    return fail(c, "%s: the records of event source %d hold no data", who, source);
  r.spec = c->evin[0].ptr;
  r.level = (const double*)c->evin[1].ptr;
  r.spec_bytes = c->evin[0].bytes;
  r.level_bytes = c->evin[1].bytes;
  std::string err;
  if (set_device(c)) return -1;
  if (events_run(c->events, ec, r, c->stream, &c->ms[kPassEvents], &c->nl[kPassEvents], c->kname[kPassEvents],
                 sizeof c->kname[kPassEvents], err))
    return fail(c, "%s: %s", who, err.c_str());
  return 0;
}

int events_fetch(odef_ctx* c, int field, const char* who, void** ptr) {
  const int source = (field - ODEF_EV_BASE) / 8, quantity = (field - ODEF_EV_BASE) % 8;
  if (events_ensure(c, source, who)) return -1;
  const EventsCache& ec = c->events.src[source];
  void* const p[7] = {ec.count, ec.time, ec.tvar, ec.u, ec.direction, ec.save, ec.neval};
  *ptr = p[quantity];
  return 0;
}

// (K lives in device memory and is known once the pass has run: called after events_fetch only)
size_t events_bytes(const odef_ctx* c, int field) {
  const int source = (field - ODEF_EV_BASE) / 8, quantity = (field - ODEF_EV_BASE) % 8;
  const size_t N = (size_t)c->cfg.n_traj, K = (size_t)c->events.src[source].K;
  switch (quantity) {
    case 0: return N * sizeof(int32_t);
    case 1: case 2: return K * N * sizeof(double);
    case 3: return K * (size_t)c->d * N * sizeof(double);
    default: return K * N * sizeof(int32_t);
  }
}

// odef_quantile_field: id = ODEF_Q_BASE + 8 source + quantity (0: the quantiles, 1: the count), and the input that odef_bind_device
// alone takes
bool is_quantile_output(int field) {
  return field >= ODEF_Q_BASE && field < ODEF_Q_BASE + 8 * 3 && (field - ODEF_Q_BASE) % 8 < 2;
}

int quantiles_check(const odef_ctx* c, int field, const char* who) {
  if (ensemble_source_check(c, (field - ODEF_Q_BASE) / 8, "ensemble quantiles", who)) return -1;
  if (c->d > 32) return fail(c, "%s: ensemble quantiles are built for d <= 32 (got d = %d)", who, c->d);
  if (!c->qprobs.ptr)
    return fail(c, "%s: ensemble quantiles: no probabilities bound: bind ODEF_Q_PROBS (double [P], 1 <= P <= 8) with odef_bind_device", who);
  if (c->qprobs.bytes % sizeof(double) != 0 || c->qprobs.bytes < sizeof(double) || c->qprobs.bytes > 8 * sizeof(double))
    return fail(c, "%s: ensemble quantiles: ODEF_Q_PROBS holds %zu bytes, it is double [P] with 1 <= P <= 8", who, c->qprobs.bytes);
  return 0;
}

size_t quantiles_bytes(const odef_ctx* c, int field) {
  const int source = (field - ODEF_Q_BASE) / 8, quantity = (field - ODEF_Q_BASE) % 8;
  const size_t P = c->qprobs.bytes / sizeof(double);
  return (size_t)summary_times(c, source) * 8 * (quantity == 1 ? 1 : P * (size_t)c->d);
}

// the cached array of a quantile field; the first request after the source's records or the probabilities changed runs the pass
int quantiles_fetch(odef_ctx* c, int field, const char* who, void** ptr) {
  const int source = (field - ODEF_Q_BASE) / 8, quantity = (field - ODEF_Q_BASE) % 8;
  const long n_t = summary_times(c, source);
  const int P = (int)(c->qprobs.bytes / sizeof(double));
  QuantileCache& qc = c->quantiles.src[source];
  if (!qc.valid || qc.n_t != n_t || qc.P != P) {
    static const int kMean[3] = {ODEF_F_MEAN, ODEF_F_SMOOTH_MEAN, ODEF_F_DENSE_MEAN};
    QuantileArgs a{};
    a.mean = (const double*)c->f[kMean[source]].ptr;
    a.retcode = (const int*)c->f[ODEF_F_RETCODE].ptr;
    a.N = c->cfg.n_traj;
    a.n_t = n_t;
    a.d = c->d;
    a.D = c->D;
    a.P = P;
    if (!a.mean || !a.retcode) return fail(c, "%s: the records of quantile source %d hold no data", who, source);
    // the probabilities are copied to the host and validated there
    HIPCHK(c, hipMemcpyAsync(a.probs, c->qprobs.ptr, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p < P; ++p)
      if (!(a.probs[p] >= 0.0 && a.probs[p] <= 1.0))
        return fail(c, "%s: ensemble quantiles: probability %d of ODEF_Q_PROBS is %g, outside [0, 1]", who, p, a.probs[p]);
    std::string err;
    if (quantiles_run(c->quantiles, qc, a, c->stream, &c->ms[kPassQuantiles], &c->nl[kPassQuantiles], err))
      return fail(c, "%s: %s", who, err.c_str());
    std::snprintf(c->kname[kPassQuantiles], sizeof c->kname[kPassQuantiles], "odef::quantile_hist_kernel");
  }
  *ptr = quantity == 1 ? (void*)qc.count : (void*)qc.q;
  return 0;
}

// odef_wsummary_field: id = ODEF_W_BASE + 8 source + quantity (0..5 as in the header's table), and the input that odef_bind_device
// alone takes
bool is_wsummary_output(int field) {
  return field >= ODEF_W_BASE && field < ODEF_W_BASE + 8 * 3 && (field - ODEF_W_BASE) % 8 < 6;
}

int wsummary_check(const odef_ctx* c, int field, const char* who) {
  if (ensemble_source_check(c, (field - ODEF_W_BASE) / 8, "weighted ensemble summary", who)) return -1;
  if (c->d > 32) return fail(c, "%s: the weighted ensemble summary is built for d <= 32 (got d = %d)", who, c->d);
  if (!c->wlogw.ptr)
    return fail(c, "%s: weighted ensemble summary: no weights bound: bind ODEF_W_LOGWEIGHT (double [N]) with odef_bind_device", who);
  return 0;
}

size_t wsummary_bytes(const odef_ctx* c, int field) {
  const int source = (field - ODEF_W_BASE) / 8, quantity = (field - ODEF_W_BASE) % 8;
  const size_t tri = (size_t)c->d * (c->d + 1) / 2;
  const size_t per_time[6] = {1, (size_t)c->d, tri, tri, 1, 1};
  return (size_t)summary_times(c, source) * 8 * per_time[quantity];
}

// the cached array of a weighted-summary field; the first request after the source's records or the weights changed runs the pass
int wsummary_fetch(odef_ctx* c, int field, const char* who, void** ptr) {
  const int source = (field - ODEF_W_BASE) / 8, quantity = (field - ODEF_W_BASE) % 8;
  const long n_t = summary_times(c, source);
  WSummaryCache& wc = c->wsummary.src[source];
  if (!wc.valid || wc.n_t != n_t) {
    static const int kMean[3] = {ODEF_F_MEAN, ODEF_F_SMOOTH_MEAN, ODEF_F_DENSE_MEAN};
    static const int kCov[3] = {ODEF_F_COV_TRIL, ODEF_F_SMOOTH_COV_TRIL, ODEF_F_DENSE_COV_TRIL};
    WSummaryArgs a;
    a.mean = (const double*)c->f[kMean[source]].ptr;
    a.cov = (const double*)c->f[kCov[source]].ptr;
    a.retcode = (const int*)c->f[ODEF_F_RETCODE].ptr;
    a.logw = (const double*)c->wlogw.ptr;
    a.N = c->cfg.n_traj;
    a.n_t = n_t;
    a.d = c->d;
    a.D = c->D;
    a.TRI = c->TRI;
    if (!a.mean || !a.cov || !a.retcode) return fail(c, "%s: the records of summary source %d hold no data", who, source);
    std::string err;
    int walk = 0;
    if (wsummary_run(c->wsummary, wc, a, c->stream, &c->ms[kPassWSummary], &c->nl[kPassWSummary], &walk, err))
      return fail(c, "%s: %s", who, err.c_str());
    std::snprintf(c->kname[kPassWSummary], sizeof c->kname[kPassWSummary], "odef::wsummary_sums_kernel<%d>", walk);
  }
  void* const p[6] = {wc.count, wc.mean, wc.within, wc.between, wc.logev, wc.ess};
  *ptr = p[quantity];
  return 0;
}

const DerivedFamily kDerived[] = {
    {is_summary_field, summary_check, summary_bytes, summary_fetch},
    {is_errors_field, errors_check, errors_bytes, errors_fetch},
    {is_datalik_output, datalik_check, datalik_bytes, datalik_fetch},
    {is_event_output, events_check, events_bytes, events_fetch, true},
    {is_quantile_output, quantiles_check, quantiles_bytes, quantiles_fetch},
    {is_wsummary_output, wsummary_check, wsummary_bytes, wsummary_fetch},
};

// the family that owns a field id, or nullptr: an ODEF_F_* buffer, a bind-only id, or no id at all
const DerivedFamily* derived_family(int field) {
  for (const DerivedFamily& fam : kDerived)
    if (fam.owns(field)) return &fam;
  return nullptr;
}

// the device array and byte count of a derived field
int derived_fetch(odef_ctx* c, const DerivedFamily* fam, int field, const char* who, void** ptr, size_t* bytes) {
  if (fam->check(c, field, who) || set_device(c) || fam->fetch(c, field, who, ptr)) return -1;
  *bytes = fam->bytes(c, field);
  return 0;
}

__global__ void transpose_in_kernel(const double* __restrict__ src /*[N][k]*/, double* __restrict__ dst /*[k][N]*/,
                                    long N, int k) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int a = 0; a < k; ++a) dst[(size_t)a * N + i] = src[(size_t)i * k + a];
}

__device__ inline unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct PerturbArgs { double base[32]; };

__global__ void perturbed_u0_kernel(PerturbArgs a, double* __restrict__ dst /*[d][N]*/, long N, int d, int n_pert,
                                    double scale, unsigned long long seed, long first) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int k = 0; k < d; ++k) {
    double v = a.base[k];
    if (k < n_pert) {
#pragma clang fp contract(off)
      const unsigned long long r = splitmix64(seed + (unsigned long long)n_pert * (unsigned long long)(first + i) + k);
      const double U = (double)(r >> 11) * 0x1.0p-53;
      // separate roundings (no FMA contraction) so that the ensemble is bit-identical to the host generators
      const double w = 2.0 * U - 1.0;
      const double sw = scale * w;
      v = a.base[k] + sw;
    }
    dst[(size_t)k * N + i] = v;
  }
}

__global__ void scale_cov_kernel(double* __restrict__ cov, double* __restrict__ diff, double* __restrict__ loglik,
                                 const int* __restrict__ nsaved, long N, long n_save_fixed, int TRI) {
  // postamble! for static diffusion (src/integrator_utils.jl:4-18): Sigma *= final_diff, diffusions .= final_diff,
  // sol.log_likelihood = NaN.  nsaved != nullptr: adaptive solve, per-trajectory record count.
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const long n_save = nsaved ? (long)nsaved[i] : n_save_fixed;
  const bool final_only = !nsaved && n_save_fixed == 1;  // final-save mode: slot 0 holds the last state and the last global diffusion
  if (!final_only && n_save < 2) {  // no step taken: sol.diffusions is empty, nothing to rescale
    loglik[i] = __builtin_nan("");
    return;
  }
  const double s = diff[(size_t)(n_save - 1) * N + i];
  for (long n = 0; n < n_save; ++n) {
    for (int k = 0; k < TRI; ++k) cov[((size_t)n * TRI + k) * N + i] *= s;
    if (n >= 1) diff[(size_t)n * N + i] = s;
  }
  loglik[i] = __builtin_nan("");
}

// postamble! of :fixedMV (src/integrator_utils.jl:4-18): with the final global diffusion diag(s_1 .. s_d) of the trajectory,
// every filter covariance becomes sqrt(D) Sigma sqrt(D), D = kron(I, diag(s)) -- entry ((J, a), (K, b)) times sqrt(s_a s_b) --,
// every diffusion record becomes the final one, sol.log_likelihood = NaN.  diff: [n_save][d][N].
__global__ void scale_cov_mv_kernel(double* __restrict__ cov, double* __restrict__ diff, double* __restrict__ loglik,
                                    const int* __restrict__ nsaved, long N, long n_save_fixed, int d, int D) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const long n_save = nsaved ? (long)nsaved[i] : n_save_fixed;
  const bool final_only = !nsaved && n_save_fixed == 1;
  if (!final_only && n_save < 2) {
    loglik[i] = __builtin_nan("");
    return;
  }
  double fin[10], rs[10];  // s_a and sqrt(s_a); odef_create admits the MV models for d <= 10 only
  for (int a = 0; a < d; ++a) {
    fin[a] = diff[((size_t)(n_save - 1) * d + a) * N + i];
    rs[a] = sqrt(fin[a]);
  }
  for (long n = 0; n < n_save; ++n) {
    for (int r = 0; r < D; ++r)
      for (int c = 0; c <= r; ++c) {
        const size_t k = (size_t)r * (r + 1) / 2 + c;
        cov[((size_t)n * D * (D + 1) / 2 + k) * N + i] *= rs[r % d] * rs[c % d];
      }
    if (n >= 1)
      for (int a = 0; a < d; ++a) diff[((size_t)n * d + a) * N + i] = fin[a];
  }
  loglik[i] = __builtin_nan("");
}

}  // namespace

extern "C" {

int odef_version(void) { return ODEF_VERSION; }

const char* odef_last_error(const odef_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int odef_rhs_compile(const char* name, const char* source, int32_t d, int32_t n_params, const char* include_dir, int32_t* rhs_id) {
  if (!rhs_id) return fail(nullptr, "odef_rhs_compile: null rhs_id");
  std::string err;
  const int id = jit_register(name, source, d, n_params, include_dir, err);
  if (id < 0) {
    g_create_error = err;  // the whole compiler log, not truncated
    return -1;
  }
  *rhs_id = id;
  return 0;
}

int odef_create(odef_ctx** out, const odef_config* cfg) {
  if (!out || !cfg) return fail(nullptr, "odef_create: null argument");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(odef_config))
    return fail(nullptr, "odef_create: struct_size %d != %zu", cfg->struct_size, sizeof(odef_config));
  RhsInfo ri{0, 0};
  if (cfg->rhs_id >= kJitFirstId) {
    if (!jit_lookup(cfg->rhs_id, &ri.d, &ri.np)) return fail(nullptr, "odef_create: unknown run-time rhs_id %d", cfg->rhs_id);
  } else {
    if (cfg->rhs_id < 0 || cfg->rhs_id > ODEF_RHS_FORCED) return fail(nullptr, "odef_create: unknown rhs_id %d", cfg->rhs_id);
    ri = kRhs[cfg->rhs_id];
  }
  if (cfg->d != ri.d) return fail(nullptr, "odef_create: rhs %d has dimension %d, got d=%d", cfg->rhs_id, ri.d, cfg->d);
  if (cfg->n_params != ri.np) return fail(nullptr, "odef_create: rhs %d has %d parameters, got %d", cfg->rhs_id, ri.np, cfg->n_params);
  if (cfg->order < 1 || cfg->order > ODEF_MAX_ORDER) return fail(nullptr, "odef_create: order %d outside 1..%d", cfg->order, ODEF_MAX_ORDER);
  if (cfg->alg != ODEF_EK0 && cfg->alg != ODEF_EK1 && cfg->alg != ODEF_IEKS) return fail(nullptr, "odef_create: unknown alg %d", cfg->alg);
  if (cfg->diffusion != ODEF_DIFFUSION_DYNAMIC && cfg->diffusion != ODEF_DIFFUSION_FIXED && cfg->diffusion != ODEF_DIFFUSION_FIXED_MAP &&
      !is_mv(cfg->diffusion))
    return fail(nullptr, "odef_create: unknown diffusion model %d", cfg->diffusion);
  if (is_mv(cfg->diffusion)) {
    // the reference asserts H == E1 * PI (src/diffusions.jl:96, :125)
    if (cfg->alg != ODEF_EK0) return fail(nullptr, "odef_create: MV diffusion models require EK0");
    // the MV models are built on the lane / row-team kernels only
    const bool team = cfg->rhs_id >= kJitFirstId ? jit_team_path(cfg->d, cfg->order)
                                                 : (cfg->rhs_id == ODEF_RHS_PLEIADES || cfg->rhs_id == ODEF_RHS_LORENZ96);
    if (team)
      return fail(nullptr, "odef_create: MV diffusion models run on the lane kernels only (state dimension d(q+1) <= 20, d <= 10); "
                           "rhs %d with d = %d, d(q+1) = %d runs on the workgroup-per-trajectory kernels", cfg->rhs_id, cfg->d,
                  cfg->d * (cfg->order + 1));
  }
  if (cfg->alg == ODEF_IEKS) {
    if (!cfg->smooth) return fail(nullptr, "odef_create: IEKS always smooths (smooth = 1)");  // src/ieks.jl:39
    // the IEKS step is built on the lane / row-team kernels only
    const bool team = cfg->rhs_id >= kJitFirstId ? jit_team_path(cfg->d, cfg->order)
                                                 : (cfg->rhs_id == ODEF_RHS_PLEIADES || cfg->rhs_id == ODEF_RHS_LORENZ96);
    if (team)
      return fail(nullptr, "odef_create: IEKS runs on the lane kernels only (state dimension d(q+1) <= 20, d <= 10); "
                           "rhs %d with d = %d, d(q+1) = %d runs on the workgroup-per-trajectory kernels", cfg->rhs_id, cfg->d,
                  cfg->d * (cfg->order + 1));
  }
  if (cfg->n_traj <= 0) return fail(nullptr, "odef_create: n_traj must be positive");
  // a time-dependent run-time field (has_time, csrc/rhs.h): the workgroup-per-trajectory kernels carry no time
  if (cfg->rhs_id >= kJitFirstId && jit_has_time(cfg->rhs_id) && jit_team_path(cfg->d, cfg->order))
    return fail(nullptr, "odef_create: time-dependent fields run on the lane and row-team kernels (state dimension d(q+1) <= 20, d <= 10); "
                         "rhs %d with d = %d, d(q+1) = %d would need the workgroup-per-trajectory kernels", cfg->rhs_id, cfg->d,
                cfg->d * (cfg->order + 1));
  // run-time compiled fields: lane / row-team kernels up to state dimension 20 (d <= 10), the workgroup-per-trajectory kernels above
  if (cfg->rhs_id >= kJitFirstId && jit_team_path(cfg->d, cfg->order) && (cfg->d % 2 != 0 || cfg->d > 32 || cfg->d * (cfg->order + 1) > 176))
    return fail(nullptr, "odef_create: run-time compiled vector fields above state dimension 20 run on the workgroup-per-trajectory kernels: even d <= 32 and d(q+1) <= 176 (got d = %d, d(q+1) = %d)",
                cfg->d, cfg->d * (cfg->order + 1));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, "odef_create: no HIP device available (libodefilter_hip has no CPU path)");
  odef_ctx* c = new odef_ctx();
  c->cfg = *cfg;
  if (c->cfg.smooth) c->cfg.save_mode = ODEF_SAVE_EVERYSTEP;
  c->d = cfg->d;
  c->q = cfg->order;
  c->D = c->d * (c->q + 1);
  c->TRI = c->D * (c->D + 1) / 2;
  c->np = cfg->n_params;
  if (cfg->device >= 0) c->device = cfg->device;
  else if (hipGetDevice(&c->device) != hipSuccess) c->device = 0;
  if (c->device >= ndev) { delete c; return fail(nullptr, "odef_create: device %d not present (%d devices)", cfg->device, ndev); }
  build_prior(c->q, c->pc);
  c->field = field_launch(cfg->rhs_id);
  if (!c->field) {
    std::string jerr;
    c->field = jit_field(cfg->rhs_id, c->q, is_ek1(cfg->alg), is_mv(cfg->diffusion), cfg->alg == ODEF_IEKS, team_abi_stamp(), jerr);
    if (!c->field) {
      g_create_error = "odef_create: " + jerr;  // the whole compiler log
      delete c;
      return -1;
    }
  }
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&c->ev[k]);
  const size_t N = (size_t)cfg->n_traj;
  if (e == hipSuccess) e = hipMalloc((void**)&c->d_u0, sizeof(double) * c->d * N);
  if (e == hipSuccess && c->np > 0) e = hipMalloc((void**)&c->d_p, sizeof(double) * c->np * (cfg->params_shared ? 1 : N));
  if (e != hipSuccess) {
    fail(nullptr, "odef_create: HIP setup failed: %s", hipGetErrorString(e));
    odef_destroy(c);
    return -1;
  }
  c->stream = c->own_stream;
  c->f[ODEF_F_U0].ptr = c->d_u0;
  c->f[ODEF_F_U0].bytes = c->f[ODEF_F_U0].valid = sizeof(double) * c->d * N;
  *out = c;
  return 0;
}

void odef_destroy(odef_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  for (int k = 0; k < ODEF_F_COUNT_; ++k)
    if (k != ODEF_F_U0 && c->f[k].owned && c->f[k].ptr) (void)hipFree(c->f[k].ptr);
  free_device(c->d_u0, c->d_p, c->d_ws, c->d_stage, c->d_hs, c->d_ptab, c->d_tgrid, c->d_tq, c->d_tab_idx);
  summary_free(c->summary);
  errors_free(c->errors);
  datalik_free(c->datalik);
  events_free(c->events);
  quantiles_free(c->quantiles);
  wsummary_free(c->wsummary);
  for (int k = 0; k < 4; ++k)
    if (c->ev[k]) (void)hipEventDestroy(c->ev[k]);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int odef_set_stream(odef_ctx* c, void* hip_stream) {
  if (!c) return -1;
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return 0;
}

int odef_set_problem(odef_ctx* c, const double* u0, const double* p, double t0) {
  if (!c || !u0) return fail(c, "odef_set_problem: null argument");
  if (c->np > 0 && !p) return fail(c, "odef_set_problem: parameters required");
  if (set_device(c)) return -1;
  const long N = c->cfg.n_traj;
  double* tmp = nullptr;
  const size_t ub = sizeof(double) * c->d * N;
  const size_t pb = (c->np > 0 && !c->cfg.params_shared) ? sizeof(double) * c->np * N : 0;
  HIPCHK(c, hipMalloc((void**)&tmp, ub > pb ? ub : pb));
  HIPCHK(c, hipMemcpyAsync(tmp, u0, ub, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(transpose_in_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, tmp, c->d_u0, N, c->d);
  if (c->np > 0) {
    if (c->cfg.params_shared) {
      HIPCHK(c, hipMemcpyAsync(c->d_p, p, sizeof(double) * c->np, hipMemcpyHostToDevice, c->stream));
    } else {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipMemcpyAsync(tmp, p, pb, hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(transpose_in_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, tmp, c->d_p, N, c->np);
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipFree(tmp));
  c->t0 = t0;
  c->have_problem = true;
  clear_lin(c);
  records_changed(c, kProblem);
  return 0;
}

int odef_set_problem_device(odef_ctx* c, const double* d_u0, const double* d_p, double t0) {
  if (!c || !d_u0) return fail(c, "odef_set_problem_device: null argument");
  if (c->np > 0 && !d_p) return fail(c, "odef_set_problem_device: parameters required");
  if (set_device(c)) return -1;
  const size_t N = (size_t)c->cfg.n_traj;
  HIPCHK(c, hipMemcpyAsync(c->d_u0, d_u0, sizeof(double) * c->d * N, hipMemcpyDeviceToDevice, c->stream));
  if (c->np > 0)
    HIPCHK(c, hipMemcpyAsync(c->d_p, d_p, sizeof(double) * c->np * (c->cfg.params_shared ? 1 : N), hipMemcpyDeviceToDevice, c->stream));
  c->t0 = t0;
  c->have_problem = true;
  clear_lin(c);
  records_changed(c, kProblem);
  return 0;
}

int odef_set_problem_perturbed(odef_ctx* c, const double* base_u0, const double* p, double t0, double scale,
                               uint64_t seed, int64_t first_index, int32_t n_perturbed) {
  if (!c || !base_u0) return fail(c, "odef_set_problem_perturbed: null argument");
  if (c->np > 0 && !p) return fail(c, "odef_set_problem_perturbed: parameters required");
  if (!c->cfg.params_shared && c->np > 0) return fail(c, "odef_set_problem_perturbed: needs params_shared = 1");
  if (n_perturbed < 0 || n_perturbed > c->d) return fail(c, "odef_set_problem_perturbed: n_perturbed %d outside 0..%d", n_perturbed, c->d);
  if (set_device(c)) return -1;
  PerturbArgs a;
  for (int k = 0; k < c->d; ++k) a.base[k] = base_u0[k];
  const long N = c->cfg.n_traj;
  hipLaunchKernelGGL(perturbed_u0_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, a, c->d_u0, N, c->d,
                     (int)n_perturbed, scale, (unsigned long long)seed, (long)first_index);
  HIPCHK(c, hipGetLastError());
  if (c->np > 0) HIPCHK(c, hipMemcpyAsync(c->d_p, p, sizeof(double) * c->np, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->t0 = t0;
  c->have_problem = true;
  clear_lin(c);
  records_changed(c, kProblem);
  return 0;
}

// the buffers of a new solve
static int alloc_outputs(odef_ctx* c, long n_save) {
  // The solve rewrites the filter records and RETCODE, by which every summary source includes its trajectories; the smoothed
  // records belong to the solve before.  Said before the launch: a solve that fails half way leaves no cache of the old records
  // behind, and the launch is then free to note the records it leaves in the stage (FieldLaunch::filter).
  records_changed(c, kAllRecs);
  static const int per_save[] = {ODEF_F_MEAN, ODEF_F_COV_TRIL, ODEF_F_DIFFUSION};
  for (int f : per_save)
    if (ensure(c, f, field_count(c, f, n_save) * sizeof(double))) return -1;
  if (c->adaptive && ensure(c, ODEF_F_T, field_count(c, ODEF_F_T, n_save) * sizeof(double))) return -1;
  static const int per_traj[] = {ODEF_F_LOGLIK, ODEF_F_NACCEPT, ODEF_F_NREJECT, ODEF_F_NF, ODEF_F_NJAC, ODEF_F_NSAVED, ODEF_F_RETCODE};
  for (int f : per_traj)
    if (ensure(c, f, (size_t)c->cfg.n_traj * field_elem(f))) return -1;
  return 0;
}

static void fill_params(odef_ctx* c, FilterParams& P) {
  std::memset(&P, 0, sizeof P);
  P.pc = c->pc;
  P.u0 = c->d_u0;
  P.p = c->d_p;
  P.p_shared = c->cfg.params_shared;
  P.N = c->cfg.n_traj;
  P.everystep = c->cfg.save_mode == ODEF_SAVE_EVERYSTEP;
  P.fixed_diffusion = (int)c->cfg.diffusion;  // 0 dynamic, 1 fixed, 2 fixedMAP (static_diffusion_update, ek_math.h), 3 / 4 dynamicMV / fixedMV
  P.want_loglik = c->cfg.want_loglik;
  {
    const char* e = getenv("ODEF_STAGGER");
    P.stagger = e ? atoi(e) : 0;
  }
  P.mean = (double*)c->f[ODEF_F_MEAN].ptr;
  P.cov = (double*)c->f[ODEF_F_COV_TRIL].ptr;
  P.diff = (double*)c->f[ODEF_F_DIFFUSION].ptr;
  P.tsave = (double*)c->f[ODEF_F_T].ptr;
  P.loglik = (double*)c->f[ODEF_F_LOGLIK].ptr;
  P.naccept = (int*)c->f[ODEF_F_NACCEPT].ptr;
  P.nreject = (int*)c->f[ODEF_F_NREJECT].ptr;
  P.nf = (int*)c->f[ODEF_F_NF].ptr;
  P.njac = (int*)c->f[ODEF_F_NJAC].ptr;
  P.nsaved = (int*)c->f[ODEF_F_NSAVED].ptr;
  P.retcode = (int*)c->f[ODEF_F_RETCODE].ptr;
}

static int complete_pending(odef_ctx* c) {
  if (c->pending == 1) {
    HIPCHK(c, hipEventSynchronize(c->ev[1]));
    HIPCHK(c, hipEventElapsedTime(&c->ms[kPassFilter], c->ev[0], c->ev[1]));
  } else if (c->pending == 2) {
    HIPCHK(c, hipEventSynchronize(c->ev[3]));
    HIPCHK(c, hipEventElapsedTime(&c->ms[kPassSmooth], c->ev[2], c->ev[3]));
  }
  c->pending = 0;
  return 0;
}

static int finish_filter(odef_ctx* c, int nlaunch) {
  // static diffusion: rescale all covariances by the final global diffusion (src/integrator_utils.jl:4-18)
  if (c->cfg.diffusion == ODEF_DIFFUSION_FIXED_MV) {
    const long N = c->cfg.n_traj;
    hipLaunchKernelGGL(scale_cov_mv_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, c->stream,
                       (double*)c->f[ODEF_F_COV_TRIL].ptr, (double*)c->f[ODEF_F_DIFFUSION].ptr,
                       (double*)c->f[ODEF_F_LOGLIK].ptr, c->adaptive ? (const int*)c->f[ODEF_F_NSAVED].ptr : (const int*)nullptr,
                       N, c->n_save, c->d, c->D);
    ++nlaunch;
    records_changed(c, kFilterRecs);
  } else if (c->cfg.diffusion != ODEF_DIFFUSION_DYNAMIC && c->cfg.diffusion != ODEF_DIFFUSION_DYNAMIC_MV) {
    const long N = c->cfg.n_traj;
    hipLaunchKernelGGL(scale_cov_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, c->stream,
                       (double*)c->f[ODEF_F_COV_TRIL].ptr, (double*)c->f[ODEF_F_DIFFUSION].ptr,
                       (double*)c->f[ODEF_F_LOGLIK].ptr, c->adaptive ? (const int*)c->f[ODEF_F_NSAVED].ptr : (const int*)nullptr,
                       N, c->n_save, c->TRI);
    ++nlaunch;
    records_changed(c, kFilterRecs);  // (records the filter may have left in the stage are the unscaled ones)
  }
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipGetLastError());
  c->nl[kPassFilter] = nlaunch;
  c->solved = true;
  c->smoothed_done = false;
  c->pending = 1;
  return c->defer ? 0 : complete_pending(c);
}

int odef_solve_fixed(odef_ctx* c, const double* tgrid, int64_t n_t) {
  if (!c || !tgrid) return fail(c, "odef_solve_fixed: null argument");
  if (!c->have_problem) return fail(c, "odef_solve_fixed: call odef_set_problem first");
  if (n_t < 2) return fail(c, "odef_solve_fixed: need at least two grid points (adaptive=false requires a dt)");
  if (tgrid[0] != c->t0) return fail(c, "odef_solve_fixed: tgrid[0] = %g differs from t0 = %g", tgrid[0], c->t0);
  for (int64_t n = 0; n + 1 < n_t; ++n)
    if (!(tgrid[n + 1] > tgrid[n])) return fail(c, "odef_solve_fixed: tgrid must be strictly increasing (index %lld)", (long long)n);
  // IEKS: the linearisation points of this iterate (alg.linearize_at = sol, src/ieks.jl:56-61), row s + 1 for step s -> s + 1
  const double* lin = nullptr;
  if (c->cfg.alg == ODEF_IEKS && lin_active(c)) {
    Buf& b = c->f[ODEF_F_LINEARIZE_AT];
    const size_t need = field_count(c, ODEF_F_LINEARIZE_AT, (long)n_t) * sizeof(double);
    if (b.bound) {
      if (b.bytes < need)
        return fail(c, "odef_solve_fixed: the bound ODEF_F_LINEARIZE_AT buffer holds %zu bytes, the grid needs n_t * d * N * 8 = %zu",
                    b.bytes, need);
      b.valid = need;
    } else if (c->lin_grid.size() != (size_t)n_t || std::memcmp(c->lin_grid.data(), tgrid, sizeof(double) * (size_t)n_t) != 0) {
      return fail(c, "odef_solve_fixed: ODEF_F_LINEARIZE_AT holds the smoothed solution on another grid (%zu points, this one has %lld); "
                     "evaluate that solution on the new grid (odef_dense_output) and bind the result (odef_bind_device)",
                  c->lin_grid.size(), (long long)n_t);
    }
    lin = (const double*)b.ptr;
  }
  if (set_device(c)) return -1;
  const long nsteps = (long)n_t - 1;
  c->adaptive = false;
  c->n_save = (c->cfg.save_mode == ODEF_SAVE_EVERYSTEP) ? nsteps + 1 : 1;
  // a repeated solve on the grid that is already on the device (ensemble sweeps, the benchmark loop) skips the table
  // construction, the four uploads and their synchronisation
  const bool same_grid = c->grid_on_device && c->tgrid.size() == (size_t)n_t &&
                         std::memcmp(c->tgrid.data(), tgrid, sizeof(double) * (size_t)n_t) == 0;
  if (!same_grid) {
    c->grid_on_device = false;
    c->tgrid.assign(tgrid, tgrid + n_t);
    // step sizes, and one preconditioner table per distinct h (src/preconditioning.jl:1-17; pval by libm pow
    // as the reference's h^(-q-1/2))
    std::vector<double> hs(nsteps), tabs;
    std::vector<int> idx(nsteps);
    std::vector<double> distinct;
    for (long n = 0; n < nsteps; ++n) {
      hs[n] = tgrid[n + 1] - tgrid[n];
      int k = -1;
      for (size_t j = distinct.size(); j-- > 0;)
        if (distinct[j] == hs[n]) { k = (int)j; break; }
      if (k < 0) {
        k = (int)distinct.size();
        distinct.push_back(hs[n]);
        tabs.resize(distinct.size() * kTabStride, 0.0);
        double* t = tabs.data() + (size_t)k * kTabStride;
        const double pval = std::pow(hs[n], -c->q - 0.5);
        switch (c->q) {
          case 1: precond_fill<2>(hs[n], pval, t); break;
          case 2: precond_fill<3>(hs[n], pval, t); break;
          case 3: precond_fill<4>(hs[n], pval, t); break;
          case 4: precond_fill<5>(hs[n], pval, t); break;
          default: precond_fill<6>(hs[n], pval, t); break;
        }
      }
      idx[n] = k;
    }
    if (c->grid_cap < (size_t)n_t) {
      if (c->d_hs) { HIPCHK(c, hipFree(c->d_hs)); HIPCHK(c, hipFree(c->d_ptab)); HIPCHK(c, hipFree(c->d_tab_idx)); HIPCHK(c, hipFree(c->d_tgrid)); }
      c->d_hs = c->d_ptab = c->d_tgrid = nullptr;
      c->d_tab_idx = nullptr;
      c->grid_cap = 0;
      HIPCHK(c, hipMalloc((void**)&c->d_hs, sizeof(double) * n_t));
      HIPCHK(c, hipMalloc((void**)&c->d_ptab, sizeof(double) * n_t * kTabStride));  // worst case: all h distinct
      HIPCHK(c, hipMalloc((void**)&c->d_tab_idx, sizeof(int) * n_t));
      HIPCHK(c, hipMalloc((void**)&c->d_tgrid, sizeof(double) * n_t));
      c->grid_cap = (size_t)n_t;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_hs, hs.data(), sizeof(double) * nsteps, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_ptab, tabs.data(), sizeof(double) * tabs.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_tab_idx, idx.data(), sizeof(int) * nsteps, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_tgrid, tgrid, sizeof(double) * n_t, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors are locals
    c->grid_on_device = true;
  }
  if (alloc_outputs(c, c->n_save)) return -1;
  FilterParams P;
  fill_params(c, P);
  P.hs = c->d_hs;
  P.ptab = c->d_ptab;
  P.tab_idx = c->d_tab_idx;
  P.nsteps = nsteps;
  P.t0 = c->t0;
  P.lin = lin;
  P.tgrid = c->d_tgrid;
  size_t have = 0;
  if (team_path(c)) {
    if (P.everystep) {  // the matrix-core kernel writes its records through the trajectory-major stage when all of them fit
      const size_t tri = (size_t)c->D * (c->D + 1) / 2, per_rec = (size_t)P.N * ((tri + 15) / 16 * 16);
      have = ensure_stage(c, nsteps + 1, per_rec);
      if (have < (size_t)(nsteps + 1) * per_rec) have = 0;
    }
  } else if ((size_t)c->TRI * (size_t)c->cfg.n_traj * sizeof(double) >= (1ull << 31)) {
    // one lane per trajectory: the per-field buffer descriptors carry 32-bit sizes
    return fail(c, "odef_solve_fixed: n_traj * D(D+1)/2 * 8 bytes must stay below 2 GiB per save slot; shard the ensemble");
  }
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  const int rc = c->field->filter(c->q, is_ek1(c->cfg.alg), P, c->stream, 0, have ? c->d_stage : nullptr, have, &c->stage_filter_recs);
  if (rc) return fail(c, "odef_solve_fixed: no %skernel for rhs %d order %d", lin ? "IEKS " : "", c->cfg.rhs_id, c->q);
  std::snprintf(c->kname[kPassFilter], sizeof c->kname[kPassFilter], "%s", last_kernel());
  return finish_filter(c, 1);
}

int odef_solve_adaptive(odef_ctx* c, double t1, double abstol, double reltol, double dt0, const odef_controller* ctrl,
                        int64_t max_steps) {
  if (!c) return -1;
  if (!c->have_problem) return fail(c, "odef_solve_adaptive: call odef_set_problem first");
  if (!(t1 > c->t0)) return fail(c, "odef_solve_adaptive: t1 must exceed t0");
  if (!(dt0 > 0.0)) return fail(c, "odef_solve_adaptive: dt0 must be positive");
  if (max_steps < 1) return fail(c, "odef_solve_adaptive: max_steps must be >= 1");
  if (c->cfg.save_mode != ODEF_SAVE_EVERYSTEP) return fail(c, "odef_solve_adaptive: needs ODEF_SAVE_EVERYSTEP");
  if (c->cfg.alg == ODEF_IEKS && lin_active(c))
    return fail(c, "odef_solve_adaptive: IEKS relinearisation runs on fixed grids (ODEF_F_LINEARIZE_AT is set; "
                   "odef_bind_device(ctx, ODEF_F_LINEARIZE_AT, NULL, 0) empties it, the step is then EK1)");
  if ((size_t)c->TRI * (size_t)c->cfg.n_traj * sizeof(double) >= (1ull << 31))
    return fail(c, "odef_solve_adaptive: n_traj * D(D+1)/2 * 8 bytes must stay below 2 GiB per save slot; shard the ensemble");
  if (set_device(c)) return -1;
  c->adaptive = true;
  c->n_save = (long)max_steps + 1;
  c->tgrid.clear();
  if (alloc_outputs(c, c->n_save)) return -1;
  FilterParams P;
  fill_params(c, P);
  P.t0 = c->t0;
  P.t1 = t1;
  P.abstol = abstol;
  P.reltol = reltol;
  P.dt0 = dt0;
  P.max_save = c->n_save;
  if (ctrl) {
    std::memcpy(&P.ctrl, ctrl, sizeof(Controller));
  } else {  // OrdinaryDiffEq defaults with src/alg_utils.jl:23-24 exponents
    P.ctrl = Controller{7.0 / (10.0 * (c->q + 1)), 2.0 / (5.0 * (c->q + 1)), 0.9, 0.2, 10.0, 1.0, 1.0, 1e-4, 0.0, 1e300};
  }
  HIPCHK(c, hipMemsetAsync(c->f[ODEF_F_T].ptr, 0, c->f[ODEF_F_T].valid, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  const int rc = c->field->filter(c->q, is_ek1(c->cfg.alg), P, c->stream, 1, nullptr, 0, &c->stage_filter_recs);
  if (rc) return fail(c, "odef_solve_adaptive: no kernel for rhs %d order %d", c->cfg.rhs_id, c->q);
  std::snprintf(c->kname[kPassFilter], sizeof c->kname[kPassFilter], "%s", last_kernel());
  return finish_filter(c, 1);
}

int odef_smooth(odef_ctx* c) {
  if (!c) return -1;
  if (!c->solved) return fail(c, "odef_smooth: nothing to smooth, call odef_solve_* first");
  if (c->cfg.save_mode != ODEF_SAVE_EVERYSTEP) return fail(c, "odef_smooth: needs ODEF_SAVE_EVERYSTEP (cfg.smooth = 1)");
  if (set_device(c)) return -1;
  if (ensure(c, ODEF_F_SMOOTH_MEAN, field_count(c, ODEF_F_SMOOTH_MEAN, c->n_save) * sizeof(double))) return -1;
  if (ensure(c, ODEF_F_SMOOTH_COV_TRIL, field_count(c, ODEF_F_SMOOTH_COV_TRIL, c->n_save) * sizeof(double))) return -1;
  SmoothParams S;
  std::memset(&S, 0, sizeof S);
  S.pc = c->pc;
  S.N = c->cfg.n_traj;
  S.n_save = c->n_save;
  S.adaptive = c->adaptive;
  S.hs = c->d_hs;
  S.ptab = c->d_ptab;
  S.tab_idx = c->d_tab_idx;
  S.tsave = (const double*)c->f[ODEF_F_T].ptr;
  S.nsaved = (const int*)c->f[ODEF_F_NSAVED].ptr;
  S.mean = (const double*)c->f[ODEF_F_MEAN].ptr;
  S.cov = (const double*)c->f[ODEF_F_COV_TRIL].ptr;
  S.diff = (const double*)c->f[ODEF_F_DIFFUSION].ptr;
  S.smean = (double*)c->f[ODEF_F_SMOOTH_MEAN].ptr;
  S.scov = (double*)c->f[ODEF_F_SMOOTH_COV_TRIL].ptr;
  S.retcode = (int*)c->f[ODEF_F_RETCODE].ptr;
  S.mv = is_mv(c->cfg.diffusion);
  if (c->adaptive) {  // unused save slots stay defined
    HIPCHK(c, hipMemsetAsync(S.smean, 0, c->f[ODEF_F_SMOOTH_MEAN].valid, c->stream));
    HIPCHK(c, hipMemsetAsync(S.scov, 0, c->f[ODEF_F_SMOOTH_COV_TRIL].valid, c->stream));
  }
  if (c->field->smooth_ws && ensure_ws(c, (size_t)c->cfg.n_traj * c->field->smooth_ws(c->q))) return -1;
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  int rc = -4;
  if (c->field->smooth_staged) {  // the covariance records go through the trajectory-major stage, in blocks (record_stage.h)
    long n_rec = S.n_save;
    if (S.adaptive) {  // save slots in use: the largest record count of the ensemble
      std::vector<int> ns((size_t)S.N);
      HIPCHK(c, hipMemcpyAsync(ns.data(), S.nsaved, ns.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      n_rec = 1;
      for (int v : ns) n_rec = v > n_rec ? v : n_rec;
      if (n_rec > S.n_save) n_rec = S.n_save;
    }
    const size_t tri = (size_t)c->D * (c->D + 1) / 2;
    const size_t per_rec = (size_t)S.N * ((tri + 15) / 16 * 16);
    // the filter's records may still be in the stage (fixed grid, every step saved, all of them fit): record r at r * per_rec
    const bool resident = !S.adaptive && n_rec >= 3 && c->stage_filter_recs == n_rec && c->stage_cap >= (size_t)n_rec * per_rec;
    const size_t have = n_rec < 3 ? 0 : resident ? (size_t)(n_rec - 1) * per_rec : ensure_stage(c, n_rec - 1, per_rec);
    if (have) rc = c->field->smooth_staged(c->q, S, n_rec, c->d_ws, c->d_stage, have, c->stream, resident ? n_rec : 0);
  }
  if (rc == -4) rc = c->field->smooth(c->q, S, c->d_ws, c->stream);
  records_changed(c, kSmoothRecs);  // (whatever the launch did: the stage no longer holds the filter records either)
  if (rc) return fail(c, "odef_smooth: no kernel for d %d order %d", c->d, c->q);
  std::snprintf(c->kname[kPassSmooth], sizeof c->kname[kPassSmooth], "%s", last_kernel());
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, hipGetLastError());
  if (c->cfg.alg == ODEF_IEKS && !c->adaptive) {
    // alg.linearize_at = sol (src/ieks.jl:58): the u rows of every smoothed mean into an owned ODEF_F_LINEARIZE_AT, one strided
    // copy; the next odef_solve_fixed on this grid linearises there.  Caller memory is never written: a bound buffer is let go.
    Buf& b = c->f[ODEF_F_LINEARIZE_AT];
    if (b.bound) b = Buf{};
    if (ensure(c, ODEF_F_LINEARIZE_AT, field_count(c, ODEF_F_LINEARIZE_AT, c->n_save) * sizeof(double))) return -1;
    const size_t N = (size_t)c->cfg.n_traj, row = (size_t)c->d * N * sizeof(double);
    HIPCHK(c, hipMemcpy2DAsync(b.ptr, row, c->f[ODEF_F_SMOOTH_MEAN].ptr, (size_t)c->D * N * sizeof(double), row, (size_t)c->n_save,
                               hipMemcpyDeviceToDevice, c->stream));
    c->lin_set = true;
    c->lin_grid = c->tgrid;
  }
  c->nl[kPassSmooth] = 1;
  c->smoothed_done = true;
  c->pending = 2;
  return c->defer ? 0 : complete_pending(c);
}

int odef_dense_output(odef_ctx* c, const double* tq, int64_t n_q, int smoothed) {
  if (!c || !tq) return fail(c, "odef_dense_output: null argument");
  if (!c->solved) return fail(c, "odef_dense_output: call odef_solve_* first");
  if (c->cfg.save_mode != ODEF_SAVE_EVERYSTEP) return fail(c, "odef_dense_output: needs ODEF_SAVE_EVERYSTEP");
  if (smoothed && !c->smoothed_done) return fail(c, "odef_dense_output: smoothed posterior requested but odef_smooth has not run");
  if (n_q < 1 || n_q > 65535) return fail(c, "odef_dense_output: n_q must be in 1..65535");
  if (!team_path(c) && c->D > 32) return fail(c, "odef_dense_output: built for state dimension <= 32 and for the workgroup-per-trajectory path (got %d)", c->D);
  if (set_device(c)) return -1;
  if (c->tq_cap < (size_t)n_q) {
    if (c->d_tq) HIPCHK(c, hipFree(c->d_tq));
    c->d_tq = nullptr;
    HIPCHK(c, hipMalloc((void**)&c->d_tq, sizeof(double) * n_q));
    c->tq_cap = (size_t)n_q;
  }
  HIPCHK(c, hipMemcpyAsync(c->d_tq, tq, sizeof(double) * n_q, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->n_q = (long)n_q;
  records_changed(c, kDenseRecs);
  const size_t N = (size_t)c->cfg.n_traj;
  if (ensure(c, ODEF_F_DENSE_MEAN, (size_t)n_q * c->D * N * sizeof(double))) return -1;
  if (ensure(c, ODEF_F_DENSE_COV_TRIL, (size_t)n_q * c->TRI * N * sizeof(double))) return -1;
  DenseParams P;
  std::memset(&P, 0, sizeof P);
  P.pc = c->pc;
  P.N = c->cfg.n_traj;
  P.n_save = c->n_save;
  P.adaptive = c->adaptive;
  P.smoothed = smoothed != 0;
  P.tgrid = c->d_tgrid;
  P.tsave = (const double*)c->f[ODEF_F_T].ptr;
  P.nsaved = (const int*)c->f[ODEF_F_NSAVED].ptr;
  P.mean = (const double*)c->f[ODEF_F_MEAN].ptr;
  P.cov = (const double*)c->f[ODEF_F_COV_TRIL].ptr;
  P.diff = (const double*)c->f[ODEF_F_DIFFUSION].ptr;
  P.smean = (const double*)c->f[ODEF_F_SMOOTH_MEAN].ptr;
  P.scov = (const double*)c->f[ODEF_F_SMOOTH_COV_TRIL].ptr;
  P.tq = c->d_tq;
  P.n_q = (long)n_q;
  P.qmean = (double*)c->f[ODEF_F_DENSE_MEAN].ptr;
  P.qcov = (double*)c->f[ODEF_F_DENSE_COV_TRIL].ptr;
  P.mv = is_mv(c->cfg.diffusion);
  if (c->field->smooth_ws && ensure_ws(c, (size_t)dense_d28_grid(P.N * P.n_q) * c->field->smooth_ws(c->q))) return -1;
  if (c->field->dense(c->q, P, c->d_ws, c->stream)) return fail(c, "odef_dense_output: no kernel for d %d order %d", c->d, c->q);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// posterior sampling (odef_sample: over the save slots; odef_dense_sample: over the filter posterior at the query times)
static SampleParams sample_params(const odef_ctx* c, long n_rec, int mean_field, int cov_field, int64_t n_samples, uint64_t seed, double noise_scale) {
  SampleParams S;
  std::memset(&S, 0, sizeof S);
  S.pc = c->pc;
  S.N = c->cfg.n_traj;
  S.n_save = n_rec;
  S.adaptive = c->adaptive;
  S.tsave = (const double*)c->f[ODEF_F_T].ptr;
  S.nsaved = (const int*)c->f[ODEF_F_NSAVED].ptr;
  S.mean = (const double*)c->f[mean_field].ptr;
  S.cov = (const double*)c->f[cov_field].ptr;
  S.diff = (const double*)c->f[ODEF_F_DIFFUSION].ptr;
  S.n_samples = (long)n_samples;
  S.seed = (unsigned long long)seed;
  S.noise_scale = noise_scale;
  S.samples = (double*)c->f[ODEF_F_SAMPLES].ptr;
  S.mv = is_mv(c->cfg.diffusion);
  return S;
}

static int run_sampler(odef_ctx* c, const SampleParams& S, const char* who) {
  if (c->field->smooth_ws && ensure_ws(c, (size_t)dense_d28_grid(S.N * S.n_samples) * c->field->smooth_ws(c->q))) return -1;
  if (c->field->sample(c->q, S, c->d_ws, c->stream)) return fail(c, "%s: no kernel for d %d order %d", who, c->d, c->q);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int odef_sample(odef_ctx* c, int64_t n_samples, uint64_t seed, double noise_scale) {
  if (!c) return -1;
  if (!c->solved) return fail(c, "odef_sample: call odef_solve_* first");
  if (c->cfg.save_mode != ODEF_SAVE_EVERYSTEP) return fail(c, "odef_sample: needs ODEF_SAVE_EVERYSTEP (sampling not implemented for non-smoothed posteriors)");
  if (n_samples < 1 || n_samples > 65535) return fail(c, "odef_sample: n_samples must be in 1..65535");
  if (!team_path(c) && c->D > 32) return fail(c, "odef_sample: built for state dimension <= 32 and for the workgroup-per-trajectory path (got %d)", c->D);
  if (set_device(c)) return -1;
  c->n_samples = (long)n_samples;
  if (ensure(c, ODEF_F_SAMPLES, field_count(c, ODEF_F_SAMPLES, c->n_save) * sizeof(double))) return -1;
  SampleParams S = sample_params(c, c->n_save, ODEF_F_MEAN, ODEF_F_COV_TRIL, n_samples, seed, noise_scale);
  S.hs = c->d_hs;
  S.ptab = c->d_ptab;
  S.tab_idx = c->d_tab_idx;
  if (c->adaptive) HIPCHK(c, hipMemsetAsync(S.samples, 0, c->f[ODEF_F_SAMPLES].valid, c->stream));  // unused slots stay defined
  return run_sampler(c, S, "odef_sample");
}

int odef_dense_sample(odef_ctx* c, const double* tq, int64_t n_q, int64_t n_samples, uint64_t seed, double noise_scale) {
  if (!c || !tq) return fail(c, "odef_dense_sample: null argument");
  if (n_samples < 1 || n_samples > 65535) return fail(c, "odef_dense_sample: n_samples must be in 1..65535");
  for (int64_t k = 1; k < n_q; ++k)
    if (!(tq[k] >= tq[k - 1])) return fail(c, "odef_dense_sample: times must be non-decreasing");
  if (odef_dense_output(c, tq, n_q, 0)) return -1;  // filter posterior at tq (src/solution_sampling.jl:66)
  c->n_samples = (long)n_samples;
  if (ensure(c, ODEF_F_SAMPLES, field_count(c, ODEF_F_SAMPLES, (long)n_q) * sizeof(double))) return -1;
  SampleParams S = sample_params(c, (long)n_q, ODEF_F_DENSE_MEAN, ODEF_F_DENSE_COV_TRIL, n_samples, seed, noise_scale);
  S.tq = c->d_tq;
  S.rec_t = c->d_tgrid;
  S.n_rec = c->n_save;
  return run_sampler(c, S, "odef_dense_sample");
}

int64_t odef_n_save(const odef_ctx* c) { return c ? c->n_save : -1; }

int odef_field_bytes(const odef_ctx* c, int field, size_t* bytes) {
  if (!c || !bytes) return -1;
  if (const DerivedFamily* fam = derived_family(field)) {
    if (fam->bytes_after_fetch) {  // (the context is the caller's own object; the pass fills its cache)
      void* unused = nullptr;
      return derived_fetch(const_cast<odef_ctx*>(c), fam, field, "odef_field_bytes", &unused, bytes);
    }
    if (fam->check(c, field, "odef_field_bytes")) return -1;
    *bytes = fam->bytes(c, field);
    return 0;
  }
  if (field < 0 || field >= ODEF_F_COUNT_) return -1;
  if (field == ODEF_F_T && !c->adaptive) { *bytes = c->tgrid.size() ? (size_t)c->n_save * sizeof(double) : 0; return 0; }
  *bytes = c->f[field].valid;
  return 0;
}

int odef_get(odef_ctx* c, int field, void* host_dst, size_t bytes) {
  if (!c || !host_dst) return fail(c, "odef_get: null argument");
  void* src = nullptr;
  size_t have = 0;
  if (const DerivedFamily* fam = derived_family(field)) {
    if (derived_fetch(c, fam, field, "odef_get", &src, &have)) return -1;
  } else {
    if (field < 0 || field >= ODEF_F_COUNT_) return fail(c, "odef_get: unknown field %d", field);
    if (set_device(c)) return -1;
    if (field == ODEF_F_T && !c->adaptive) {  // the shared grid lives on the host
      if (c->tgrid.empty()) return fail(c, "odef_get: no solve yet");
      const size_t need = (size_t)c->n_save * sizeof(double);
      if (bytes != need) return fail(c, "odef_get: field T holds %zu bytes, caller asked for %zu", need, bytes);
      if (c->n_save == 1) ((double*)host_dst)[0] = c->tgrid.back();
      else std::memcpy(host_dst, c->tgrid.data(), need);
      return 0;
    }
    const Buf& b = c->f[field];
    if (!b.ptr || !b.valid) return fail(c, "odef_get: field %d holds no data yet", field);
    src = b.ptr;
    have = b.valid;
  }
  if (bytes != have) return fail(c, "odef_get: field %d holds %zu bytes, caller asked for %zu", field, have, bytes);
  HIPCHK(c, hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int odef_get_device(odef_ctx* c, int field, void** dev_ptr, size_t* bytes) {
  if (!c || !dev_ptr || !bytes) return fail(c, "odef_get_device: null argument");
  if (const DerivedFamily* fam = derived_family(field)) return derived_fetch(c, fam, field, "odef_get_device", dev_ptr, bytes);
  if (field < 0 || field >= ODEF_F_COUNT_) return fail(c, "odef_get_device: unknown field %d", field);
  records_changed(c, record_set_of(field));  // the pointer handed out is writable
  const Buf& b = c->f[field];
  if (!b.ptr || !b.valid) return fail(c, "odef_get_device: field %d holds no data yet", field);
  *dev_ptr = b.ptr;
  *bytes = b.valid;
  return 0;
}

int odef_bind_device(odef_ctx* c, int field, void* dev_ptr, size_t bytes) {
  if (!c) return -1;
  if (field == ODEF_E_REFERENCE) {  // the truth of the solution errors: caller memory, read only; NULL lets it go
    c->err_ref = (const double*)dev_ptr;
    c->err_ref_bytes = dev_ptr ? bytes : 0;
    records_changed(c, kTruth);
    return 0;
  }
  if (is_datalik_input(field)) {  // the observations of the data log-likelihood: caller memory, read only; NULL lets it go
    Buf& b = c->obs[field - ODEF_L_OBS_SAVE];
    b = Buf{};
    if (dev_ptr) {
      b.ptr = dev_ptr;
      b.bytes = bytes;
      b.bound = true;
    }
    records_changed(c, kObservations);
    return 0;
  }
  if (is_event_input(field)) {  // the spec and the level of the event location: caller memory, read only; NULL lets it go
    Buf& b = c->evin[field - ODEF_EV_SPEC];
    b = Buf{};
    if (dev_ptr) {
      b.ptr = dev_ptr;
      b.bytes = bytes;
      b.bound = true;
    }
    records_changed(c, kEventSpec);
    return 0;
  }
  if (field == ODEF_Q_PROBS) {  // the probabilities of the ensemble quantiles: caller memory, read only; NULL lets it go
    c->qprobs = Buf{};
    if (dev_ptr) {
      c->qprobs.ptr = dev_ptr;
      c->qprobs.bytes = bytes;
      c->qprobs.bound = true;
    }
    records_changed(c, kQuantileProbs);
    return 0;
  }
  if (field == ODEF_W_LOGWEIGHT) {  // the log-weights of the weighted summary: caller memory, read only; NULL lets it go
    if (dev_ptr && bytes != sizeof(double) * (size_t)c->cfg.n_traj)
      return fail(c, "odef_bind_device: ODEF_W_LOGWEIGHT is double [N]: %zu bytes for N = %ld, got %zu",
                  sizeof(double) * (size_t)c->cfg.n_traj, (long)c->cfg.n_traj, bytes);
    c->wlogw = Buf{};
    if (dev_ptr) {
      c->wlogw.ptr = dev_ptr;
      c->wlogw.bytes = bytes;
      c->wlogw.bound = true;
    }
    records_changed(c, kLogWeights);
    return 0;
  }
  if (field < 0 || field >= ODEF_F_COUNT_ || field == ODEF_F_U0) return fail(c, "odef_bind_device: field %d cannot be bound", field);
  records_changed(c, record_set_of(field));
  if (field == ODEF_F_LINEARIZE_AT && dev_ptr && c->cfg.alg != ODEF_IEKS)
    return fail(c, "odef_bind_device: ODEF_F_LINEARIZE_AT belongs to an IEKS context (alg = ODEF_IEKS)");
  if (set_device(c)) return -1;
  Buf& b = c->f[field];
  if (b.owned && b.ptr) HIPCHK(c, hipFree(b.ptr));
  b = Buf{};
  if (field == ODEF_F_LINEARIZE_AT) {  // bound (caller memory, read only) or, with NULL, empty
    c->lin_set = false;
    c->lin_grid.clear();
  }
  if (dev_ptr) {
    b.ptr = dev_ptr;
    b.bytes = bytes;
    b.bound = true;
  }
  return 0;
}

int odef_synchronize(odef_ctx* c) {
  if (!c) return -1;
  if (set_device(c)) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int odef_kernel_name(odef_ctx* c, int which, char* buf, size_t n) {
  if (!c || which < 0 || which >= kPassCount || !buf || n == 0) return -1;
  std::snprintf(buf, n, "%s", c->kname[which]);
  return 0;
}

int odef_kernel_time_ms(odef_ctx* c, int which, float* ms, int* n_launches) {
  if (!c || which < 0 || which >= kPassCount || !ms) return -1;
  *ms = c->ms[which];
  if (n_launches) *n_launches = c->nl[which];
  return 0;
}

int odef_ibm(int d, int q, double* A, double* Q_L) {
  if (d < 1 || q < 1 || q > ODEF_MAX_ORDER || !A || !Q_L) return -1;
  PriorConsts pc;
  build_prior(q, pc);
  const int D = d * (q + 1);
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      const bool same = (i % d) == (j % d);
      A[i * D + j] = same ? pc.At[i / d][j / d] : 0.0;
      Q_L[i * D + j] = same ? pc.QLt[i / d][j / d] : 0.0;
    }
  return 0;
}

int odef_preconditioner(int d, int q, double h, double* P_diag) {
  if (d < 1 || q < 0 || !P_diag || !(h > 0.0)) return -1;
  double val = std::pow(h, -q - 0.5);  // src/preconditioning.jl:9
  for (int j = 0; j <= q; ++j) {
    for (int i = 0; i < d; ++i) P_diag[j * d + i] = val;
    val *= h;
  }
  return 0;
}


/* ---- ensemble sharded over the GPUs of one node (single process) ------------------------------------------------- */

int odef_shard_range(int64_t n_traj, int32_t n_shards, int32_t shard, int64_t* first, int64_t* count) {
  if (n_traj < 0 || n_shards < 1 || shard < 0 || shard >= n_shards || !first || !count) return -1;
  // contiguous blocks, the first n_traj % n_shards shards one trajectory longer
  const int64_t base = n_traj / n_shards, rem = n_traj % n_shards;
  *first = shard * base + (shard < rem ? shard : rem);
  *count = base + (shard < rem ? 1 : 0);
  return 0;
}

}  // extern "C"

namespace {

// librccl is bound at run time (dlopen): the library also has to load where RCCL is not installed, and a group of ONE
// device needs no collective library at all.
struct Rccl {
  void* h = nullptr;
  int (*CommInitAll)(void**, int, const int*) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool load(std::string& err) {
    if (h) return true;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* n : names)
      if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) { err = std::string("librccl.so not loadable: ") + dlerror(); return false; }
    CommInitAll = (decltype(CommInitAll))dlsym(h, "ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
    GroupStart = (decltype(GroupStart))dlsym(h, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(h, "ncclGroupEnd");
    AllGather = (decltype(AllGather))dlsym(h, "ncclAllGather");
    GetErrorString = (decltype(GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !AllGather || !GetErrorString) {
      err = "librccl.so lacks an expected symbol";
      dlclose(h);
      h = nullptr;
      return false;
    }
    return true;
  }
};
Rccl g_rccl;
constexpr int kNcclDouble = 8;  // ncclFloat64 (rccl.h)

// final posterior mean of every trajectory of a shard, [D][cnt_max] (padding columns zero): the last record of a fixed
// grid, record NSAVED-1 of an adaptive solve
__global__ void pack_final_kernel(const double* __restrict__ mean, const int* __restrict__ nsaved, long n_save_fixed,
                                  int D, long N, long cnt_max, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt_max) return;
  const long slot = i < N ? (nsaved ? (long)nsaved[i] - 1 : n_save_fixed - 1) : 0;
  for (int k = 0; k < D; ++k) out[(size_t)k * cnt_max + i] = i < N ? mean[((size_t)slot * D + k) * N + i] : 0.0;
}

}  // namespace

struct odef_group {
  std::vector<odef_ctx*> ctx;
  std::vector<int64_t> first, count;
  int64_t n_total = 0, cnt_max = 0;
  int D = 0;
  std::vector<void*> comm;         // ncclComm_t per device (empty until the first all-gather of a multi-device group)
  std::vector<double*> send, recv; // per device: [D][cnt_max] and [G][D][cnt_max]
  bool gathered = false;
  std::string err;
};

namespace {
int gfail(odef_group* g, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (g) g->err = buf;
  else g_create_error = buf;
  return -1;
}
template <class F>
int for_all_then_complete(odef_group* g, const char* what, F&& launch) {
  for (odef_ctx* c : g->ctx) c->defer = true;
  int rc = 0;
  size_t launched = 0;
  for (; launched < g->ctx.size() && rc == 0; ++launched) {
    rc = launch(g->ctx[launched], (int)launched);
    if (rc) gfail(g, "%s, shard %zu: %s", what, launched, g->ctx[launched]->err.c_str());
  }
  for (size_t k = 0; k < g->ctx.size(); ++k) {
    odef_ctx* c = g->ctx[k];
    c->defer = false;
    if (c->pending && set_device(c) == 0 && complete_pending(c) != 0 && rc == 0)
      rc = gfail(g, "%s, shard %zu: %s", what, k, c->err.c_str());
  }
  g->gathered = false;
  return rc;
}
}  // namespace

extern "C" {

const char* odef_group_last_error(const odef_group* g) { return g ? g->err.c_str() : g_create_error.c_str(); }

int odef_group_layout(int64_t n_traj, int32_t n_devices, int32_t state_dim, int64_t* first, int64_t* count, int64_t* cnt_max,
                      int64_t* block_doubles) {
  if (n_devices < 1 || n_traj < n_devices || state_dim < 1) return -1;
  int64_t longest = 0;
  for (int32_t k = 0; k < n_devices; ++k) {
    int64_t f = 0, c = 0;
    if (odef_shard_range(n_traj, n_devices, k, &f, &c) != 0) return -1;
    if (first) first[k] = f;
    if (count) count[k] = c;
    longest = c > longest ? c : longest;
  }
  if (cnt_max) *cnt_max = longest;
  if (block_doubles) *block_doubles = (int64_t)state_dim * longest;
  return 0;
}

int odef_unpad_gathered(const double* gathered, int32_t n_devices, int32_t state_dim, int64_t n_traj, double* dst) {
  if (!gathered || !dst) return -1;
  int64_t cnt_max = 0, blk = 0;
  if (odef_group_layout(n_traj, n_devices, state_dim, nullptr, nullptr, &cnt_max, &blk) != 0) return -1;
  for (int32_t k = 0; k < n_devices; ++k) {  // drop the padding columns of the shorter shards
    int64_t f = 0, c = 0;
    odef_shard_range(n_traj, n_devices, k, &f, &c);
    for (int32_t r = 0; r < state_dim; ++r)
      std::memcpy(dst + (size_t)r * (size_t)n_traj + (size_t)f, gathered + (size_t)k * (size_t)blk + (size_t)r * (size_t)cnt_max,
                  (size_t)c * sizeof(double));
  }
  return 0;
}

int odef_group_create(odef_group** out, const odef_config* cfg, int32_t n_devices, const int32_t* device_ids) {
  if (!out || !cfg) return gfail(nullptr, "odef_group_create: null argument");
  *out = nullptr;
  if (n_devices < 1) return gfail(nullptr, "odef_group_create: n_devices must be >= 1");
  if (cfg->n_traj < n_devices) return gfail(nullptr, "odef_group_create: fewer trajectories (%lld) than devices (%d)", (long long)cfg->n_traj, n_devices);
  odef_group* g = new odef_group();
  g->n_total = cfg->n_traj;
  for (int k = 0; k < n_devices; ++k) {
    int64_t first = 0, count = 0;
    odef_shard_range(cfg->n_traj, n_devices, k, &first, &count);
    odef_config sc = *cfg;
    sc.n_traj = count;
    sc.device = device_ids ? device_ids[k] : k;
    odef_ctx* c = nullptr;
    if (odef_create(&c, &sc) != 0) {
      gfail(nullptr, "odef_group_create: shard %d on device %d: %s", k, sc.device, g_create_error.c_str());
      odef_group_destroy(g);
      return -1;
    }
    g->ctx.push_back(c);
    g->first.push_back(first);
    g->count.push_back(count);
    if (count > g->cnt_max) g->cnt_max = count;
    g->D = c->D;
  }
  *out = g;
  return 0;
}

void odef_group_destroy(odef_group* g) {
  if (!g) return;
  for (size_t k = 0; k < g->ctx.size(); ++k) {
    (void)hipSetDevice(g->ctx[k]->device);
    if (k < g->comm.size() && g->comm[k] && g_rccl.CommDestroy) g_rccl.CommDestroy(g->comm[k]);
    if (k < g->send.size() && g->send[k]) (void)hipFree(g->send[k]);
    if (k < g->recv.size() && g->recv[k]) (void)hipFree(g->recv[k]);
    odef_destroy(g->ctx[k]);
  }
  delete g;
}

int32_t odef_group_size(const odef_group* g) { return g ? (int32_t)g->ctx.size() : -1; }
odef_ctx* odef_group_ctx(odef_group* g, int32_t shard) {
  return (g && shard >= 0 && shard < (int32_t)g->ctx.size()) ? g->ctx[shard] : nullptr;
}
int odef_group_shard(const odef_group* g, int32_t shard, int64_t* first, int64_t* count) {
  if (!g || shard < 0 || shard >= (int32_t)g->ctx.size() || !first || !count) return -1;
  *first = g->first[shard];
  *count = g->count[shard];
  return 0;
}

int odef_group_set_problem(odef_group* g, const double* u0, const double* p, double t0) {
  if (!g || !u0) return gfail(g, "odef_group_set_problem: null argument");
  for (size_t k = 0; k < g->ctx.size(); ++k) {
    odef_ctx* c = g->ctx[k];
    const double* pk = (p && !c->cfg.params_shared) ? p + (size_t)g->first[k] * c->np : p;
    if (odef_set_problem(c, u0 + (size_t)g->first[k] * c->d, pk, t0) != 0)
      return gfail(g, "odef_group_set_problem, shard %zu: %s", k, c->err.c_str());
  }
  return 0;
}

int odef_group_set_problem_perturbed(odef_group* g, const double* base_u0, const double* p, double t0, double scale,
                                     uint64_t seed, int32_t n_perturbed) {
  if (!g) return -1;
  for (size_t k = 0; k < g->ctx.size(); ++k)  // global numbering: the ensemble does not depend on the number of shards
    if (odef_set_problem_perturbed(g->ctx[k], base_u0, p, t0, scale, seed, g->first[k], n_perturbed) != 0)
      return gfail(g, "odef_group_set_problem_perturbed, shard %zu: %s", k, g->ctx[k]->err.c_str());
  return 0;
}

int odef_group_solve_fixed(odef_group* g, const double* tgrid, int64_t n_t) {
  if (!g) return -1;
  return for_all_then_complete(g, "odef_group_solve_fixed", [&](odef_ctx* c, int) { return odef_solve_fixed(c, tgrid, n_t); });
}
int odef_group_solve_adaptive(odef_group* g, double t1, double abstol, double reltol, double dt0, const odef_controller* ctrl,
                              int64_t max_steps) {
  if (!g) return -1;
  return for_all_then_complete(g, "odef_group_solve_adaptive",
                               [&](odef_ctx* c, int) { return odef_solve_adaptive(c, t1, abstol, reltol, dt0, ctrl, max_steps); });
}
int odef_group_smooth(odef_group* g) {
  if (!g) return -1;
  return for_all_then_complete(g, "odef_group_smooth", [&](odef_ctx* c, int) { return odef_smooth(c); });
}

int odef_allgather(odef_group* g, int smoothed) {
  if (!g) return -1;
  const int G = (int)g->ctx.size();
  const size_t blk = (size_t)g->D * (size_t)g->cnt_max;  // doubles per shard block
  if (g->send.empty()) {
    g->send.assign(G, nullptr);
    g->recv.assign(G, nullptr);
    for (int k = 0; k < G; ++k) {
      odef_ctx* c = g->ctx[k];
      if (set_device(c)) return gfail(g, "odef_allgather: %s", c->err.c_str());
      if (hipMalloc((void**)&g->send[k], blk * sizeof(double)) != hipSuccess ||
          hipMalloc((void**)&g->recv[k], blk * G * sizeof(double)) != hipSuccess)
        return gfail(g, "odef_allgather: out of device memory on device %d", c->device);
    }
  }
  // shards that share a device (a test rig with fewer GPUs than shards) cannot form an RCCL communicator: the gather
  // is then device-to-device copies
  bool distinct = true;
  for (int a = 0; a < G; ++a)
    for (int b = a + 1; b < G; ++b) distinct = distinct && g->ctx[a]->device != g->ctx[b]->device;
  if (g->comm.empty() && distinct) {
    std::string lerr;
    if (g_rccl.load(lerr)) {
      std::vector<int> devs(G);
      for (int k = 0; k < G; ++k) devs[k] = g->ctx[k]->device;
      g->comm.assign(G, nullptr);
      const int rc = g_rccl.CommInitAll(g->comm.data(), G, devs.data());
      if (rc != 0) {
        g->comm.clear();
        return gfail(g, "odef_allgather: ncclCommInitAll over %d devices failed: %s", G, g_rccl.GetErrorString(rc));
      }
    } else if (G > 1) {
      return gfail(g, "odef_allgather: %s", lerr.c_str());
    }
  }
  // pack the final means of every shard
  for (int k = 0; k < G; ++k) {
    odef_ctx* c = g->ctx[k];
    if (!c->solved) return gfail(g, "odef_allgather: shard %d has not been solved", k);
    const int f = smoothed ? ODEF_F_SMOOTH_MEAN : ODEF_F_MEAN;
    if (smoothed && !c->smoothed_done) return gfail(g, "odef_allgather: smoothed means requested but odef_group_smooth has not run");
    if (set_device(c)) return gfail(g, "odef_allgather: %s", c->err.c_str());
    const long N = (long)c->cfg.n_traj;
    hipLaunchKernelGGL(pack_final_kernel, dim3((unsigned)((g->cnt_max + 255) / 256)), dim3(256), 0, c->stream,
                       (const double*)c->f[f].ptr, c->adaptive ? (const int*)c->f[ODEF_F_NSAVED].ptr : (const int*)nullptr,
                       c->n_save, c->D, N, (long)g->cnt_max, g->send[k]);
  }
  // the one collective of the path: an all-gather over xGMI (RCCL), every device ends with all shards' blocks
  if (!g->comm.empty()) {
    int rc = g_rccl.GroupStart();
    for (int k = 0; k < G && rc == 0; ++k) {
      (void)hipSetDevice(g->ctx[k]->device);
      rc = g_rccl.AllGather(g->send[k], g->recv[k], blk, kNcclDouble, g->comm[k], g->ctx[k]->stream);
    }
    const int rc2 = g_rccl.GroupEnd();
    if (rc == 0) rc = rc2;
    if (rc != 0) return gfail(g, "odef_allgather: ncclAllGather failed: %s", g_rccl.GetErrorString(rc));
  } else {  // one device without RCCL, or shards sharing a device: the gather is a set of copies
    for (int k = 0; k < G; ++k)
      if (hipStreamSynchronize(g->ctx[k]->stream) != hipSuccess) return gfail(g, "odef_allgather: synchronisation failed");
    for (int k = 0; k < G; ++k)
      for (int j = 0; j < G; ++j)
        if (hipMemcpyAsync(g->recv[k] + (size_t)j * blk, g->send[j], blk * sizeof(double), hipMemcpyDeviceToDevice,
                           g->ctx[k]->stream) != hipSuccess)
          return gfail(g, "odef_allgather: device copy failed");
  }
  for (int k = 0; k < G; ++k) {
    (void)hipSetDevice(g->ctx[k]->device);
    if (hipStreamSynchronize(g->ctx[k]->stream) != hipSuccess) return gfail(g, "odef_allgather: synchronisation of device %d failed", g->ctx[k]->device);
  }
  g->gathered = true;
  return 0;
}

int odef_group_get_gathered(odef_group* g, int32_t shard, double* host_dst /* [D][n_total] */, void** dev_ptr, size_t* dev_bytes) {
  if (!g || shard < 0 || shard >= (int32_t)g->ctx.size()) return -1;
  if (!g->gathered) return gfail(g, "odef_group_get_gathered: call odef_allgather first");
  const int G = (int)g->ctx.size();
  const size_t blk = (size_t)g->D * (size_t)g->cnt_max;
  if (dev_ptr) *dev_ptr = g->recv[shard];
  if (dev_bytes) *dev_bytes = blk * G * sizeof(double);
  if (host_dst) {
    odef_ctx* c = g->ctx[shard];
    if (set_device(c)) return gfail(g, "odef_group_get_gathered: %s", c->err.c_str());
    std::vector<double> tmp(blk * G);
    if (hipMemcpy(tmp.data(), g->recv[shard], tmp.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return gfail(g, "odef_group_get_gathered: copy from device %d failed", c->device);
    if (odef_unpad_gathered(tmp.data(), G, g->D, g->n_total, host_dst) != 0) return gfail(g, "odef_group_get_gathered: inconsistent layout");
  }
  return 0;
}

}  // extern "C"

namespace odef {
namespace {
thread_local char g_last_kernel[192] = "";
}
void note_kernel(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_last_kernel, sizeof g_last_kernel, fmt, ap);
  va_end(ap);
}
const char* last_kernel() { return g_last_kernel; }

const FieldLaunch* field_launch(int rhs_id) {
  switch (rhs_id) {
    case ODEF_RHS_FHN: return field_fhn();
    case ODEF_RHS_LORENZ63: return field_lorenz63();
    case ODEF_RHS_LOTKA_VOLTERRA: return field_lotka_volterra();
    case ODEF_RHS_VANDERPOL: return field_vanderpol();
    case ODEF_RHS_LINEAR: return field_linear();
    case ODEF_RHS_FORCED: return field_forced();
    case ODEF_RHS_PLEIADES: return field_pleiades();
    case ODEF_RHS_LORENZ96: return field_lorenz96();
    default: return nullptr;
  }
}
}  // namespace odef
