// Per-trajectory solution errors (errors.h).  One lane per trajectory walks the trajectory's saves; the time axis
// is cut into chunks so that the grid covers the device (errors_split), and a second small kernel folds the chunks in chunk
// order.  No floating-point atomics: the order of every sum depends on (N, d, n_save) only, two requests agree bit for bit.
//
//   errors_partial_kernel<DR, TruthBuffer>     here: the truth is a bound reference buffer
//   errors_partial_kernel<DR, TruthAnalytic>   in the field's own translation unit (errors_field.h), reached through
//                                              FieldLaunch::errors
//   errors_fold_kernel                         here, for both
#include "errors.h"

#include <cstdint>
#include <cstdio>

#include "errors_kernels.h"

namespace odef {
namespace {

template <int DR>
void launch_buffer(const ErrArgs& a, const TruthBuffer::Args& t, unsigned grid, unsigned block, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL((errors_partial_kernel<DR, TruthBuffer>), dim3(grid), dim3(block), lds, st, a, t);
}

AnalyticArgs analytic_args(const ErrorsRequest& r) {
  AnalyticArgs t;
  t.u0 = r.u0;
  t.p = r.p;
  t.t = r.t;
  t.N = r.N;
  t.t_sk = r.t_sk;
  t.t_si = r.t_si;
  t.p_shared = r.p_shared;
  return t;
}

}  // namespace

int errors_run(ErrorsState& st, ErrorsCache& c, const ErrorsRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname,
               size_t kname_n, std::string& err) {
  c.valid = false;
  const int tri = r.d * (r.d + 1) / 2;
  if (r.d < 1 || r.d > 32 || r.d > r.D || tri > r.TRI || r.N < 1 || r.n_save < 1)
    return pass_fail(err, "solution errors: built for d <= 32");
  if (!r.ref && !r.field) return pass_fail(err, "solution errors: no truth");
  ErrArgs a;
  a.mean = r.mean;
  a.cov = r.cov;
  a.tsave = r.tsave;
  a.nsaved = r.nsaved;
  a.N = r.N;
  a.n_save = r.n_save;
  a.d = r.d;
  a.D = r.D;
  a.TRI = r.TRI;
  a.lanes = errors_lanes(r.d);
  a.n_split = errors_split(r.N, r.n_save, a.lanes);
  a.chunk = (r.n_save + a.n_split - 1) / a.n_split;
  const long n_block = (r.N + a.lanes - 1) / a.lanes;
  if (n_block * a.n_split >= (1l << 31)) return pass_fail(err, "solution errors: more than 2^31 workgroups; shard the ensemble");
  const bool regs = r.d <= kErrRegD;
  const unsigned grid = (unsigned)(n_block * a.n_split), block = regs ? kErrBlock : 64;
  const size_t lds = regs ? 0 : (size_t)(tri + r.d) * a.lanes * sizeof(double);
  if (!c.nused) {
    bool ok = hipMalloc((void**)&c.nused, sizeof(long long) * r.N) == hipSuccess;
    for (double*& v : c.val) ok = ok && hipMalloc((void**)&v, sizeof(double) * r.N) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      return pass_fail(err, "solution errors: out of device memory");
    }
  }
  if (!grow((void**)&st.part, &st.part_cap, sizeof(double) * (size_t)a.n_split * kErrPartRows * r.N) ||
      !grow((void**)&st.part_cnt, &st.cnt_cap, sizeof(int) * (size_t)a.n_split * 2 * r.N))
    return pass_fail(err, "solution errors: out of device memory");
  a.part = st.part;
  a.part_cnt = st.part_cnt;
  if (st.timer.begin(stream) != hipSuccess) return pass_fail(err, "solution errors: hipEventCreate failed");
  if (r.ref) {
    const TruthBuffer::Args t{r.ref, r.N, r.d};
    switch (regs ? r.d : 0) {
      case 1: launch_buffer<1>(a, t, grid, block, lds, stream); break;
      case 2: launch_buffer<2>(a, t, grid, block, lds, stream); break;
      case 3: launch_buffer<3>(a, t, grid, block, lds, stream); break;
      case 4: launch_buffer<4>(a, t, grid, block, lds, stream); break;
      case 5: launch_buffer<5>(a, t, grid, block, lds, stream); break;
      case 6: launch_buffer<6>(a, t, grid, block, lds, stream); break;
      case 7: launch_buffer<7>(a, t, grid, block, lds, stream); break;
      case 8: launch_buffer<8>(a, t, grid, block, lds, stream); break;
      default: launch_buffer<0>(a, t, grid, block, lds, stream); break;
    }
    if (kname) std::snprintf(kname, kname_n, "odef::errors_partial_kernel<%d, odef::TruthBuffer>", regs ? r.d : 0);
  } else if (r.field(a, analytic_args(r), grid, block, lds, nullptr, stream, kname, kname_n)) {
    return pass_fail(err, "solution errors: the field's analytic launcher failed");
  }
  hipLaunchKernelGGL(errors_fold_kernel<>, dim3((unsigned)((r.N + 255) / 256)), dim3(256), 0, stream, (const double*)st.part,
                     (const int*)st.part_cnt, a.n_split, r.N, r.d, c.val[0], c.val[1], c.val[2], c.val[3], c.nused);
  if (const hipError_t e = st.timer.end(stream, ms); e != hipSuccess)
    return pass_fail(err, "solution errors: %s", hipGetErrorString(e));
  if (n_launches) *n_launches = 2;
  c.valid = true;
  return 0;
}

int errors_truth(ErrorsCache& c, const ErrorsRequest& r, hipStream_t stream, std::string& err) {
  c.truth_valid = false;
  if (!r.field) return pass_fail(err, "solution errors: no analytic");
  if (!grow((void**)&c.truth, &c.truth_cap, sizeof(double) * (size_t)r.n_save * r.d * r.N))
    return pass_fail(err, "solution errors: out of device memory");
  const long n_block = (r.N + kErrBlock - 1) / kErrBlock;
  if (n_block * r.n_save >= (1l << 31)) return pass_fail(err, "solution errors: more than 2^31 workgroups; shard the ensemble");
  ErrArgs a{};
  a.nsaved = r.nsaved;
  a.N = r.N;
  a.n_save = r.n_save;
  a.d = r.d;
  hipError_t e = hipSuccess;
  if (r.field(a, analytic_args(r), (unsigned)(n_block * r.n_save), kErrBlock, 0, c.truth, stream, nullptr, 0)) e = hipErrorLaunchFailure;
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return pass_fail(err, "solution errors: %s", hipGetErrorString(e));
  c.truth_valid = true;
  return 0;
}

void errors_free(ErrorsState& st) {
  for (ErrorsCache& c : st.src) free_device(c.val[0], c.val[1], c.val[2], c.val[3], c.nused, c.truth);
  free_device(st.part, st.part_cnt);
  st.timer.destroy();
  st = ErrorsState{};
}

}  // namespace odef
