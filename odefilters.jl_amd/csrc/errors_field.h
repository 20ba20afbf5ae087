// The solution-error kernels of a vector field that has an `analytic` member (errors_kernels.h around TruthAnalytic<RHS>), and
// their launcher: what the field's FieldLaunch table carries as `errors` (nullptr for a field without one).  Included by the
// field's own translation unit -- inst_linear.hip, and the module jit.hip builds around a run-time compiled field.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "errors.h"
#include "errors_kernels.h"
#include "rhs.h"

namespace odef {

template <class RHS>
int errors_analytic(const ErrArgs& a, const AnalyticArgs& t, unsigned grid, unsigned block, size_t lds, double* truth_out, hipStream_t s,
                    char* kname, size_t kname_n) {
  using Truth = TruthAnalytic<RHS>;
  if (a.d != RHS::d) return -3;
  if (truth_out) {
    hipLaunchKernelGGL(errors_truth_kernel<Truth>, dim3(grid), dim3(block), 0, s, t, a.nsaved, a.N, a.n_save, a.d, truth_out);
  } else {
    constexpr int DR = RHS::d <= kErrRegD ? RHS::d : 0;
    hipLaunchKernelGGL((errors_partial_kernel<DR, Truth>), dim3(grid), dim3(block), lds, s, a, t);
    if (kname) std::snprintf(kname, kname_n, "odef::errors_partial_kernel<%d, odef::TruthAnalytic<odef::%s>>", DR, RHS::name);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class RHS>
constexpr ErrorsFieldFn errors_launcher() {
  if constexpr (HasAnalytic<RHS>::value) return &errors_analytic<RHS>;
  else return nullptr;
}

}  // namespace odef
