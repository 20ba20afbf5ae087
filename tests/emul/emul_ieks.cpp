// TEST INFRASTRUCTURE: host build of the IEKS step (ek_lane.h / rows_filter.h with IEKS = true) on top of the emulator of
// emul.cpp, so that the arithmetic of ek_filter_fixed_ieks_kernel and ek_filter_rows_ieks_kernel can be checked against the
// numpy restatement (tests/_ieks_reference.py) without a GPU.  Not part of the product.
#include "emul.cpp"

namespace {
struct RunFilterIeks {
  const FilterParams& P;
  int kernel;  // 0: lane kernel, 1: lane kernel with lagged record stores, 2: row-team kernel
  int rc = 0;
  template <class RHS, int q, bool EK1>
  void operator()() {
    if constexpr (!EK1) {
      rc = -2;
    } else {
      for (long i = 0; i < P.N; ++i) {
        const long i0 = (i / 64) * 64;
        if (kernel == 2) {
          if constexpr (RHS::d * (q + 1) <= 16) {
            std::vector<double> ws(RowsStep<RHS, q, true, true>::kLdsDoublesAdaptive);
            const RowsTeam tm{i, i, true, 0, ws.data(), nullptr};
            rows_filter_fixed<RHS, q, true, true, true>(P, tm);
          } else {
            rc = -3;
          }
        } else if (kernel == 1) {
          filter_fixed_lane<RHS, q, true, true, true, false, true>(P, i0, (unsigned)(i - i0));
        } else {
          filter_fixed_lane<RHS, q, true, true, false, false, true>(P, i0, (unsigned)(i - i0));
        }
      }
    }
  }
};
}  // namespace

// the fixed-grid filter of an IEKS context with ODEF_F_LINEARIZE_AT = lin ([n_t][d][N]); a->everystep must be 1
extern "C" int emul_filter_ieks(const EmulArgs* a, const double* lin, int kernel) {
  FilterParams P;
  std::memset(&P, 0, sizeof P);
  fill(*a, P);
  P.stagger = kernel == 1 ? 7 : kernel == 2 ? 9 : 0;
  P.lin = lin;
  RunFilterIeks r{P, kernel};
  int rc;
  switch (a->rhs) {
    case 0: rc = dispatch_order<RhsFHN>(a->q, 1, r); break;
    case 1: rc = dispatch_order<RhsLorenz63>(a->q, 1, r); break;
    case 2: rc = dispatch_order<RhsLotkaVolterra>(a->q, 1, r); break;
    case 3: rc = dispatch_order<RhsVanDerPol>(a->q, 1, r); break;
    case 4: rc = dispatch_order<RhsLinear>(a->q, 1, r); break;
    default: return -2;
  }
  return rc ? rc : r.rc;
}
