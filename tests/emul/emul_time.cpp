// TEST INFRASTRUCTURE: host build of the filter kernels around a time-dependent field (RhsForced, has_time: ek_lane.h /
// rows_filter.h with P.tgrid set) on top of the emulator of emul.cpp, so that the arithmetic of the lane kernel (plain and
// lagged record stores), the row-team kernel, the adaptive kernels and their MV and IEKS twins can be checked against the
// reference (tests/_time_reference.py) without a GPU.  Not part of the product.
#include "emul.cpp"

namespace {
struct RunFilterTime {
  const FilterParams& P;
  int kernel;  // 0: lane kernel, 1: lane kernel with lagged record stores, 2: row-team kernel
  int adaptive;
  int rc = 0;
  template <class RHS, int q, bool EK1>
  void operator()() {
    const bool mv = P.fixed_diffusion >= 3;
    for (long i = 0; i < P.N; ++i) {
      const long i0 = (i / 64) * 64;
      const unsigned lane = (unsigned)(i - i0);
      if (P.lin) {  // IEKS: EK1, fixed grid, every step saved
        if constexpr (EK1) {
          if (kernel == 2) {
            std::vector<double> ws(RowsStep<RHS, q, true, true>::kLdsDoublesAdaptive);
            const RowsTeam tm{i, i, true, 0, ws.data(), nullptr};
            rows_filter_fixed<RHS, q, true, true, true>(P, tm);
          } else if (kernel == 1) {
            filter_fixed_lane<RHS, q, true, true, true, false, true>(P, i0, lane);
          } else {
            filter_fixed_lane<RHS, q, true, true, false, false, true>(P, i0, lane);
          }
        } else {
          rc = -2;
        }
      } else if (mv) {  // MV diffusion models: EK0, lane kernels
        if constexpr (!EK1) {
          if (adaptive) filter_adaptive_lane<RHS, q, false, true>(P, i0, lane);
          else if (!P.everystep) filter_fixed_lane<RHS, q, false, false, false, true>(P, i0, lane);
          else if (kernel == 1) filter_fixed_lane<RHS, q, false, true, true, true>(P, i0, lane);
          else filter_fixed_lane<RHS, q, false, true, false, true>(P, i0, lane);
        } else {
          rc = -2;
        }
      } else if (kernel == 2) {
        std::vector<double> ws(RowsStep<RHS, q, EK1>::kLdsDoublesAdaptive);
        const RowsTeam tm{i, i, true, 0, ws.data(), nullptr};
        if (adaptive) rows_filter_adaptive<RHS, q, EK1>(P, tm);
        else if (P.everystep) rows_filter_fixed<RHS, q, EK1, true>(P, tm);
        else rows_filter_fixed<RHS, q, EK1, false>(P, tm);
      } else if (adaptive) {
        filter_adaptive_lane<RHS, q, EK1>(P, i0, lane);
      } else if (!P.everystep) {
        filter_fixed_lane<RHS, q, EK1, false>(P, i0, lane);
      } else if (kernel == 1) {
        filter_fixed_lane<RHS, q, EK1, true, true>(P, i0, lane);
      } else {
        filter_fixed_lane<RHS, q, EK1, true>(P, i0, lane);
      }
    }
  }
};
}  // namespace

// the filter of RhsForced; tgrid [nsteps + 1] (fixed grids; the adaptive kernels take the time from their own t + dt),
// lin: ODEF_F_LINEARIZE_AT [n_t][d][N] of an IEKS context or null.  MV: a->fixed_diffusion 3 / 4 (diff then holds d per save).
extern "C" int emul_filter_time(const EmulArgs* a, const double* tgrid, const double* lin, int kernel) {
  FilterParams P;
  std::memset(&P, 0, sizeof P);
  fill(*a, P);
  P.stagger = 0;
  P.tgrid = tgrid;
  P.lin = lin;
  RunFilterTime r{P, kernel, a->adaptive};
  const int rc = dispatch_order<RhsForced>(a->q, a->ek1, r);
  return rc ? rc : r.rc;
}
