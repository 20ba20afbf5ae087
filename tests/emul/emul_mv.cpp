// TEST INFRASTRUCTURE: host build of the MV diffusion models :dynamicMV / :fixedMV (ek_lane.h with MV = true: the body of
// ek_filter_fixed_mv_kernel, with and without lagged record stores; smooth_rows.h with MV = true: the body of
// rts_smooth_mv_kernel) on top of the emulator of emul.cpp, so that their arithmetic can be checked against the
// extended-precision fixtures (tests/golden/exact_model_*mv_ld.npz) without a GPU.  Not part of the product.
#include "emul.cpp"

namespace {
struct RunFilterMv {
  const FilterParams& P;
  int lag;  // 1: lagged record stores
  int rc = 0;
  template <class RHS, int q, bool EK1>
  void operator()() {
    if constexpr (EK1) {
      rc = -2;  // the MV models are EK0's
    } else {
      for (long i = 0; i < P.N; ++i) {
        const long i0 = (i / 64) * 64;
        if (lag) filter_fixed_lane<RHS, q, false, true, true, true>(P, i0, (unsigned)(i - i0));
        else filter_fixed_lane<RHS, q, false, true, false, true>(P, i0, (unsigned)(i - i0));
      }
    }
  }
};
struct RunSmoothMv {
  const SmoothParams& P;
  template <int d, int q>
  void operator()() {
    constexpr int D = d * (q + 1);
    if constexpr (D <= 32) {  // the team width of the device (ek_kernels.h SmoothTeam): 16 lanes for D <= 16, else 32
      constexpr int TEAM = (D <= 16) ? 16 : 32;
      std::vector<double> ws(RowsWs<d, q + 1>::size);
      std::vector<RowState<D>> st(TEAM);
      for (long i = 0; i < P.N; ++i) smooth_rows_lane<d, q, TEAM, true>(P, i, 0, ws.data(), st.data());
    }
  }
};
}  // namespace

// the fixed-grid, every-step filter of an MV context: a->fixed_diffusion 3 (:dynamicMV) / 4 (:fixedMV), a->ek1 0,
// a->diff [n_save][d][N]
extern "C" int emul_filter_mv(const EmulArgs* a, int lag) {
  if (a->fixed_diffusion != 3 && a->fixed_diffusion != 4) return -4;
  if (a->ek1 || a->everystep != 1 || a->adaptive) return -2;
  FilterParams P;
  std::memset(&P, 0, sizeof P);
  fill(*a, P);
  P.stagger = lag ? 7 : 0;
  RunFilterMv r{P, lag};
  int rc;
  switch (a->rhs) {
    case 0: rc = dispatch_order<RhsFHN>(a->q, 0, r); break;
    case 1: rc = dispatch_order<RhsLorenz63>(a->q, 0, r); break;
    case 2: rc = dispatch_order<RhsLotkaVolterra>(a->q, 0, r); break;
    case 3: rc = dispatch_order<RhsVanDerPol>(a->q, 0, r); break;
    case 4: rc = dispatch_order<RhsLinear>(a->q, 0, r); break;
    default: return -2;
  }
  return rc ? rc : r.rc;
}

// the MV instantiation of the row-team smoother over the records of emul_filter_mv (after the postamble, for :fixedMV)
extern "C" int emul_smooth_mv(const EmulArgs* a, int d) {
  SmoothParams P;
  std::memset(&P, 0, sizeof P);
  std::memcpy(P.pc.At, a->At, sizeof(P.pc.At));
  std::memcpy(P.pc.Qt, a->Qt, sizeof(P.pc.Qt));
  std::memcpy(P.pc.QLt, a->QLt, sizeof(P.pc.QLt));
  P.N = a->N; P.n_save = a->n_save; P.adaptive = 0; P.mv = 1;
  P.hs = a->hs; P.ptab = a->ptab; P.tab_idx = a->tab_idx; P.tsave = a->tsave; P.nsaved = a->nsaved;
  P.mean = a->mean; P.cov = a->cov; P.diff = a->diff; P.smean = a->smean; P.scov = a->scov;
  P.retcode = a->retcode;
  RunSmoothMv r{P};
  if (d == 2) return dispatch_smooth_order<2>(a->q, r);
  if (d == 3) return dispatch_smooth_order<3>(a->q, r);
  return -2;
}
