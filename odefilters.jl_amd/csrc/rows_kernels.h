// Kernels of the 16-lanes-per-trajectory mapping (rows_filter.h, rows_smooth.h, rows_store.h): small and sharded ensembles,
// state dimension <= 16.  In a header of their own so that jit.hip can build them around a run-time compiled vector field.
#pragma once
#include <hip/hip_runtime.h>
#include "rows_filter.h"
#include "rows_smooth.h"
#include "rows_launch.h"

namespace odef {

// Small / sharded ensembles: 16 lanes per trajectory (rows_filter.h), 4 trajectories per wavefront.
// Workgroups go round-robin over the 8 XCDs; the block -> trajectory map gives each XCD one contiguous range of
// trajectories, so that the 32-byte runs neighbouring wavefronts write into one cache line meet in the same L2.
// Workgroup = 4 wavefronts = 16 teams = 16 consecutive trajectories: one 128-byte line per record element (rows_store.h).
constexpr int kRowsBlock = kRowsWgTeams * tv::kTeam;  // 256 threads
static_assert(kRowsWgTeams == kRowsWgTraj && tv::kTeam == kRowsMaxD, "rows_launch.h sizes the grids of these kernels");
template <int d, int NB, int STAGE>
struct RowsLds {  // doubles: 16 teams' exchange rows + the staging image of the record stores
  static constexpr int team = tv::lds_rows(d, NB) * tv::lds_ld(d * NB);
  static constexpr int size = kRowsWgTeams * team + STAGE;
};
__device__ inline RowsTeam rows_team(long N, double* lds, int team_doubles) {
  const long per = (long)(gridDim.x / 8u);  // the grid is a multiple of 8 workgroups
  const long g = (long)(blockIdx.x % 8u) * per + (long)(blockIdx.x / 8u);
  RowsTeam tm;
  tm.tcol = (int)(threadIdx.x / tv::kTeam);
  tm.i16 = g * kRowsWgTeams;
  const long i = tm.i16 + tm.tcol;
  tm.valid = i < N;
  tm.i = tm.valid ? i : N - 1;  // padding teams of the last workgroup compute a duplicate and store nothing
  tm.lds_team = lds + tm.tcol * team_doubles;
  tm.stage = lds + kRowsWgTeams * team_doubles;
  return tm;
}
// (each kernel is a one-line wrapper around an always-inline entry, so that its modes -- EVERY, IEKS -- share one body)
template <class RHS, int q, bool EK1, bool EVERY, bool IEKS = false>
__device__ __attribute__((always_inline)) inline void rows_filter_fixed_entry(const FilterParams& P) {
  using L = RowsLds<RHS::d, q + 1, EVERY ? RowsSink<RHS::d*(q + 1), true, false>::kStageDoubles : 0>;
  __shared__ __attribute__((aligned(16))) double lds[L::size];
  const RowsTeam tm = rows_team(P.N, lds, L::team);
  if (tm.i16 < P.N) rows_filter_fixed<RHS, q, EK1, EVERY, IEKS>(P, tm);  // workgroup-uniform
}
template <class RHS, int q, bool EK1, bool EVERY>
__global__ __launch_bounds__(kRowsBlock) void ek_filter_rows_kernel(const FilterParams P) {
  rows_filter_fixed_entry<RHS, q, EK1, EVERY>(P);
}
// IEKS (P.lin set): the EK1 step with the Jacobian at the linearisation points, every step saved
template <class RHS, int q>
__global__ __launch_bounds__(kRowsBlock) void ek_filter_rows_ieks_kernel(const FilterParams P) {
  rows_filter_fixed_entry<RHS, q, true, true, true>(P);
}
template <class RHS, int q, bool EK1>
__device__ __attribute__((always_inline)) inline void rows_filter_adaptive_entry(const FilterParams& P) {
  using S = RowsStep<RHS, q, EK1>;
  constexpr int kStage = RowsSink<S::D, true, true>::kStageDoubles;
  __shared__ __attribute__((aligned(16))) double lds[kRowsWgTeams * S::kLdsDoublesAdaptive + kStage];
  const RowsTeam tm = rows_team(P.N, lds, S::kLdsDoublesAdaptive);
  if (tm.i16 < P.N) rows_filter_adaptive<RHS, q, EK1>(P, tm);
}
template <class RHS, int q, bool EK1>
__global__ __launch_bounds__(kRowsBlock) void ek_filter_rows_adaptive_kernel(const FilterParams P) {
  rows_filter_adaptive_entry<RHS, q, EK1>(P);
}
// Smoother on DPP broadcasts (rows_smooth.h), 16 lanes per trajectory, D <= 16: small and sharded ensembles.
// (which ensemble sizes it serves: smooth_rows_max_n, launch.h)
#ifndef ODEF_ROWS_SMOOTH_WAVES
#define ODEF_ROWS_SMOOTH_WAVES 2  // waves per SIMD the smoother is compiled for (<= 256 registers)
#endif
template <int d, int q, bool ADAPT>
__device__ __attribute__((always_inline)) inline void rows_smooth_entry(const SmoothParams& P) {
  using SM = RowsSmoother<d, q, ADAPT>;
  constexpr int kStage = RowsSink<d*(q + 1), false, false>::kStageDoubles;
  __shared__ __attribute__((aligned(16))) double lds[kRowsWgTeams * SM::kLdsDoubles + kStage];
  __shared__ int wg_n_hi;
  const RowsTeam tm = rows_team(P.N, lds, SM::kLdsDoubles);
  if (tm.i16 >= P.N) return;  // workgroup-uniform
  long n_hi = P.n_save;
  if constexpr (ADAPT) {  // largest record count among the workgroup's trajectories
    if (threadIdx.x == 0) wg_n_hi = 0;
    __syncthreads();
    if (tm.valid && threadIdx.x % tv::kTeam == 0) atomicMax(&wg_n_hi, P.nsaved[tm.i]);
    __syncthreads();
    n_hi = wg_n_hi;
  }
  RowsSmoother<d, q, ADAPT> sm;
  sm.run(P, tm, n_hi);
}
template <int d, int q, bool ADAPT>
__global__ __launch_bounds__(kRowsBlock) void rts_smooth_bcast_kernel(const SmoothParams P) {
  rows_smooth_entry<d, q, ADAPT>(P);
}

}  // namespace odef
