// Kernel templates of the lane and row-team paths (state dimension <= 32, the compiled-in fields of inst_*.hip and the lane
// modules jit.hip builds): one lane per trajectory, one 64-lane wavefront per workgroup, or row-per-lane teams; and their
// launchers.  (256 CUs x 4 SIMDs = 1024 wave slots at one wave per SIMD: 65 536 trajectories fill the chip exactly once;
// block size 64 lets the dispatcher spread waves over all SIMDs.)  The workgroup-per-trajectory kernels: team_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include "dispatch.h"
#include "smooth_rows.h"
#include "smooth_lane.h"
#include "dense_lane.h"
#include "sample_lane.h"
#include "rows_kernels.h"
#include "dense_rows.h"
#include "sample_rows.h"
#include "launch.h"
#include "wave_map.h"

namespace odef {

constexpr int kWave = 64;
inline unsigned lane_grid(long N) { return (unsigned)((N + kWave - 1) / kWave); }

// All waves run the same instruction stream and would reach their per-step store burst (91 x 512 B at D = 12) together; a
// one-off start skew spreads the bursts over the step period so that the HBM write stream is steady.  Speed only: results do
// not depend on it.
__device__ __attribute__((always_inline)) inline void stagger_start(const FilterParams& P) {
  if (P.stagger > 0) {
    const int n = (int)(blockIdx.x % 16u) * P.stagger;
    for (int k = 0; k < n; ++k) __builtin_amdgcn_s_sleep(1);  // 64 clocks each
  }
}
template <class RHS, int q, bool EK1, bool EVERY, bool LAG = false>
__global__ __launch_bounds__(kWave) void ek_filter_fixed_kernel(const FilterParams P) {
  const long i0 = wave_first_trajectory(blockIdx.x, gridDim.x, P.wave_map);  // wave-uniform, once, in front of the time loop
  stagger_start(P);
  if (i0 + threadIdx.x < P.N) filter_fixed_lane<RHS, q, EK1, EVERY, LAG>(P, i0, threadIdx.x);
}
template <class RHS, int q, bool EK1>
__global__ __launch_bounds__(kWave) void ek_filter_adaptive_kernel(const FilterParams P) {
  const long i0 = (long)blockIdx.x * kWave;
  if (i0 + threadIdx.x < P.N) filter_adaptive_lane<RHS, q, EK1>(P, i0, threadIdx.x);
}
// The same two kernels for the MV diffusion models :dynamicMV / :fixedMV (EK0 only; P.fixed_diffusion = 3 / 4), d diffusions per
// record.  Kernels of their own, so that the scalar-model kernels above stay what they are.
template <class RHS, int q, bool EVERY, bool LAG>
__global__ __launch_bounds__(kWave) void ek_filter_fixed_mv_kernel(const FilterParams P) {
  const long i0 = wave_first_trajectory(blockIdx.x, gridDim.x, P.wave_map);
  stagger_start(P);
  if (i0 + threadIdx.x < P.N) filter_fixed_lane<RHS, q, false, EVERY, LAG, true>(P, i0, threadIdx.x);
}
template <class RHS, int q>
__global__ __launch_bounds__(kWave) void ek_filter_adaptive_mv_kernel(const FilterParams P) {
  const long i0 = (long)blockIdx.x * kWave;
  if (i0 + threadIdx.x < P.N) filter_adaptive_lane<RHS, q, false, true>(P, i0, threadIdx.x);
}
// The IEKS step (P.lin set): EK1 with the Jacobian at the previous iterate's smoothed u, fixed grid, every step saved.  A
// kernel of its own, so that the EK1 kernels above stay what they are.
template <class RHS, int q, bool LAG>
__global__ __launch_bounds__(kWave) void ek_filter_fixed_ieks_kernel(const FilterParams P) {
  const long i0 = wave_first_trajectory(blockIdx.x, gridDim.x, P.wave_map);
  stagger_start(P);
  if (i0 + threadIdx.x < P.N) filter_fixed_lane<RHS, q, true, true, LAG, false, true>(P, i0, threadIdx.x);
}

// Smoother, dense output and sampling on row-per-lane teams (smooth_rows.h, dense_rows.h, sample_rows.h): 16 lanes per item
// for D <= 16 (4 items per wavefront), 32 lanes for D <= 32; per-team matrices in LDS.  The kernels of the scalar and of the
// MV diffusion models (MV: d diffusions per record) share one always-inline body each.
template <int D>
struct SmoothTeam {
  static constexpr int lanes = (D <= 16) ? 16 : 32;
  static unsigned grid(long items) { return (unsigned)((items + kWave / lanes - 1) / (kWave / lanes)); }
};
template <int d, int q, bool MV>
__device__ __attribute__((always_inline)) inline void smooth_team_entry(const SmoothParams& P) {
  constexpr int D = d * (q + 1), TEAM = SmoothTeam<D>::lanes, TPB = kWave / TEAM;
  using W = RowsWs<d, q + 1>;
  __shared__ double lds[TPB * W::size];
  const int team = threadIdx.x / TEAM, tid = threadIdx.x % TEAM;
  const long i = (long)blockIdx.x * TPB + team;
  RowState<D> st;
  if (i < P.N) smooth_rows_lane<d, q, TEAM, MV>(P, i, tid, lds + team * W::size, &st);
}
template <int d, int q>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_num_vgpr(128))) void rts_smooth_kernel(const SmoothParams P) {
  smooth_team_entry<d, q, false>(P);
}
// ... for the MV diffusion models: the one smoother of those models, at every ensemble size
template <int d, int q>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_num_vgpr(128))) void rts_smooth_mv_kernel(const SmoothParams P) {
  smooth_team_entry<d, q, true>(P);
}
// Smoother, one lane per trajectory (D <= 12): the read-only filter covariance of the step sits in
// lane-private LDS (78 doubles x 64 lanes = 39 KB per wave at D = 12), everything else in registers.
constexpr int kSmoothLaneMaxD = 12;
// Ensemble size from which the lane kernel is used.  Measured on Lorenz EK1(3), 1 023 steps: N = 2 048 / 4 096:
// 27.6 / 27.7 ms (lane) against 13.9 / 15.5 ms (row teams); N = 16 384: 30.4 against 42.4 ms.
// ODEF_SMOOTH_LANE_MIN_N overrides it (read at every launch, so tests can exercise both kernels).
constexpr long kSmoothLaneMinN = 6144;
inline long smooth_lane_min_n() { return env_long("ODEF_SMOOTH_LANE_MIN_N", kSmoothLaneMinN); }
// Ensemble size below which the every-step filter stores its records lagged by one step (LaggedSink, ek_lane.h);
// ODEF_FILTER_LAG_MAX_N overrides it (read at every launch).  On today's kernel the lagged form is the slower one wherever it
// was measured (Lorenz-63 EK1(3), 1 024 steps, lane filter forced: 4.88 / 4.91 / 5.10 ms against 4.54 / 4.56 / 4.67 ms at
// 4 096 / 16 384 / 24 576 trajectories, profiles/r04_lag_ab.jsonl), so it ends where the scalar models leave the row-team
// filter for the lane filter (kFilterRowsMaxN): no ensemble that reaches the lane filter by default stores lagged.  Below that
// size it stays what a forced lane filter and the models without a row-team filter (MV, D > 16; not measured) get.
constexpr long kFilterLagMaxN = kFilterRowsMaxN;
inline long filter_lag_max_n() { return env_long("ODEF_FILTER_LAG_MAX_N", kFilterLagMaxN); }
// Wave -> trajectory map of the fixed-step lane filter kernels (wave_map.h): 0 = identity, 1 = XCD-contiguous.
// ODEF_WAVE_MAP overrides it (read at every launch, so that both maps can be timed alternately within one process).
// Measured that way on the headline workload (65 536 x 1 024, every step saved; profiles/r04_wave_map_ab.jsonl): 8.85 ms under
// map 1 against 9.25 / 9.27 ms under map 0, -4.3 % with the two map-0 series 0.2 % apart; ensembles of 4 096 - 24 576
// trajectories (fewer waves than SIMDs) run the same under either map, within 0.1 %.
static_assert(kWaveMapLanes == kWave, "wave_map.h counts trajectories in wavefronts of the lane kernels");
constexpr long kWaveMapDefault = 1;
inline int wave_map_mode() { return (int)env_long("ODEF_WAVE_MAP", kWaveMapDefault); }
// Two kernels (fixed grid / adaptive records) so that each gets its own register allocation.
template <int d, int q, bool ADAPT>
__global__ __launch_bounds__(kWave) void rts_smooth_lane_kernel(const SmoothParams P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kWave];
  const long i0 = (long)blockIdx.x * kWave;
  const LaneMem xl{lds + threadIdx.x, kWave};
  const bool valid = i0 + threadIdx.x < P.N;
  long n_hi = P.n_save;
  if constexpr (ADAPT) n_hi = wave_uniform_max(valid ? (long)P.nsaved[i0 + threadIdx.x] : 0, valid);
  if (valid) smooth_lane_v2<d, q, ADAPT>(P, i0, threadIdx.x, xl, n_hi);
}

// Dense output: blockIdx.y = query time, one lane per trajectory (D <= 12).  The lane pairs of dense output and sampling keep
// a body each: through a shared entry the compiler schedules both kernels of a pair differently.
template <int d, int q>
__global__ __launch_bounds__(kWave) void dense_output_kernel(const DenseParams P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kWave];
  const long i = (long)blockIdx.x * kWave + threadIdx.x;
  const LaneMem xl{lds + threadIdx.x, kWave};
  if (i < P.N) dense_lane<d, q>(P, i, (long)blockIdx.y, xl);
}
template <int d, int q>
__global__ __launch_bounds__(kWave) void dense_output_mv_kernel(const DenseParams P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kWave];
  const long i = (long)blockIdx.x * kWave + threadIdx.x;
  const LaneMem xl{lds + threadIdx.x, kWave};
  if (i < P.N) dense_lane<d, q, true>(P, i, (long)blockIdx.y, xl);
}
// ... and 12 < D <= 32: one row-per-lane team per (trajectory, query time) item (dense_rows.h)
template <int d, int q, bool MV>
__device__ __attribute__((always_inline)) inline void dense_team_entry(const DenseParams& P) {
  constexpr int D = d * (q + 1), TEAM = SmoothTeam<D>::lanes, TPB = kWave / TEAM;
  using W = RowsWs<d, q + 1>;
  __shared__ double lds[TPB * W::size];
  const int team = threadIdx.x / TEAM, tid = threadIdx.x % TEAM;
  const long it = (long)blockIdx.x * TPB + team;  // item = (query time, trajectory), trajectory fastest
  RowState<D> st;
  if (it < P.N * P.n_q) dense_rows_lane<d, q, TEAM, MV>(P, it % P.N, it / P.N, tid, lds + team * W::size, &st);
}
template <int d, int q>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_num_vgpr(128))) void dense_rows_kernel(const DenseParams P) {
  dense_team_entry<d, q, false>(P);
}
template <int d, int q>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_num_vgpr(128))) void dense_rows_mv_kernel(const DenseParams P) {
  dense_team_entry<d, q, true>(P);
}

// Posterior sampling (sample_lane.h): one lane per (trajectory, sample); blockIdx.y = sample.
template <int d, int q>
__global__ __launch_bounds__(kWave) void sample_kernel(const SampleParams P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kWave];
  const long i = (long)blockIdx.x * kWave + threadIdx.x;
  const LaneMem xl{lds + threadIdx.x, kWave};
  const bool valid = i < P.N;
  const long n_hi = (P.adaptive && !P.tq) ? wave_uniform_max(valid ? (long)P.nsaved[i] : 0, valid) : P.n_save;
  if (valid) sample_lane<d, q>(P, i, (long)blockIdx.y, xl, n_hi);
}
template <int d, int q>
__global__ __launch_bounds__(kWave) void sample_mv_kernel(const SampleParams P) {
  constexpr int D = d * (q + 1), TRI = D * (D + 1) / 2;
  __shared__ double lds[TRI * kWave];
  const long i = (long)blockIdx.x * kWave + threadIdx.x;
  const LaneMem xl{lds + threadIdx.x, kWave};
  const bool valid = i < P.N;
  const long n_hi = (P.adaptive && !P.tq) ? wave_uniform_max(valid ? (long)P.nsaved[i] : 0, valid) : P.n_save;
  if (valid) sample_lane<d, q, true>(P, i, (long)blockIdx.y, xl, n_hi);
}
// ... and 12 < D <= 32: one row-per-lane team per (trajectory, sample) item (sample_rows.h)
template <int d, int q, bool MV>
__device__ __attribute__((always_inline)) inline void sample_team_entry(const SampleParams& P) {
  constexpr int D = d * (q + 1), TEAM = SmoothTeam<D>::lanes, TPB = kWave / TEAM;
  using W = RowsWs<d, q + 1>;
  __shared__ double lds[TPB * W::size];
  const int team = threadIdx.x / TEAM, tid = threadIdx.x % TEAM;
  const long it = (long)blockIdx.x * TPB + team;  // item = (sample, trajectory), trajectory fastest
  RowState<D> st;
  if (it < P.N * P.n_samples) sample_rows_lane<d, q, TEAM, MV>(P, it % P.N, it / P.N, tid, lds + team * W::size, &st);
}
template <int d, int q>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_num_vgpr(128))) void sample_rows_kernel(const SampleParams P) {
  sample_team_entry<d, q, false>(P);
}
template <int d, int q>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_num_vgpr(128))) void sample_rows_mv_kernel(const SampleParams P) {
  sample_team_entry<d, q, true>(P);
}

// The launchers, one per pass.  Each picks the model's mode once (scalar, MV, IEKS) and then walks one decision path -- size
// tests, lag, grid -- in which the mode only picks the kernel at the leaf.  WITH_MV: the kernels of the MV diffusion models
// (EK0; P.mv / P.fixed_diffusion 3 / 4) are instantiated beside the scalar ones; WITH_IEKS: the IEKS kernels (EK1, fixed grid,
// every step saved; P.lin set) beside the EK1 ones.  A launcher built without a mode's kernels returns -2 for it, and so does
// one asked for a pass its mode has no kernel for.  The MV kernels are named before the scalar ones: the order in which a
// translation unit instantiates the kernels of a pair changes the code the compiler gives the largest orders.
template <bool WITH_MV = true>
struct LaunchDenseT {
  const DenseParams& P;
  hipStream_t s;
  int rc = 0;
  template <int d, int q>
  void operator()() {
    if (P.mv) {
      if constexpr (WITH_MV) launch<d, q, true>();
      else rc = -2;
      return;
    }
    launch<d, q, false>();
  }
  template <int d, int q, bool MV>
  void launch() {
    constexpr int D = d * (q + 1);
    if constexpr (D <= kSmoothLaneMaxD) {
      const dim3 grid(lane_grid(P.N), (unsigned)P.n_q);
      if constexpr (MV) hipLaunchKernelGGL((dense_output_mv_kernel<d, q>), grid, dim3(kWave), 0, s, P);
      else hipLaunchKernelGGL((dense_output_kernel<d, q>), grid, dim3(kWave), 0, s, P);
    } else if constexpr (D <= 32) {
      const dim3 grid(SmoothTeam<D>::grid(P.N * P.n_q));
      if constexpr (MV) hipLaunchKernelGGL((dense_rows_mv_kernel<d, q>), grid, dim3(kWave), 0, s, P);
      else hipLaunchKernelGGL((dense_rows_kernel<d, q>), grid, dim3(kWave), 0, s, P);
    } else {
      rc = MV ? -2 : -3;
    }
  }
};
template <bool WITH_MV = true>
struct LaunchSampleT {
  const SampleParams& P;
  hipStream_t s;
  int rc = 0;
  template <int d, int q>
  void operator()() {
    if (P.mv) {
      if constexpr (WITH_MV) launch<d, q, true>();
      else rc = -2;
      return;
    }
    launch<d, q, false>();
  }
  template <int d, int q, bool MV>
  void launch() {
    constexpr int D = d * (q + 1);
    if constexpr (D <= kSmoothLaneMaxD) {
      const dim3 grid(lane_grid(P.N), (unsigned)P.n_samples);
      if constexpr (MV) hipLaunchKernelGGL((sample_mv_kernel<d, q>), grid, dim3(kWave), 0, s, P);
      else hipLaunchKernelGGL((sample_kernel<d, q>), grid, dim3(kWave), 0, s, P);
    } else if constexpr (D <= 32) {
      const dim3 grid(SmoothTeam<D>::grid(P.N * P.n_samples));
      if constexpr (MV) hipLaunchKernelGGL((sample_rows_mv_kernel<d, q>), grid, dim3(kWave), 0, s, P);
      else hipLaunchKernelGGL((sample_rows_kernel<d, q>), grid, dim3(kWave), 0, s, P);
    } else {
      rc = MV ? -2 : -3;
    }
  }
};
template <bool WITH_MV = true>
struct LaunchSmoothT {
  const SmoothParams& P;
  hipStream_t s;
  int rc = 0;
  template <int d, int q>
  void operator()() {
    if (P.mv) {
      if constexpr (WITH_MV && d * (q + 1) <= 32) launch<d, q, true>();
      else rc = -2;
      return;
    }
    launch<d, q, false>();
  }
  template <int d, int q, bool MV>
  void launch() {
    constexpr int D = d * (q + 1);
    // MV models: the row-team smoother at every ensemble size (the broadcast and lane smoothers carry one diffusion).
    // Scalar models, small state AND a large ensemble: one lane per trajectory.  A small ensemble does not fill the chip that
    // way (N / 64 wavefronts for 1 024 SIMDs); the row-per-lane team kernel gives TPB x fewer trajectories per wavefront, i.e.
    // more wavefronts, and wins below kSmoothLaneMinN.
    if constexpr (!MV && D <= kRowsMaxD) {
      if (P.N < smooth_rows_max_n()) {
        const dim3 grid(rows_grid(P.N));
        note_kernel("odef::rts_smooth_bcast_kernel<%d, %d, %s>", d, q, tf(P.adaptive));
        if (P.adaptive) hipLaunchKernelGGL((rts_smooth_bcast_kernel<d, q, true>), grid, dim3(kRowsBlock), 0, s, P);
        else hipLaunchKernelGGL((rts_smooth_bcast_kernel<d, q, false>), grid, dim3(kRowsBlock), 0, s, P);
        return;
      }
    }
    if constexpr (!MV && D <= kSmoothLaneMaxD) {
      if (P.N >= smooth_lane_min_n()) {
        const dim3 grid(lane_grid(P.N));
        note_kernel("odef::rts_smooth_lane_kernel<%d, %d, %s>", d, q, tf(P.adaptive));
        if (P.adaptive) hipLaunchKernelGGL((rts_smooth_lane_kernel<d, q, true>), grid, dim3(kWave), 0, s, P);
        else hipLaunchKernelGGL((rts_smooth_lane_kernel<d, q, false>), grid, dim3(kWave), 0, s, P);
        return;
      }
    }
    const dim3 grid(SmoothTeam<D>::grid(P.N));
    note_kernel(MV ? "odef::rts_smooth_mv_kernel<%d, %d>" : "odef::rts_smooth_kernel<%d, %d>", d, q);
    if constexpr (MV) hipLaunchKernelGGL((rts_smooth_mv_kernel<d, q>), grid, dim3(kWave), 0, s, P);
    else hipLaunchKernelGGL((rts_smooth_kernel<d, q>), grid, dim3(kWave), 0, s, P);
  }
};
// An MV context takes the lane kernels at every ensemble size: the row-team filters (rows_filter.h) carry the scalar models
// only.  IEKS takes the kernels at the ensemble-size thresholds of the EK1 kernels.
template <bool WITH_MV = true, bool WITH_IEKS = true>
struct LaunchFilterT {
  const FilterParams& P;
  int adaptive;
  hipStream_t s;
  int rc = 0;
  enum Mode { kScalar, kMv, kIeks };
  template <class RHS, int q, bool EK1>
  void operator()() {
    const bool mv = P.fixed_diffusion >= 3;
    if (P.lin) {
      if constexpr (WITH_IEKS && EK1) {
        if (!adaptive && P.everystep && !mv) return launch<RHS, q, EK1, kIeks>();
      }
      rc = -2;
    } else if (mv) {
      if constexpr (WITH_MV && !EK1) launch<RHS, q, EK1, kMv>();
      else rc = -2;
    } else {
      launch<RHS, q, EK1, kScalar>();
    }
  }
  template <class RHS, int q, bool EK1, Mode M>
  void launch() {
    if constexpr (RHS::d * (q + 1) <= kRowsMaxD && M != kMv) {
      if (P.N < filter_rows_max_n()) {  // small ensemble: 16 lanes per trajectory
        const dim3 grid(rows_grid(P.N));
        if constexpr (M == kIeks) {
          note_kernel("odef::ek_filter_rows_ieks_kernel<odef::%s, %d>", RHS::name, q);
          hipLaunchKernelGGL((ek_filter_rows_ieks_kernel<RHS, q>), grid, dim3(kRowsBlock), 0, s, P);
        } else if (adaptive) {
          note_kernel("odef::ek_filter_rows_adaptive_kernel<odef::%s, %d, %s>", RHS::name, q, tf(EK1));
          hipLaunchKernelGGL((ek_filter_rows_adaptive_kernel<RHS, q, EK1>), grid, dim3(kRowsBlock), 0, s, P);
        } else {
          note_kernel("odef::ek_filter_rows_kernel<odef::%s, %d, %s, %s>", RHS::name, q, tf(EK1), tf(P.everystep));
          if (P.everystep) hipLaunchKernelGGL((ek_filter_rows_kernel<RHS, q, EK1, true>), grid, dim3(kRowsBlock), 0, s, P);
          else hipLaunchKernelGGL((ek_filter_rows_kernel<RHS, q, EK1, false>), grid, dim3(kRowsBlock), 0, s, P);
        }
        return;
      }
    }
    const dim3 grid(lane_grid(P.N));
    if constexpr (M != kIeks) {
      if (adaptive) {
        if constexpr (M == kMv) {
          note_kernel("odef::ek_filter_adaptive_mv_kernel<odef::%s, %d>", RHS::name, q);
          hipLaunchKernelGGL((ek_filter_adaptive_mv_kernel<RHS, q>), grid, dim3(kWave), 0, s, P);
        } else {
          note_kernel("odef::ek_filter_adaptive_kernel<odef::%s, %d, %s>", RHS::name, q, tf(EK1));
          hipLaunchKernelGGL((ek_filter_adaptive_kernel<RHS, q, EK1>), grid, dim3(kWave), 0, s, P);
        }
        return;
      }
    }
    const bool lag = P.everystep && P.N < filter_lag_max_n();  // small ensemble: spread the record stores over the next step
    FilterParams Pw = P;  // this launch's copy: the wave map is chosen here
    Pw.wave_map = wave_map_mode();
    if constexpr (M == kIeks) {
      note_kernel("odef::ek_filter_fixed_ieks_kernel<odef::%s, %d, %s>", RHS::name, q, tf(lag));
      if (lag) hipLaunchKernelGGL((ek_filter_fixed_ieks_kernel<RHS, q, true>), grid, dim3(kWave), 0, s, Pw);
      else hipLaunchKernelGGL((ek_filter_fixed_ieks_kernel<RHS, q, false>), grid, dim3(kWave), 0, s, Pw);
    } else if constexpr (M == kMv) {
      note_kernel("odef::ek_filter_fixed_mv_kernel<odef::%s, %d, %s, %s>", RHS::name, q, tf(P.everystep), tf(lag));
      if (lag) hipLaunchKernelGGL((ek_filter_fixed_mv_kernel<RHS, q, true, true>), grid, dim3(kWave), 0, s, Pw);
      else if (P.everystep) hipLaunchKernelGGL((ek_filter_fixed_mv_kernel<RHS, q, true, false>), grid, dim3(kWave), 0, s, Pw);
      else hipLaunchKernelGGL((ek_filter_fixed_mv_kernel<RHS, q, false, false>), grid, dim3(kWave), 0, s, Pw);
    } else {
      note_kernel("odef::ek_filter_fixed_kernel<odef::%s, %d, %s, %s, %s>", RHS::name, q, tf(EK1), tf(P.everystep), tf(lag));
      if (lag) hipLaunchKernelGGL((ek_filter_fixed_kernel<RHS, q, EK1, true, true>), grid, dim3(kWave), 0, s, Pw);
      else if (P.everystep) hipLaunchKernelGGL((ek_filter_fixed_kernel<RHS, q, EK1, true>), grid, dim3(kWave), 0, s, Pw);
      else hipLaunchKernelGGL((ek_filter_fixed_kernel<RHS, q, EK1, false>), grid, dim3(kWave), 0, s, Pw);
    }
  }
};

// The launchers above with the signatures of a FieldLaunch table (launch.h); ONLYQ / ONLYEK1 as for dispatch_order.
// WITH_MV: with the kernels of the MV diffusion models (a run-time compiled field builds them only for an MV context, jit.hip);
// WITH_IEKS: with the IEKS kernels (EK1 only; a run-time compiled field builds them only for an IEKS context)
template <class RHS, int ONLYQ = 0, bool ONLYEK1 = false, bool WITH_MV = true, bool WITH_IEKS = true>
int lane_filter(int q, int ek1, const FilterParams& P, hipStream_t s, int adaptive, double*, size_t, long*) {
  LaunchFilterT<WITH_MV, WITH_IEKS> f{P, adaptive, s};
  const int rc = dispatch_order<RHS, ONLYQ, ONLYEK1>(q, ek1, f);
  return rc ? rc : f.rc;
}
template <int d, int ONLYQ = 0, bool WITH_MV = true>
int lane_smooth(int q, const SmoothParams& P, double*, hipStream_t s) {
  LaunchSmoothT<WITH_MV> f{P, s};
  const int rc = dispatch_smooth_order<d, ONLYQ>(q, f);
  return rc ? rc : f.rc;
}
template <int d, int ONLYQ = 0, bool WITH_MV = true>
int lane_dense(int q, const DenseParams& P, double*, hipStream_t s) {
  LaunchDenseT<WITH_MV> f{P, s};
  const int rc = dispatch_smooth_order<d, ONLYQ>(q, f);
  return rc ? rc : f.rc;
}
template <int d, int ONLYQ = 0, bool WITH_MV = true>
int lane_sample(int q, const SampleParams& P, double*, hipStream_t s) {
  LaunchSampleT<WITH_MV> f{P, s};
  const int rc = dispatch_smooth_order<d, ONLYQ>(q, f);
  return rc ? rc : f.rc;
}
// the smoother, dense output and sampler of d = 2 / 3 are instantiated once, in inst_smooth_d{2,3}.hip (whose ISA listing
// tests/test_build_hygiene.py checks); the fields' tables only point at them
extern template int lane_smooth<2>(int, const SmoothParams&, double*, hipStream_t);
extern template int lane_dense<2>(int, const DenseParams&, double*, hipStream_t);
extern template int lane_sample<2>(int, const SampleParams&, double*, hipStream_t);
extern template int lane_smooth<3>(int, const SmoothParams&, double*, hipStream_t);
extern template int lane_dense<3>(int, const DenseParams&, double*, hipStream_t);
extern template int lane_sample<3>(int, const SampleParams&, double*, hipStream_t);

}  // namespace odef
