// Which 64 trajectories a wavefront of the fixed-step lane filter owns.  A header without dependencies, callable on host and
// device (tests/test_wave_map.py compiles it into a host program).
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define ODEF_WAVE_MAP_HD __host__ __device__
#else
#define ODEF_WAVE_MAP_HD
#endif

namespace odef {

constexpr int kWaveMapLanes = 64;
constexpr unsigned kWaveMapXcds = 8;

// First trajectory of workgroup `block` of `n_blocks` single-wave workgroups.
//   mode 0: the identity, block b owns trajectories [64 b, 64 b + 64).
//   mode 1: XCD-contiguous.  The dispatcher deals workgroups round-robin over the 8 XCDs, so under mode 0 the eight 512-byte
//           pieces of every 4 KB of a record row go through eight different L2s.  Here the blocks of one residue class
//           x = b % 8 own one contiguous range of slots instead: cnt_x = (n_blocks - x + 7) / 8 of them, starting at
//           first_x = sum of cnt_y over y < x, block b at slot first_x + b / 8.  With n_blocks = 8 a + r that is
//           cnt_x = a + (x < r) and first_x = x a + min(x, r).  A bijection of [0, n_blocks) for every n_blocks.
// The placement of blocks on XCDs is an assumption about speed only: every trajectory is computed by exactly one lane under
// either mode, whatever the hardware does, and its arithmetic does not depend on the wavefront that carries it.  With
// N % 64 != 0 the partial wave is the last SLOT, which under mode 1 is not the last block; the kernels guard each lane by
// i0 + lane < N.
ODEF_WAVE_MAP_HD inline long wave_first_trajectory(unsigned block, unsigned n_blocks, int mode) {
  unsigned slot = block;
  if (mode == 1) {
    const unsigned a = n_blocks / kWaveMapXcds, r = n_blocks % kWaveMapXcds, x = block % kWaveMapXcds;
    slot = x * a + (x < r ? x : r) + block / kWaveMapXcds;
  }
  return (long)slot * kWaveMapLanes;
}

}  // namespace odef
