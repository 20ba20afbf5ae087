// Lorenz-96 with 16 variables on the workgroup-per-trajectory kernels (state dimension 32 .. 96): the matrix-core filter (fixed
// grids and adaptive), smoother (persistent and split pass), dense output and sampler instantiated for a second shape
// (d = 16: derivative blocks of two 8-row tiles) -- the kernels of filter_mfma.h / smooth_mfma.h are not Pleiades-shaped.
#include "team_launch_impl.h"
namespace odef {
const FieldLaunch* field_lorenz96() {
  static const FieldLaunch t = {16, team_filter<RhsLorenz96>, team_smooth_inplace<16>, team_smooth_staged<16>, team_dense<16>, team_sample<16>, team_smooth_ws<16>};
  return &t;
}
}  // namespace odef
