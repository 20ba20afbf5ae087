#include "ek_kernels.h"
namespace odef {
const FieldLaunch* field_lorenz63() {
  static const FieldLaunch t = {3, lane_filter<RhsLorenz63>, lane_smooth<3>, nullptr, lane_dense<3>, lane_sample<3>, nullptr};
  return &t;
}
}  // namespace odef
