#include "ek_kernels.h"
namespace odef {
const FieldLaunch* field_linear() {
  static const FieldLaunch t = {2, lane_filter<RhsLinear>, lane_smooth<2>, nullptr, lane_dense<2>, lane_sample<2>, nullptr};
  return &t;
}
}  // namespace odef
