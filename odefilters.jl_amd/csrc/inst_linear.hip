#include "ek_kernels.h"
#include "errors_field.h"
namespace odef {
const FieldLaunch* field_linear() {
  static const FieldLaunch t = {2, lane_filter<RhsLinear>, lane_smooth<2>, nullptr, lane_dense<2>, lane_sample<2>, nullptr,
                                       errors_launcher<RhsLinear>()};
  return &t;
}
}  // namespace odef
