#include "ek_kernels.h"
#include "errors_field.h"
namespace odef {
const FieldLaunch* field_forced() {
  static const FieldLaunch t = {2, lane_filter<RhsForced>, lane_smooth<2>, nullptr, lane_dense<2>, lane_sample<2>, nullptr,
                                       errors_launcher<RhsForced>()};
  return &t;
}
}  // namespace odef
