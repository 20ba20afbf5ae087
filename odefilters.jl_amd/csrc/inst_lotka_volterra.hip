#include "ek_kernels.h"
namespace odef {
const FieldLaunch* field_lotka_volterra() {
  static const FieldLaunch t = {2, lane_filter<RhsLotkaVolterra>, lane_smooth<2>, nullptr, lane_dense<2>, lane_sample<2>, nullptr};
  return &t;
}
}  // namespace odef
