#include "ek_kernels.h"
namespace odef {
const FieldLaunch* field_vanderpol() {
  static const FieldLaunch t = {2, lane_filter<RhsVanDerPol>, lane_smooth<2>, nullptr, lane_dense<2>, lane_sample<2>, nullptr};
  return &t;
}
}  // namespace odef
