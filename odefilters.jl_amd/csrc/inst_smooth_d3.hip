#include "ek_kernels.h"
namespace odef {
template int lane_smooth<3>(int, const SmoothParams&, double*, hipStream_t);
template int lane_dense<3>(int, const DenseParams&, double*, hipStream_t);
template int lane_sample<3>(int, const SampleParams&, double*, hipStream_t);
}  // namespace odef
