#include "ek_kernels.h"
namespace odef {
template int lane_smooth<2>(int, const SmoothParams&, double*, hipStream_t);
template int lane_dense<2>(int, const DenseParams&, double*, hipStream_t);
template int lane_sample<2>(int, const SampleParams&, double*, hipStream_t);
}  // namespace odef
