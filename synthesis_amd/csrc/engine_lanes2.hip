// synthesis_amd — third translation unit of the library: the two-trees-per-lane kernels (lane2_kernel.cuh), compiled beside
// engine.hip and engine_conv.hip (`make -j3`). engine.hip declares the same instantiations `extern template` and launches them
// through their host stubs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/synthesis_amd.h"
#include "lane2_kernel.cuh"
#include "lane_instances.h"

namespace syn {
#define SYN_X(MODE, COUNT, FAST, NW, POLICY, TILE) template __global__ void selfplay_kernel_lanes2<MODE, COUNT, FAST, NW, POLICY, TILE>(EngineParams);
SYN_LANES2_LIST(SYN_X)
#undef SYN_X
}  // namespace syn
