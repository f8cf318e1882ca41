// synthesis_amd — second translation unit of the library: the lane-per-tree kernels instantiated for Connect4ConvNet
// (POLICY == 2, convnet.cuh). They are 18 of the ~60 kernels of engine.hip and compile independently of everything else, so
// building them beside engine.hip (`make -j2`) takes the conv network's share out of the build's critical path. engine.hip
// declares the same instantiations `extern template` and launches them through their host stubs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/synthesis_amd.h"
#include "lane_kernel.cuh"
#include "lane_instances.h"

namespace syn {
#define SYN_X(MODE, COUNT, FAST, NW, PROF, POLICY) template __global__ void selfplay_kernel_lanes<MODE, COUNT, FAST, NW, PROF, POLICY>(EngineParams);
SYN_LANES_CONV_LIST(SYN_X)
#undef SYN_X
}  // namespace syn
