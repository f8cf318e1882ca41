// synthesis_amd — translation unit of the library: the free-running kernels for at most 16 trees per CU (free_kernel.cuh: four waves of four
// trees, every wave evaluating its own leaves; f16x2 network arithmetic). engine.hip declares the same instantiations `extern template`; built beside it by `make -j`.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/synthesis_amd.h"
#include "free_kernel.cuh"
#include "lane_instances.h"

namespace syn {
#define SYN_X(MODE, COUNT, FAST, PROF) template __global__ void selfplay_kernel_free<MODE, COUNT, FAST, PROF>(EngineParams);
SYN_FREE_LIST(SYN_X)
#undef SYN_X
}  // namespace syn
