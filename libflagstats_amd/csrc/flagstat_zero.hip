// flagstat_zero.hip -- the kernel behind fsk_zero_words (flagstat_kernels.h): the zeroes the store forms put in front of their kernel
// while their stream is being captured into a graph.  A translation unit and a code object of its own, so that K1's code object
// stays the one profiles/traffic.json was measured on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_kernels.h"

namespace fsk {
__global__ void zero_words(uint64_t* __restrict__ words, uint64_t nwords)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < nwords; i += stride) words[i] = 0;
}
}  // namespace fsk

extern "C" hipError_t fsk_launch_zero_words(uint64_t* d_words, uint64_t nwords, hipStream_t stream)
{
    if (nwords == 0) return hipSuccess;
    const uint64_t blocks = (nwords + fsk::kThreads - 1) / fsk::kThreads;
    const dim3 grid(static_cast<uint32_t>(blocks < 1024 ? blocks : 1024));
    hipLaunchKernelGGL(fsk::zero_words, grid, dim3(fsk::kThreads), 0, stream, d_words, nwords);
    return hipGetLastError();
}
