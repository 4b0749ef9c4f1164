// Host stand-in for <hip/hip_runtime.h>, for tests/test_trace_host.py only: enough to compile hinge_amd/csrc/trace_kernels.h with g++
// and run a kernel as 64 host threads in lock step (threadIdx is thread-local, __syncthreads() a barrier of the 64).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__
#define __align__(x)
struct Idx3 { unsigned x, y, z; };
extern thread_local Idx3 threadIdx, blockIdx;
void __syncthreads();
using std::max;
using std::min;
