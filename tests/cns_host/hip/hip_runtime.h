// Host stand-in for <hip/hip_runtime.h>, for tests/test_consensus_host.py only: enough to compile hinge_amd/csrc/consensus_kernels.h
// with g++ and run its kernels on the CPU - one thread after the other where a kernel has no barrier, a workgroup of host threads
// with a barrier for __syncthreads() where it has one (driver.cpp's launch()).  Atomics are plain while one thread runs and
// __atomic_* while several do.  The cross-lane shuffles of k_cns_call / k_cns_emit are declared so that the header compiles; those
// two kernels are not run here.
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
#define __shared__ static
#define HIP_DYNAMIC_SHARED(type, var) extern type var[];      // (the driver defines hinge::cnt_lds)
struct Idx3 { unsigned x, y, z; };
extern thread_local Idx3 threadIdx, blockIdx;
extern Idx3 gridDim, blockDim;
extern bool hip_host_parallel;       // several host threads run the kernel at once
void __syncthreads();
using std::max;
using std::min;
struct int2 { int x, y; };
inline int2 make_int2(int x, int y) { int2 v; v.x = x; v.y = y; return v; }
inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
inline unsigned __brev(unsigned v) {
    unsigned r = 0;
    for (int b = 0; b < 32; b++) r |= ((v >> b) & 1u) << (31 - b);
    return r;
}
template <typename T> inline T atomicAdd(T* p, T v) {
    if (hip_host_parallel) return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
    const T old = *p; *p = (T)(old + v); return old;
}
template <typename T> inline T atomicOr(T* p, T v) {
    if (hip_host_parallel) return __atomic_fetch_or(p, v, __ATOMIC_RELAXED);
    const T old = *p; *p = old | v; return old;
}
inline int atomicMax(int* p, int v) {
    if (!hip_host_parallel) { const int old = *p; if (v > old) *p = v; return old; }
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
template <typename T> inline T __shfl_xor(T, int) { abort(); }
template <typename T> inline T __shfl_up(T, int) { abort(); }
