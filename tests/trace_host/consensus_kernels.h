// Host stand-in for hinge_amd/csrc/consensus_kernels.h, for tests/test_trace_host.py only: the three definitions trace_kernels.h uses
// of it (the packed-base fetch and the strand frame), restated; the real header needs a device compiler.
#pragma once
#include <hip/hip_runtime.h>
namespace hinge {
struct CnsSeqs { const unsigned char* bps; const long long* boff; const int* rlen; };
inline int cns_base(const unsigned char* bps, long long boff, int p) { return (int)((bps[boff + (p >> 2)] >> (6 - 2 * (p & 3))) & 3u); }
struct CnsPair {
    const unsigned char* abps; long long aoff;
    const unsigned char* bbps; long long boff;
    int comp, blen;
    int A(int x) const { return cns_base(abps, aoff, x); }
    int B(int x) const { return comp ? 3 - cns_base(bbps, boff, blen - 1 - x) : cns_base(bbps, boff, x); }
};
}  // namespace hinge
