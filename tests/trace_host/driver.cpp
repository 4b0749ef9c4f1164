// tests/test_trace_host.py: k_trace_fill and k_trace_walk of hinge_amd/csrc/trace_kernels.h (a copy made by the test, beside the host
// stand-ins of this directory) run on the CPU - a wavefront = 64 threads in lock step - under AddressSanitizer and UBSan, with guard
// words around every buffer.  stdin: "n W tspace", then per placement "abpos comp bbpos CONTIG READ aepos bepos" (bases as digits
// 0-3, the read as stored); stdout per placement: status diffs [trace values].
#include "trace_kernels.h"
#include <pthread.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <iostream>
thread_local Idx3 threadIdx, blockIdx;
namespace hinge { unsigned char trace_lds[1 << 18]; }
static pthread_barrier_t bar;
void __syncthreads() { pthread_barrier_wait(&bar); }
using namespace hinge;
static std::vector<unsigned char> pack(const std::string& s) {
    std::vector<unsigned char> o((s.size() + 3) / 4 + 8, 0);
    for (size_t p = 0; p < s.size(); p++) o[p >> 2] |= (unsigned char)((s[p] - '0') << (6 - 2 * (p & 3)));
    return o;
}
int main() {
    int n, W, ts;
    std::cin >> n >> W >> ts;
    const int tmax = ts <= 125 ? 255 : 65534;
    for (int x = 0; x < n; x++) {
        int ab, comp, bb;
        std::string A, B;
        std::cin >> ab >> comp >> bb >> A >> B;     // A = whole contig, B = whole stored read; the placement is A[ab..end), B frame [bb .. bb + blen)
        int ae, be;
        std::cin >> ae >> be;
        std::vector<unsigned char> pa = pack(A), pb = pack(B);
        long long boffA = 0, boffB = 0;
        int rlA = (int)A.size(), rlB = (int)B.size();
        CnsSeqs SA{pa.data(), &boffA, &rlA}, SB{pb.data(), &boffB, &rlB};
        TraceJob J;
        J.a = 0; J.b = 0; J.comp = comp; J.ab = ab; J.ae = ae; J.bb = bb; J.be = be; J.blen = rlB; J.nseg = trace_segments(ab, ae, ts); J.pad = 0; J.dir_off = 3; J.trace_off = 2;
        const long long words = trace_dir_words(ae - ab, W);
        std::vector<unsigned> dirs((size_t)words + 6, 0xdeadbeefu);
        std::vector<unsigned short> tr((size_t)2 * J.nseg + 4, 0xffff);
        int cost = -1, diffs = -1, status = -1;
        if (trace_lds_bytes(W) > sizeof(trace_lds)) return 3;
        memset(trace_lds, 0xa5, sizeof(trace_lds));
        pthread_barrier_init(&bar, nullptr, 64);
        std::vector<std::thread> th;
        for (int l = 0; l < 64; l++)
            th.emplace_back([&, l] { threadIdx = Idx3{(unsigned)l, 0, 0}; blockIdx = Idx3{0, 0, 0}; k_trace_fill(SA, SB, &J, 1, W, dirs.data(), &cost); });
        for (auto& t : th) t.join();
        pthread_barrier_destroy(&bar);
        // guard words around the job's directions untouched?
        for (int g = 0; g < 3; g++) if (dirs[g] != 0xdeadbeefu || dirs[(size_t)words + 3 + g] != 0xdeadbeefu) { printf("GUARD\n"); return 4; }
        threadIdx = Idx3{0, 0, 0}; blockIdx = Idx3{0, 0, 0};
        k_trace_walk(&J, 1, W, ts, tmax, dirs.data(), &cost, tr.data(), &diffs, &status);
        if (tr[0] != 0xffff || tr[1] != 0xffff || tr[2 * J.nseg + 2] != 0xffff) { printf("GUARD\n"); return 4; }
        printf("%d %d", status, diffs);
        if (status == 0) for (int k = 0; k < 2 * J.nseg; k++) printf(" %d", (int)tr[2 + k]);
        printf("\n");
    }
    return 0;
}
