// tests/test_trace_local_host.py: k_trace_fill_local, then k_trace_walk_local, of hinge_amd/csrc/trace_kernels.h (a copy made by the
// test, beside the host stand-ins of this directory) run on the CPU - a wavefront = 64 threads in lock step - under AddressSanitizer
// and UBSan, with guard words around the directions, the best cell, the trace, the kept cells and the score.  The cross-lane
// exchange of the fill's reduction is an array of 64 slots between two barriers.  The boxes arrive widened (the widening is the
// host's).  stdin: "n W tspace match diff min_score", then per box "abpos comp bbpos CONTIG READ aepos bepos" (bases as digits 0-3, the
// read as stored); stdout per box: status diffs score i0 j0 i1 j1 [the kept segments' trace values].
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
static int lanes[64];
static int lane_xor(int v, int lane_mask) {
    lanes[threadIdx.x] = v;
    pthread_barrier_wait(&bar);
    const int got = lanes[threadIdx.x ^ (unsigned)lane_mask];
    pthread_barrier_wait(&bar);
    return got;
}
using namespace hinge;
static std::vector<unsigned char> pack(const std::string& s) {
    std::vector<unsigned char> o((s.size() + 3) / 4 + 8, 0);
    for (size_t p = 0; p < s.size(); p++) o[p >> 2] |= (unsigned char)((s[p] - '0') << (6 - 2 * (p & 3)));
    return o;
}
int main() {
    int n, W, ts, match, diff, min_score;
    std::cin >> n >> W >> ts >> match >> diff >> min_score;
    const int tmax = ts <= 125 ? 255 : 65534;
    const int G = 0x5a5a5a5a;
    trace_lane_xor_host = lane_xor;
    for (int x = 0; x < n; x++) {
        int ab, comp, bb, ae, be;
        std::string A, B;
        std::cin >> ab >> comp >> bb >> A >> B >> ae >> be;
        std::vector<unsigned char> pa = pack(A), pb = pack(B);
        long long boffA = 0, boffB = 0;
        int rlA = (int)A.size(), rlB = (int)B.size();
        CnsSeqs SA{pa.data(), &boffA, &rlA}, SB{pb.data(), &boffB, &rlB};
        TraceJob J;
        J.a = 0; J.b = 0; J.comp = comp; J.ab = ab; J.ae = ae; J.bb = bb; J.be = be; J.blen = rlB; J.nseg = trace_segments(ab, ae, ts); J.pad = 0; J.dir_off = 3; J.trace_off = 2;
        const long long words = trace_dir_words(ae - ab, W);
        std::vector<unsigned> dirs((size_t)words + 6, 0xdeadbeefu);
        std::vector<unsigned short> tr((size_t)2 * J.nseg + 4, 0xffff);
        // the job is x = 0: its slots are [0, 3) of best, [0] of diffs / status / score and [0, 4) of clip, guard words on either side
        int best[9] = {G, G, G, -1, -1, -1, G, G, G};
        int diffs[3] = {G, -1, G}, status[3] = {G, -1, G}, score[3] = {G, -1, G}, clip[12] = {G, G, G, G, -1, -1, -1, -1, G, G, G, G};
        if (trace_lds_bytes(W) > sizeof(trace_lds)) return 3;
        memset(trace_lds, 0xa5, sizeof(trace_lds));
        pthread_barrier_init(&bar, nullptr, 64);
        std::vector<std::thread> th;
        for (int l = 0; l < 64; l++)
            th.emplace_back([&, l] { threadIdx = Idx3{(unsigned)l, 0, 0}; blockIdx = Idx3{0, 0, 0}; k_trace_fill_local(SA, SB, &J, 1, W, match, diff, dirs.data(), best + 3); });
        for (auto& t : th) t.join();
        pthread_barrier_destroy(&bar);
        for (int g = 0; g < 3; g++) if (dirs[g] != 0xdeadbeefu || dirs[(size_t)words + 3 + g] != 0xdeadbeefu) { printf("GUARD dirs\n"); return 4; }
        for (int g = 0; g < 3; g++) if (best[g] != G || best[6 + g] != G) { printf("GUARD best\n"); return 4; }
        threadIdx = Idx3{0, 0, 0}; blockIdx = Idx3{0, 0, 0};
        k_trace_walk_local(&J, 1, W, ts, tmax, match, diff, min_score, trace_local_margin(W), dirs.data(), best + 3, tr.data(), diffs + 1, status + 1, clip + 4, score + 1);
        if (tr[0] != 0xffff || tr[1] != 0xffff || tr[2 * J.nseg + 2] != 0xffff || tr[2 * J.nseg + 3] != 0xffff) { printf("GUARD trace\n"); return 4; }
        if (diffs[0] != G || diffs[2] != G || status[0] != G || status[2] != G || score[0] != G || score[2] != G) { printf("GUARD slots\n"); return 4; }
        for (int g = 0; g < 4; g++) if (clip[g] != G || clip[8 + g] != G) { printf("GUARD cells\n"); return 4; }
        const int* c = clip + 4;
        printf("%d %d %d %d %d %d %d", status[1], diffs[1], score[1], c[0], c[1], c[2], c[3]);
        if (status[1] == 0) {
            // the kept segments among the box's slots, and nothing written outside them
            const int first = (ab + c[0]) / ts - ab / ts, cnt = trace_segments(ab + c[0], ab + c[2], ts);
            for (int s = 0; s < J.nseg; s++) {
                const bool in = s >= first && s < first + cnt;
                for (int h = 0; h < 2; h++) {
                    const unsigned short v = tr[2 + 2 * s + h];
                    if (!in && v != 0xffff) { printf(" STRAY\n"); return 5; }
                    if (in) printf(" %d", (int)v);
                }
            }
        }
        printf("\n");
    }
    return 0;
}
