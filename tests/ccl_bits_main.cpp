// Host check of the two lane-mask functions of csrc/ggc_ccl.h, built and run by tests/test_ccl_bits_cpu.py.  A pair is a
// candidate for the run starts and a mask of valid lanes; the wave's starts follow from it as in the kernels: a valid lane
// starts a run if the candidate says so, if it is lane 0, or if the lane below it is not valid.  For every valid lane
// ccl_run_start_lane, and for every start ccl_run_length, must equal a plain walk over the lanes.
#include "../gcn-grabcut_amd/csrc/ggc_ccl.h"
#include <cstdio>

typedef unsigned long long u64;

static bool bit(u64 m, int lane) { return (m >> lane) & 1ull; }

// lanes lo .. hi - 1 are looked at; vmask has no lane outside them, or lo = 0 and hi = 64
static bool check(u64 cand, u64 vmask, int lo, int hi) {
    const u64 starts = vmask & (cand | ~(vmask << 1) | 1ull);
    for (int lane = lo; lane < hi; ++lane) {
        if (!bit(vmask, lane)) continue;
        int first = lane;
        while (!bit(starts, first)) --first;
        const int got = ggc::ccl_run_start_lane(starts, lane);
        if (got != first) { std::printf("starts %016llx lane %d: run starts at %d, got %d\n", starts, lane, first, got); return false; }
        if (!bit(starts, lane)) continue;
        int len = 1;
        while (lane + len < 64 && bit(vmask, lane + len) && !bit(starts, lane + len)) ++len;
        const int glen = ggc::ccl_run_length(starts, vmask, lane);
        if (glen != len) { std::printf("starts %016llx vmask %016llx lane %d: run of %d, got %d\n", starts, vmask, lane, len, glen); return false; }
    }
    return true;
}

static u64 splitmix(u64& s) {
    u64 z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    long pairs = 0;
    const int offsets[3] = {0, 26, 52};                          // 52 + 12 = 64: the window's top lane is lane 63
    for (int off : offsets)
        for (u64 c = 0; c < 4096; ++c)
            for (u64 v = 0; v < 4096; ++v, ++pairs)
                if (!check(c << off, v << off, off, off + 12)) return 1;
    u64 special[67];
    int n = 0;
    special[n++] = ~0ull;
    special[n++] = 0x5555555555555555ull;
    special[n++] = 0xAAAAAAAAAAAAAAAAull;
    for (int b = 0; b < 64; ++b) special[n++] = 1ull << b;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j, ++pairs)
            if (!check(special[i], special[j], 0, 64)) return 1;
    u64 seed = 20240611;
    for (int i = 0; i < 4096; ++i, ++pairs) {
        const u64 c = splitmix(seed), v = splitmix(seed);
        if (!check(c, v, 0, 64)) return 1;
    }
    std::printf("ok %ld\n", pairs);
    return 0;
}
