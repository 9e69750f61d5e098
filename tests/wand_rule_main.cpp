// The per-pixel rule of csrc/ggc_wand.h on the host: the reference sums of a seed and match(p, s).  A 6 x 7 image of seeded
// random bytes drawn from a few values; every pixel in turn is the seed (so every corner and border position), at every
// sample of {1, 3, 5}, against 24 random (pixel, tolerance) pairs each.  Prints the image, then one line per case:
//   r c n tolerance pr pc ref0 ref1 ref2 match
// tests/test_wand_rule_cpu.py builds it with the host sanitizers and compares every line with tests/wand_ref.py.
// No HIP call: built for the host only.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../gcn-grabcut_amd/csrc/ggc_wand.h"

using namespace ggc;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}

int main() {
    const int H = 6, W = 7;
    const uint8_t values[8] = {0, 1, 2, 100, 128, 200, 254, 255};
    std::vector<uint8_t> img((size_t)H * W * 3);
    for (auto& v : img) v = values[next_u32() % 8];
    std::printf("image %d %d", H, W);
    for (uint8_t v : img) std::printf(" %d", (int)v);
    std::printf("\n");
    const int tolerances[8] = {0, 1, 2, 27, 100, 128, 254, 255};
    long long cases = 0;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c)
            for (int n = 1; n <= 5; n += 2) {
                int32_t ref[3];
                wand_ref_sums(img.data(), H, W, r, c, n, ref);
                for (int k = 0; k < 24; ++k) {
                    const int pr = (int)(next_u32() % H), pc = (int)(next_u32() % W), tol = tolerances[next_u32() % 8];
                    const bool m = wand_match(&img[3 * ((size_t)pr * W + pc)], ref, n * n, n * n * tol);
                    std::printf("%d %d %d %d %d %d %d %d %d %d\n", r, c, n, tol, pr, pc, ref[0], ref[1], ref[2], (int)m);
                    ++cases;
                }
            }
    std::printf("%lld cases\nok\n", cases);
    return 0;
}
