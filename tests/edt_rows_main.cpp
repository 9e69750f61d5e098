// The 1-D row rule of csrc/ggc_edt.h on the host, against the two-line brute minimum: every row of length <= 6 with entries in
// {0, 1, 2, 5, none}, seeded random rows up to length 300, and the worst case (all none but one end), each at every x, every
// cap of {0 = unbounded, 1, 4, 25, 10^4} and with and without the edge rule.  Prints the number of rule calls and "ok".
// tests/test_edt_rows_cpu.py builds it with the host sanitizers.  No HIP call: built for the host only.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../gcn-grabcut_amd/csrc/ggc_edt.h"

using namespace ggc;

static uint32_t brute(const std::vector<uint32_t>& g, int x, int64_t cap2, bool edge) {
    int64_t best = EDT_FAR;
    const int W = (int)g.size();
    for (int xx = edge ? -1 : 0; xx <= (edge ? W : W - 1); ++xx) {
        const bool outside = xx < 0 || xx >= W;
        if (!outside && g[xx] == EDT_NONE) continue;
        const int64_t v = outside ? 0 : g[xx], d = v * v + (int64_t)(x - xx) * (x - xx);
        if (d < best) best = d;
    }
    return (uint32_t)((cap2 > 0 && best > cap2) ? EDT_FAR : best);
}

static long long calls = 0;

static bool check_row(const std::vector<uint32_t>& g, const char* what) {
    const int64_t caps[5] = {0, 1, 4, 25, 10000};
    const int W = (int)g.size();
    for (int64_t cap : caps)
        for (int edge = 0; edge < 2; ++edge)
            for (int x = 0; x < W; ++x) {
                const int rcap = cap == 0 ? -1 : (int)edt_isqrt(cap);
                const uint32_t cap2 = cap == 0 ? EDT_FAR : (uint32_t)cap;
                const uint32_t got = edt_row_min([&](int xx) { return g[xx]; }, W, x, rcap, cap2, edge != 0);
                const uint32_t want = brute(g, x, cap, edge != 0);
                ++calls;
                if (got != want) {
                    std::printf("%s: W=%d x=%d cap=%lld edge=%d: rule %u, brute %u\n", what, W, x, (long long)cap, edge, got, want);
                    return false;
                }
            }
    return true;
}

int main() {
    const uint32_t vals[5] = {0, 1, 2, 5, EDT_NONE};
    for (int W = 1; W <= 6; ++W) {
        int n = 1;
        for (int i = 0; i < W; ++i) n *= 5;
        std::vector<uint32_t> g(W);
        for (int code = 0; code < n; ++code) {
            for (int i = 0, c = code; i < W; ++i, c /= 5) g[i] = vals[c % 5];
            if (!check_row(g, "exhaustive")) return 1;
        }
    }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int t = 0; t < 400; ++t) {
        const int W = 1 + (int)(next() % 300);
        const int none_pct = (int)(next() % 101), top = 1 + (int)(next() % (t % 2 ? 16384 : 40));
        std::vector<uint32_t> g(W);
        for (int i = 0; i < W; ++i) g[i] = (int)(next() % 100) < none_pct ? EDT_NONE : (uint32_t)(next() % (top + 1));
        if (!check_row(g, "random")) return 1;
    }
    for (int W : {1, 2, 64, 300}) {
        for (uint32_t v : {0u, 7u, 16384u}) {
            std::vector<uint32_t> g(W, EDT_NONE);
            g[0] = v;
            if (!check_row(g, "worst case, left end")) return 1;
            g[0] = EDT_NONE; g[W - 1] = v;
            if (!check_row(g, "worst case, right end")) return 1;
        }
        if (!check_row(std::vector<uint32_t>(W, EDT_NONE), "all none")) return 1;
    }
    for (int64_t v : {0ll, 1ll, 2ll, 3ll, 4ll, 24ll, 25ll, 26ll, 9999ll, 10000ll, (1ll << 29) - 1, 1ll << 29, 2ll * 16384 * 16384})
        if (edt_isqrt(v) * edt_isqrt(v) > v || (edt_isqrt(v) + 1) * (edt_isqrt(v) + 1) <= v) {
            std::printf("edt_isqrt(%lld) = %lld\n", (long long)v, (long long)edt_isqrt(v));
            return 1;
        }
    std::printf("%lld calls\nok\n", calls);
    return 0;
}
