// The 2x2 rule of csrc/ggc_outline.h on the host: for every block (16), arrival direction (4) and connectivity (4, 8), one
// line "block d connectivity leaving successor", then the step, right-pixel and shoelace helpers against their definitions.
// tests/test_outline_rule_cpu.py holds the lines against a table written out by hand.  No HIP call: built for the host only.
#include <cstdio>
#include "../gcn-grabcut_amd/csrc/ggc_outline.h"

int main() {
    using namespace ggc;
    for (int block = 0; block < 16; ++block)
        for (int d = 0; d < 4; ++d)
            for (int conn = 4; conn <= 8; conn += 4) {
                const int leave = ol_leaving(block);
                const int a = ol_successor(block, d, conn), b = ol_successor_of(leave, d, conn);
                if (a != b) { std::printf("ol_successor and ol_successor_of differ at %d %d %d\n", block, d, conn); return 1; }
                std::printf("%d %d %d %d %d\n", block, d, conn, leave, a);
            }
    // a crack's head, the pixel on its right and its shoelace term, at a tail away from the origin
    const int dr[4] = {0, 1, 0, -1}, dc[4] = {1, 0, -1, 0};
    const int pr[4] = {0, 0, -1, -1}, pc[4] = {0, -1, -1, 0};
    for (int d = 0; d < 4; ++d) {
        if (ol_step_r(d) != dr[d] || ol_step_c(d) != dc[d] || ol_right_r(d) != pr[d] || ol_right_c(d) != pc[d]) {
            std::printf("step or right pixel wrong at direction %d\n", d);
            return 1;
        }
        for (int r = 0; r < 5; ++r)
            for (int c = 0; c < 7; ++c)
                if (ol_shoelace(r, c, d) != c * (r + dr[d]) - (c + dc[d]) * r) {
                    std::printf("shoelace term wrong at %d %d %d\n", r, c, d);
                    return 1;
                }
    }
    std::printf("ok\n");
    return 0;
}
