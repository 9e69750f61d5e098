// Host check of relax_tiles_holding (csrc/ggc_relax.h), built and run by tests/test_relax_tiles_cpu.py.  For every tile of a
// 3x3 grid and every pixel of the tile, the tiles the function names must be exactly the tiles whose 34x34 halo window
// (the tile grown by one pixel on each side) contains the pixel, each named once.
#include "../gcn-grabcut_amd/csrc/ggc_relax.h"
#include <cstdio>

int main() {
    using namespace ggc;
    const int G = 3;
    long checked = 0;
    for (int tyi = 0; tyi < G; ++tyi)
        for (int txi = 0; txi < G; ++txi)
            for (int ly = 0; ly < RX_T; ++ly)
                for (int lx = 0; lx < RX_T; ++lx) {
                    int named[G][G] = {};
                    relax_tiles_holding(tyi, txi, ly, lx, G, G, [&](int ny, int nx) {
                        if (ny < 0 || ny >= G || nx < 0 || nx >= G) { std::printf("tile (%d, %d) outside the grid\n", ny, nx); std::exit(1); }
                        ++named[ny][nx];
                    });
                    const int y = tyi * RX_T + ly, x = txi * RX_T + lx;
                    for (int ny = 0; ny < G; ++ny)
                        for (int nx = 0; nx < G; ++nx) {
                            const bool holds = y >= ny * RX_T - 1 && y <= ny * RX_T + RX_T && x >= nx * RX_T - 1 && x <= nx * RX_T + RX_T;
                            if (named[ny][nx] != (holds ? 1 : 0)) {
                                std::printf("pixel (%d, %d): tile (%d, %d) named %d times, holds it: %d\n", y, x, ny, nx, named[ny][nx], (int)holds);
                                return 1;
                            }
                            ++checked;
                        }
                }
    std::printf("ok %ld\n", checked);
    return 0;
}
