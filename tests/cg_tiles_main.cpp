// Host check of cg_list_tiles (csrc/ggc_cg.h), built and run by tests/test_cg_tiles_cpu.py.  On small tile grids the list
// must hold exactly the tiles within the ring of a tile with U, each once and in raster order, image after image; the runs
// must be contiguous and empty for an image that is not solved; the slot map must be the inverse of the list.
#include "../gcn-grabcut_amd/csrc/ggc_cg.h"
#include <cstdio>
#include <cstdlib>

using namespace ggc;

#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        if (!(cond)) { std::printf("%s: ", what); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

static long n_checked = 0;

// cnt [B][nty * ntx]; tile_px = the pixels of a tile, so that skip_u = nt * tile_px is "U covers every pixel"
static void check(const char* what, int B, int ntx, int nty, const std::vector<int32_t>& cnt, int ring, int64_t skip_u) {
    const int nt = ntx * nty;
    std::vector<int2> list;
    std::vector<CgImage> img;
    std::vector<int64_t> u;
    std::vector<int32_t> slot;
    const int n_solve = cg_list_tiles(B, ntx, nty, cnt.data(), ring, skip_u, list, img, u, &slot);
    CHECK((int)img.size() == B && (int)u.size() == B && (int)slot.size() == B * nt, "output sizes");
    int at = 0, want_solve = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* c = cnt.data() + (size_t)b * nt;
        int64_t total = 0;
        for (int k = 0; k < nt; ++k) total += c[k];
        const bool solved = total != 0 && total != skip_u;
        want_solve += solved;
        CHECK(u[b] == total, "image %d: U count %lld, want %lld", b, (long long)u[b], (long long)total);
        CHECK(img[b].tile_lo == at, "image %d: run starts at %d, the list stands at %d", b, img[b].tile_lo, at);
        CHECK(img[b].done == (solved ? 0 : 1), "image %d: done %d", b, img[b].done);
        CHECK(img[b].iters == 0 && img[b].rel == 0.0 && img[b].stop == 0.0, "image %d: state not cleared", b);
        for (int k = 0; k < nt; ++k) {                                   // brute force: any tile with U within the ring
            bool want = false;
            for (int j = 0; j < nt && solved; ++j)
                want = want || (c[j] > 0 && std::abs(j / ntx - k / ntx) <= ring && std::abs(j % ntx - k % ntx) <= ring);
            if (want) {
                CHECK(at < (int)list.size() && list[at].x == b && list[at].y == k, "image %d: tile %d missing or out of order at %d", b, k, at);
                CHECK(slot[(size_t)b * nt + k] == at, "image %d tile %d: slot %d, listed at %d", b, k, slot[(size_t)b * nt + k], at);
                ++at;
            } else {
                CHECK(slot[(size_t)b * nt + k] == -1, "image %d tile %d: slot %d of a tile not listed", b, k, slot[(size_t)b * nt + k]);
            }
            ++n_checked;
        }
        CHECK(img[b].tile_hi == at, "image %d: run ends at %d, the list stands at %d", b, img[b].tile_hi, at);
        CHECK(solved || img[b].tile_lo == img[b].tile_hi, "image %d: a skipped image with tiles", b);
    }
    CHECK(at == (int)list.size(), "%d entries beyond the last image", (int)list.size() - at);
    CHECK(n_solve == want_solve, "solve count %d, want %d", n_solve, want_solve);
    // without a slot map the same list
    std::vector<int2> list2;
    CHECK(cg_list_tiles(B, ntx, nty, cnt.data(), ring, skip_u, list2, img, u, nullptr) == n_solve && list2.size() == list.size(),
          "the list differs without a slot map");
    for (size_t k = 0; k < list.size(); ++k) CHECK(list2[k].x == list[k].x && list2[k].y == list[k].y, "entry %zu differs without a slot map", k);
}

int main() {
    const int PX = CG_T * CG_T;
    char what[96];
    const int grids[3][2] = {{1, 1}, {4, 1}, {3, 3}};                    // ntx, nty
    for (int ring = 0; ring <= 1; ++ring)
        for (const auto& g : grids) {
            const int ntx = g[0], nty = g[1], nt = ntx * nty;
            const int64_t full = (int64_t)nt * PX;
            // one image: U in each single tile in turn (corner, edge and middle tiles of the 3 x 3 grid), in a pair, nowhere
            for (int k = 0; k < nt; ++k) {
                std::vector<int32_t> c(nt, 0);
                c[k] = 1 + k;
                std::snprintf(what, sizeof what, "ring %d grid %dx%d U in tile %d", ring, ntx, nty, k);
                check(what, 1, ntx, nty, c, ring, full);
                c[nt - 1 - k] = PX;
                std::snprintf(what, sizeof what, "ring %d grid %dx%d U in tiles %d and %d", ring, ntx, nty, k, nt - 1 - k);
                check(what, 1, ntx, nty, c, ring, nt == 1 ? 0 : full);
            }
            std::snprintf(what, sizeof what, "ring %d grid %dx%d no U", ring, ntx, nty);
            check(what, 1, ntx, nty, std::vector<int32_t>(nt, 0), ring, full);
            // three images, the middle one without U / all U with the skip on / all U with the skip off
            for (int mid = 0; mid < 3; ++mid) {
                std::vector<int32_t> c(3 * nt, 0);
                c[0] = 3;
                c[2 * nt + nt - 1] = 5;
                if (mid > 0) for (int k = 0; k < nt; ++k) c[nt + k] = PX;
                std::snprintf(what, sizeof what, "ring %d grid %dx%d batch of three, middle %s", ring, ntx, nty,
                              mid == 0 ? "without U" : (mid == 1 ? "all U, skipped" : "all U, solved"));
                check(what, 3, ntx, nty, c, ring, mid == 1 ? full : 0);
            }
        }
    std::printf("ok %ld\n", n_checked);
    return 0;
}
