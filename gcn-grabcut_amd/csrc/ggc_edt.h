// ggc_edt.h — the 1-D row rule of the exact distance transform (include/ggc.h K2), shared by the row
// kernel of ggc_distance.hip and by a stand-alone host program (tests/edt_rows_main.cpp), as ggc_outline.h is shared.
//
// A row of column distances g: g(x') is the distance, within column x', from this row to the nearest pixel of the class
// opposite to the pixel the rule is asked about: 0 where (row, x') itself is such a pixel, EDT_NONE where the column holds
// none.  The rule returns  min over x' of g(x')^2 + (x - x')^2,  EDT_FAR where nothing is in reach.
// Integer only; the rule reads g through a functor and touches no memory of its own.  Below it, the two passes of a step as
// per-column and per-pixel functions, so that the kernels are launch geometry and nothing else.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GGC_EDT_HD __host__ __device__ inline
#else
#define GGC_EDT_HD inline
#endif

namespace ggc {

constexpr uint32_t EDT_NONE = 0x7FFFu;          // all ones in the 15 bits a stored g has; a real g is at most 16384
constexpr uint32_t EDT_FAR = 0x7FFFFFFFu;       // GGC_DIST_FAR

// rcap: how far to look to each side, -1 = to the ends of the row.  cap2: a minimum above it is reported as EDT_FAR
// (EDT_FAR itself = no cap).  edge: the positions x' = -1 and x' = W count as opposite pixels of this row (g = 0 there).
// Exact: the candidates at offset k are at least k^2 away, so the walk outward stops once k^2 reaches the best so far.
// EDT_NONE never enters a sum; g <= 16384 and k <= 16384, so g^2 + k^2 <= 2^29.
template <class G>
GGC_EDT_HD uint32_t edt_row_min(G g, int W, int x, int rcap, uint32_t cap2, bool edge) {
    const uint32_t g0 = g(x);
    uint32_t best = g0 == EDT_NONE ? EDT_FAR : g0 * g0;
    if (edge) {
        const uint32_t e = (uint32_t)(x + 1 < W - x ? x + 1 : W - x);
        if (e * e < best) best = e * e;
    }
    const int reach = x > W - 1 - x ? x : W - 1 - x;
    const int kmax = (rcap < 0 || rcap > reach) ? reach : rcap;
    for (int k = 1; k <= kmax; ++k) {
        const uint32_t k2 = (uint32_t)k * (uint32_t)k;
        if (k2 >= best) break;
        if (x - k >= 0) {
            const uint32_t v = g(x - k);
            if (v != EDT_NONE && v * v + k2 < best) best = v * v + k2;
        }
        if (x + k < W) {
            const uint32_t v = g(x + k);
            if (v != EDT_NONE && v * v + k2 < best) best = v * v + k2;
        }
    }
    return best > cap2 ? EDT_FAR : best;
}

// floor(sqrt(v)) for 0 <= v < 2^62, in integers.
GGC_EDT_HD int64_t edt_isqrt(int64_t v) {
    int64_t r = 0;
    for (int64_t bit = int64_t(1) << 30; bit > 0; bit >>= 1)
        if ((r + bit) * (r + bit) <= v) r += bit;
    return r;
}

// ---- the two passes of a step, one pixel column / one pixel at a time (ggc_distance.hip runs them one per lane) ----------

// The reach of one step, per class of the pixel asked about (0 = background: its D_out, 1 = foreground: its D_in).
struct EdtReach {
    int rcap[2];            // columns / rows to look to each side, -1 = all
    uint32_t cap2[2];       // a magnitude above it is FAR (EDT_FAR = no cap)
};

enum EdtMode : int { EDT_D2 = 0, EDT_GROW, EDT_SHRINK, EDT_BORDER, EDT_TRIMAP };

// One class's reach for a squared radius r2 >= 0: nothing is further than 2 * 16383^2 < 2^29, so a larger r2 is no cap.
// FAR itself never counts as within a radius.
GGC_EDT_HD void edt_reach(int64_t r2, int& rcap, uint32_t& cap2) {
    if (r2 >= (int64_t(1) << 29)) { rcap = -1; cap2 = EDT_FAR - 1; }
    else { rcap = (int)edt_isqrt(r2); cap2 = (uint32_t)r2; }
}
// A class that is not asked about: look nowhere, every magnitude (>= 1) is FAR.
GGC_EDT_HD void edt_skip(int& rcap, uint32_t& cap2) { rcap = 0; cap2 = 0; }

// Column pass: column x of the image whose pixel (0, 0) is mask[0] / g[0].  Two sweeps: down leaves the distance to the
// nearest opposite pixel above, up takes the minimum with the one below.  Stored per pixel: g in the low 15 bits (EDT_NONE =
// none, and every g beyond the class's reach, which could not win), the pixel's class in bit 15.  Under `border` the rows
// -1 and H are background.  The loops are unrolled so that a lane has eight rows' loads in flight: the pass is bound by the
// latency of its one-byte loads, not by their bytes.
GGC_EDT_HD void edt_column(int H, int W, const EdtReach& reach, int border, int x, const uint8_t* __restrict__ mask,
                           uint16_t* __restrict__ g) {
    const int none = 1 << 20;                                           // as a row index: further than any real row
    int last0 = border ? -1 : -none, last1 = -none;
#pragma unroll 8
    for (int y = 0; y < H; ++y) {
        const int fg = mask[x + (size_t)y * W] != 0;
        const int d = y - (fg ? last0 : last1);
        g[x + (size_t)y * W] = (uint16_t)(d > 16384 ? EDT_NONE : (uint32_t)d);
        if (fg) last1 = y; else last0 = y;
    }
    int next0 = border ? H : none, next1 = none;
#pragma unroll 8
    for (int y = H - 1; y >= 0; --y) {
        const int fg = mask[x + (size_t)y * W] != 0;
        const int up = g[x + (size_t)y * W];
        int d = (fg ? next0 : next1) - y;
        if (d > 16384) d = (int)EDT_NONE;
        if (up < d) d = up;
        const int rc = reach.rcap[fg];
        if (rc >= 0 && d > rc) d = (int)EDT_NONE;
        g[x + (size_t)y * W] = (uint16_t)(d | (fg << 15));
        if (fg) next1 = y; else next0 = y;
    }
}

// Row pass: pixel x of a row of stored words.  A neighbour of the other class has g = 0, one of the pixel's own class its
// stored g.  Returns the magnitude in *mag (EDT_FAR = out of reach) and the pixel's class.
GGC_EDT_HD int edt_pixel(const uint16_t* row, int W, int x, const EdtReach& reach, int border, uint32_t* mag) {
    const uint32_t fg = (uint32_t)row[x] >> 15, cls = fg << 15;
    auto gx = [row, cls](int xx) -> uint32_t {
        const uint32_t v = row[xx];
        return ((v ^ cls) & 0x8000u) ? 0u : (v & 0x7FFFu);
    };
    *mag = edt_row_min(gx, W, x, reach.rcap[fg], reach.cap2[fg], border && fg);
    return (int)fg;
}

// What a modifier's last pass writes for a pixel of class fg whose magnitude is within its radius (near) or not.
GGC_EDT_HD uint8_t edt_threshold(int mode, int fg, bool near) {
    if (mode == EDT_GROW) return (uint8_t)(fg | (int)near);
    if (mode == EDT_SHRINK) return (uint8_t)(fg & (int)!near);
    if (mode == EDT_BORDER) return (uint8_t)near;
    return (uint8_t)(near ? 128 : (fg ? 255 : 0));
}

// The steps of ggc_modify_mask's op (0 GROW .. 5 TRIMAP): one, or two for OPEN and CLOSE.  Returns their number.
struct EdtStep { EdtReach reach; int mode; };
GGC_EDT_HD int edt_plan(int op, int64_t r2_a, int64_t r2_b, EdtStep steps[2]) {
    EdtStep grow, shrink, both;                                         // grow asks the background only, shrink the foreground only
    edt_reach(r2_a, grow.reach.rcap[0], grow.reach.cap2[0]);
    edt_skip(grow.reach.rcap[1], grow.reach.cap2[1]);
    grow.mode = EDT_GROW;
    edt_reach(r2_a, shrink.reach.rcap[1], shrink.reach.cap2[1]);
    edt_skip(shrink.reach.rcap[0], shrink.reach.cap2[0]);
    shrink.mode = EDT_SHRINK;
    edt_reach(r2_a, both.reach.rcap[1], both.reach.cap2[1]);
    edt_reach(r2_b, both.reach.rcap[0], both.reach.cap2[0]);
    both.mode = op == 2 ? EDT_BORDER : EDT_TRIMAP;
    switch (op) {
        case 0: steps[0] = grow; return 1;
        case 1: steps[0] = shrink; return 1;
        case 3: steps[0] = shrink; steps[1] = grow; return 2;
        case 4: steps[0] = grow; steps[1] = shrink; return 2;
        default: steps[0] = both; return 1;
    }
}

} // namespace ggc
