// ggc_outline.h — the 2x2 rule of mask outlines (include/ggc.h K1), shared by the kernels of
// ggc_outlines.hip and by a stand-alone host program (tests/outline_rule_main.cpp), as ccl_run_start_lane is shared.
//
// A corner (r, c) of the lattice sees four pixels, the BLOCK, as four bits (anything outside the image is clear):
//     1 = NW (r-1, c-1)    2 = NE (r-1, c)
//     4 = SW (r,   c-1)    8 = SE (r,   c)
// A crack is a unit step with a set pixel on its right and a clear one on its left; directions 0 = E, 1 = S, 2 = W, 3 = N.
// Integer only; nothing here touches memory.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GGC_OL_HD __host__ __device__ inline
#else
#define GGC_OL_HD inline
#endif

namespace ggc {

constexpr int OL_NW = 1, OL_NE = 2, OL_SW = 4, OL_SE = 8;

// The cracks that leave the corner: bit d is set iff the crack in direction d exists.
//   E: SE set, NE clear.   S: SW set, SE clear.   W: NW set, SW clear.   N: NE set, NW clear.
GGC_OL_HD int ol_leaving(int block) {
    const int nw = block & 1, ne = (block >> 1) & 1, sw = (block >> 2) & 1, se = (block >> 3) & 1;
    return (se & (ne ^ 1)) | ((sw & (se ^ 1)) << 1) | ((nw & (sw ^ 1)) << 2) | ((ne & (nw ^ 1)) << 3);
}

// The successor of a crack that arrives in direction d at a corner whose leaving cracks are `leaving`: the first that
// exists among left, straight, right (8 neighbours: diagonal pixels belong together) or right, straight, left (4).
// -1 when none of the three exists, which cannot happen at the head of a crack.  A U-turn is never tried.
GGC_OL_HD int ol_successor_of(int leaving, int d, int connectivity) {
    const int first = connectivity == 8 ? 3 : 1, last = connectivity == 8 ? 1 : 3;
    const int a = (d + first) & 3, c = (d + last) & 3;
    if ((leaving >> a) & 1) return a;
    if ((leaving >> d) & 1) return d;
    if ((leaving >> c) & 1) return c;
    return -1;
}
GGC_OL_HD int ol_successor(int block, int d, int connectivity) { return ol_successor_of(ol_leaving(block), d, connectivity); }

// The corner a crack leads to, and the pixel on its right, both relative to its tail (r, c).
GGC_OL_HD int ol_step_r(int d) { return d == 1 ? 1 : (d == 3 ? -1 : 0); }
GGC_OL_HD int ol_step_c(int d) { return d == 0 ? 1 : (d == 2 ? -1 : 0); }
GGC_OL_HD int ol_right_r(int d) { return d >= 2 ? -1 : 0; }            // E (r, c)   S (r, c-1)   W (r-1, c-1)   N (r-1, c)
GGC_OL_HD int ol_right_c(int d) { return (d == 1 || d == 2) ? -1 : 0; }

// The crack's term of the shoelace sum  c r' - c' r  (tail (r, c), head (r', c')): twice the loop's area is their sum, the
// points between two vertices add nothing.
GGC_OL_HD int ol_shoelace(int r, int c, int d) { return d == 0 ? -r : (d == 1 ? c : (d == 2 ? r : -c)); }

} // namespace ggc
