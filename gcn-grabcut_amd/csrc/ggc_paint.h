// ggc_paint.h — the tile painter shared by ggc_hints.hip, ggc_strokes.hip and ggc_polygons.hip.
//
// One workgroup of 256 lanes paints one 32x8 pixel tile of one image, a lane per pixel.  The image's primitives (clicks,
// segments, polygon edges) are taken 256 at a time, a lane per primitive; the ones that can reach the tile go into an LDS
// list IN PRIMITIVE ORDER (paint_slot) and every lane walks it for its pixel, a later entry overwriting an earlier one: "the
// last primitive wins" follows the index, not timing.  Three barriers per pass: in paint_slot, after the records are
// stored, after the walk.  The pass loop is written out in each kernel: the records and what a walk carries differ.
#pragma once
#include "ggc_internal.h"

namespace ggc {

constexpr int PT_W = 32, PT_H = 8, PT_THREADS = PT_W * PT_H;   // 4 waves, each two 32-pixel rows of the tile

// This lane's pixel: image b = blockIdx.y, tile blockIdx.x of tiles_x per row of tiles, pixel (y, x) at offset p of the batch.
struct PaintTile {
    int b, tx0, ty0, x, y;
    bool inside;                           // the tile may hang over the image's right and lower border
    size_t p;
};
__device__ __forceinline__ PaintTile paint_tile(int H, int W, int tiles_x) {
    PaintTile t;
    const int tid = threadIdx.x;
    t.b = blockIdx.y;
    t.tx0 = (blockIdx.x % tiles_x) * PT_W; t.ty0 = (blockIdx.x / tiles_x) * PT_H;
    t.x = t.tx0 + (tid & (PT_W - 1)); t.y = t.ty0 + tid / PT_W;
    t.inside = t.x < W && t.y < H;
    t.p = (size_t)t.b * H * W + (size_t)t.y * W + t.x;
    return t;
}

// Order-keeping compaction over the workgroup: pos = the number of keepers among the lanes before this one (its slot in
// the list), n = the workgroup's keepers, extra = the OR of `extra` over the workgroup.  Per-wave ballot, the wave's count
// in s_wave[wave], the pass's first barrier, a prefix over the four waves.  With EXTRA the bit travels above the count in
// the same word; without it `extra` is ignored (pass false) and the word is the count alone.  Every lane of the workgroup
// calls it; s_wave: PT_THREADS / WAVE words of LDS, free to be rewritten after the pass's next barrier.
struct PaintSlot { int pos, n; bool extra; };
template <bool EXTRA>
__device__ __forceinline__ PaintSlot paint_slot(bool keep, bool extra, int* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    const int wave_extra = EXTRA && __ballot(extra) != 0;
    if (lane == 0) s_wave[wave] = __popcll(m) | (wave_extra << 16);
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull)), sum = 0;
    for (int w = 0; w < PT_THREADS / WAVE; ++w) {
        pos += w < wave ? s_wave[w] : 0;
        sum += s_wave[w];
    }
    if (!EXTRA) return PaintSlot{pos, sum, false};
    return PaintSlot{pos & 0xffff, sum & 0xffff, (sum >> 16) != 0};
}

} // namespace ggc
