// ggc_fullcut.hip — O3f: a working-size binary mask carried to a larger size as the start of a banded graph cut there
// (Lombaert, Sun, Grady and Xu, ICCV 2005): the lifted mask, and GrabCut labels that leave only a band around the lifted
// mask's edge open.  include/ggc.h states the definition; DESIGN.md §5.18 the tiling and the bytes.
//
// The result is one byte per full-size pixel, and nothing wider is ever written: the lifted mask M1, its edge E and the
// dilations live as bit planes, one 64-bit word per 64 pixels of a row (bit j of word w of a row = pixel 64 w + j).
//   k_fc_mask    M1 per pixel from the working mask (the float64 bilinear value >= 0.5), 64 pixels of a row packed into a
//                word by one wave's ballot                                                     -> plane M  (1/8 B / pixel)
//   k_fc_hdil    per word: E from the 3 x 3 neighbourhood of M (three rows, shifts by one bit with the carry of the
//                neighbour words), then the horizontal dilation by `band` as shifts and ORs     -> plane Hd (1/8 B / pixel)
//   k_fc_labels  per block a strip of 32 rows x 256 pixels: the 32 + 2 band rows of Hd in LDS, their vertical OR = U,
//                then the label bytes M1 | U << 1 (0 BGD, 1 FGD, 2 PR_BGD, 3 PR_FGD) as 16-byte stores
// A neighbourhood clipped to the image holds both values exactly when the replicated one does, so the rows above the
// first and below the last are read as those rows, and for the AND the bits outside the image count as set.
#include "ggc_image.h"

namespace ggc {

namespace {

typedef unsigned long long u64;

constexpr int FC_THREADS = 256;
constexpr int FC_WORDS = FC_THREADS / WAVE;       // words (of 64 pixels) per block and row: one per wave
constexpr int FC_MASK_ROWS = 16;                  // rows per block of k_fc_mask
constexpr int FC_ROWS = 32;                       // rows per block of k_fc_labels
constexpr int FC_BAND_MAX = 64;

// the bits of word w that lie inside a row of W1 pixels
__device__ __forceinline__ u64 fc_valid(int w, int W1) {
    const int rem = W1 - w * WAVE;
    return rem >= WAVE ? ~0ull : (rem <= 0 ? 0ull : (1ull << rem) - 1ull);
}

// grid (cdiv(NW, 4), cdiv(H1, 16), B), 256 threads: wave k of a block owns word 4 blockIdx.x + k of 16 rows.  A lane's
// column coordinate is computed once; lane r computes the row coordinate of the block's row r and the wave reads it by
// shuffle.  Lanes past W1 compute on the last column (so every read stays inside the working mask) and vote 0.
__global__ void __launch_bounds__(FC_THREADS) k_fc_mask(int H, int W, int H1, int W1, int NW,
                                                        const uint8_t* __restrict__ binary, u64* __restrict__ mbits) {
    const int lane = threadIdx.x & (WAVE - 1), w = blockIdx.x * FC_WORDS + (threadIdx.x >> 6);
    if (w >= NW) return;                                           // the same for every lane of the wave
    const int x = w * WAVE + lane, ya = blockIdx.y * FC_MASK_ROWS;
    int x0, x1, ry0, ry1;
    double wx, rwy;
    half_pixel_coord(min(x, W1 - 1), W, W1, x0, x1, wx);
    half_pixel_coord(min(ya + min(lane, FC_MASK_ROWS - 1), H1 - 1), H, H1, ry0, ry1, rwy);
    const uint8_t* m = binary + (size_t)blockIdx.z * H * W;
    u64* out = mbits + ((size_t)blockIdx.z * H1 + ya) * NW + w;
    const int rows = min(FC_MASK_ROWS, H1 - ya);
    for (int r = 0; r < rows; ++r) {
        const int y0 = __shfl(ry0, r), y1 = __shfl(ry1, r);
        const double wy = __shfl(rwy, r);
        const double m00 = m[(size_t)y0 * W + x0] != 0 ? 1.0 : 0.0, m01 = m[(size_t)y0 * W + x1] != 0 ? 1.0 : 0.0;
        const double m10 = m[(size_t)y1 * W + x0] != 0 ? 1.0 : 0.0, m11 = m[(size_t)y1 * W + x1] != 0 ? 1.0 : 0.0;
        const double v = lerp(lerp(m00, m01, wx), lerp(m10, m11, wx), wy);
        const u64 word = __ballot(x < W1 && v >= 0.5);
        if (lane == 0) out[(size_t)r * NW] = word;
    }
}

// one thread per word of plane M, grid (cdiv(H1 NW, 256), 1, B): E of the words w - 1, w, w + 1 of row y, then
// Hd[y][w] = E dilated horizontally by `band` pixels
__global__ void __launch_bounds__(FC_THREADS) k_fc_hdil(int H1, int W1, int NW, int band, const u64* __restrict__ mbits,
                                                        u64* __restrict__ hdil) {
    const int idx = blockIdx.x * FC_THREADS + threadIdx.x;
    if (idx >= H1 * NW) return;
    const int y = idx / NW, w = idx - y * NW;
    const u64* plane = mbits + (size_t)blockIdx.z * H1 * NW;
    const u64 *ra = plane + (size_t)max(y - 1, 0) * NW, *rb = plane + (size_t)y * NW, *rc = plane + (size_t)min(y + 1, H1 - 1) * NW;
    u64 o[5], a[5];                                                // OR and AND down the three rows, words w - 2 .. w + 2
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int ww = w - 2 + k;
        if (ww < 0 || ww >= NW) { o[k] = 0ull; a[k] = ~0ull; continue; }
        const u64 v0 = ra[ww], v1 = rb[ww], v2 = rc[ww];
        o[k] = v0 | v1 | v2;
        a[k] = (v0 & v1 & v2) | ~fc_valid(ww, W1);
    }
    u64 e[3];                                                      // E of the words w - 1, w, w + 1
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u64 hi = o[k + 1] | (o[k + 1] << 1) | (o[k] >> 63) | (o[k + 1] >> 1) | (o[k + 2] << 63);
        const u64 lo = a[k + 1] & ((a[k + 1] << 1) | (a[k] >> 63)) & ((a[k + 1] >> 1) | (a[k + 2] << 63));
        e[k] = hi & ~lo & fc_valid(w - 1 + k, W1);
    }
    u64 d = e[1];
    for (int s = 1; s <= band && s < WAVE; ++s)
        d |= (e[1] << s) | (e[0] >> (WAVE - s)) | (e[1] >> s) | (e[2] << (WAVE - s));
    if (band >= WAVE) d |= e[0] | e[2];
    hdil[(size_t)blockIdx.z * H1 * NW + idx] = d & fc_valid(w, W1);
}

// four bits -> four bytes of 0 / 1 (bit i lands on bit 8 i: the products i + 7 k are distinct, so nothing carries)
__device__ __forceinline__ uint32_t fc_spread(uint32_t nibble) { return (nibble * 0x00204081u) & 0x01010101u; }

// grid (cdiv(NW, 4), cdiv(H1, 32), B), 256 threads: a strip of 32 rows x 4 words.  hdil == NULL: no band (mask_full only).
// VEC: W1 is a multiple of 16 and both outputs are 16-byte aligned, so 16 pixels are one aligned uint4; else bytes.
template <bool VEC>
__global__ void __launch_bounds__(FC_THREADS) k_fc_labels(int H1, int W1, int NW, int band, const u64* __restrict__ mbits,
                                                          const u64* __restrict__ hdil, uint8_t* __restrict__ labels,
                                                          uint8_t* __restrict__ mask_full) {
    __shared__ u64 s_hd[(FC_ROWS + 2 * FC_BAND_MAX) * FC_WORDS];
    __shared__ u64 s_u[FC_ROWS * FC_WORDS], s_m[FC_ROWS * FC_WORDS];
    const int tid = threadIdx.x, w0 = blockIdx.x * FC_WORDS, ya = blockIdx.y * FC_ROWS;
    const size_t plane = (size_t)blockIdx.z * H1 * NW;
    if (hdil) {
        for (int i = tid; i < (FC_ROWS + 2 * band) * FC_WORDS; i += FC_THREADS) {
            const int y = ya - band + i / FC_WORDS, w = w0 + i % FC_WORDS;
            s_hd[i] = (y >= 0 && y < H1 && w < NW) ? hdil[plane + (size_t)y * NW + w] : 0ull;
        }
        __syncthreads();
    }
    if (tid < FC_ROWS * FC_WORDS) {
        const int r = tid / FC_WORDS, c = tid % FC_WORDS, y = ya + r, w = w0 + c;
        u64 u = 0ull;
        if (hdil)
            for (int k = 0; k <= 2 * band; ++k) u |= s_hd[(r + k) * FC_WORDS + c];
        s_u[tid] = u;
        s_m[tid] = (y < H1 && w < NW) ? mbits[plane + (size_t)y * NW + w] : 0ull;
    }
    __syncthreads();
    const size_t image = (size_t)blockIdx.z * H1 * W1;
    if (VEC) {
        constexpr int CHUNKS = FC_WORDS * 4;                       // 16-pixel chunks per row of the strip
        for (int i = tid; i < FC_ROWS * CHUNKS; i += FC_THREADS) {
            const int r = i / CHUNKS, ch = i % CHUNKS, y = ya + r, x = w0 * WAVE + ch * 16;
            if (y >= H1 || x >= W1) continue;                      // W1 % 16 == 0: a chunk is inside or outside as a whole
            const int sh = (ch & 3) * 16;
            const uint32_t m16 = (uint32_t)(s_m[r * FC_WORDS + ch / 4] >> sh) & 0xFFFFu;
            const uint32_t u16 = (uint32_t)(s_u[r * FC_WORDS + ch / 4] >> sh) & 0xFFFFu;
            uint4 mv, lv;
            mv.x = fc_spread(m16 & 15u);         lv.x = mv.x | (fc_spread(u16 & 15u) << 1);
            mv.y = fc_spread((m16 >> 4) & 15u);  lv.y = mv.y | (fc_spread((u16 >> 4) & 15u) << 1);
            mv.z = fc_spread((m16 >> 8) & 15u);  lv.z = mv.z | (fc_spread((u16 >> 8) & 15u) << 1);
            mv.w = fc_spread(m16 >> 12);         lv.w = mv.w | (fc_spread(u16 >> 12) << 1);
            const size_t o = image + (size_t)y * W1 + x;
            if (labels) *reinterpret_cast<uint4*>(labels + o) = lv;
            if (mask_full) *reinterpret_cast<uint4*>(mask_full + o) = mv;
        }
    } else {
        const int c = tid >> 6, bit = tid & (WAVE - 1), x = (w0 + c) * WAVE + bit;
        if (x >= W1) return;
        for (int r = 0; r < FC_ROWS && ya + r < H1; ++r) {
            const uint8_t mb = (uint8_t)((s_m[r * FC_WORDS + c] >> bit) & 1ull), ub = (uint8_t)((s_u[r * FC_WORDS + c] >> bit) & 1ull);
            const size_t o = image + (size_t)(ya + r) * W1 + x;
            if (labels) labels[o] = (uint8_t)(mb | (ub << 1));
            if (mask_full) mask_full[o] = mb;
        }
    }
}

} // namespace

} // namespace ggc

using namespace ggc;

extern "C" int ggc_lift_labels(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* binary, int H1, int W1,
                               int band, uint8_t* labels_full, uint8_t* mask_full) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H1 >= H && W1 >= W && H1 <= 32768 && W1 <= 32768,
                GGC_E_SHAPE, "bad shape B=%d H=%d W=%d H1=%d W1=%d", B, H, W, H1, W1);
    GGC_REQUIRE(ctx, labels_full || mask_full, GGC_E_INVALID_ARG, "null pointer: no output asked for");
    GGC_REQUIRE(ctx, B == 0 || binary, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, band >= 0 && band <= FC_BAND_MAX, GGC_E_INVALID_ARG, "lift band %d outside 0..64", band);
    if (B == 0) return GGC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    const int NW = cdiv(W1, WAVE);
    const size_t words = (size_t)B * H1 * NW;
    u64 *mbits = nullptr, *hdil = nullptr;
    if (!carve_scratch(ctx, S_FULLCUT, [&](Carve& c) {
            mbits = c.take<u64>(words);
            if (labels_full) hdil = c.take<u64>(words);
        }))
        return GGC_E_OOM;
    ProfScope prof(ctx, st, "lift_labels");
    hipLaunchKernelGGL(k_fc_mask, dim3(cdiv(NW, FC_WORDS), cdiv(H1, FC_MASK_ROWS), B), dim3(FC_THREADS), 0, st, H, W, H1, W1,
                       NW, binary, mbits);
    if (labels_full)
        hipLaunchKernelGGL(k_fc_hdil, dim3(cdiv((int64_t)H1 * NW, FC_THREADS), 1, B), dim3(FC_THREADS), 0, st, H1, W1, NW, band,
                           mbits, hdil);
    const dim3 grid(cdiv(NW, FC_WORDS), cdiv(H1, FC_ROWS), B);
    const bool vec = W1 % 16 == 0 && (reinterpret_cast<uintptr_t>(labels_full) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(mask_full) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_fc_labels<true>, grid, dim3(FC_THREADS), 0, st, H1, W1, NW, band, mbits, hdil, labels_full, mask_full);
    else
        hipLaunchKernelGGL(k_fc_labels<false>, grid, dim3(FC_THREADS), 0, st, H1, W1, NW, band, mbits, hdil, labels_full, mask_full);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
