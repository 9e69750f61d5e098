// ggc_wand.hip — H5: the magic wand.  A seed selects the pixels whose colour is within a tolerance of the seed's own and that
// are connected to it through such pixels (connectivity 4 or 8), or every such pixel (connectivity 0, "select similar").
// include/ggc.h states the definition; the per-pixel rule is ggc_wand.h; DESIGN.md §5.30 has the schedule and the bytes.
//
// The host reads the seeds back, drops those outside their image and uploads a table of the live ones in seed order;
// k_wand_refs fills in their reference sums.  Then
//   contiguous    the live seeds go through in passes of S (as many as keep the parent maps within 1 GiB, at least one;
//                 GGC_WAND_SEEDS_PER_PASS fixes S).  A pass labels one plane per seed with the union-find of ggc_ccl.h over the
//                 flat index i = j P + p, seed j of the pass, pixel p: k_wand_init (match from bgr and the seed's sums, no
//                 predicate plane), k_wand_merge (joined(q) = the sign of the parent plane), k_wand_compress.  k_wand_decide
//                 then runs over the pixels of the images that own a seed of the pass, walks that image's seeds of the pass
//                 from last to first and notes the first whose plane has root(p) == root(seed pixel) in a one-byte decision
//                 plane.  Passes run in seed order, so a later one overwrites an earlier one: the image's last seed wins
//                 whatever S is.  k_wand_emit writes mask, select and counts from the decision plane.
//   similar       k_wand_similar: one streaming launch, the same walk on match alone, straight to the outputs.
// counts are added per block in LDS and issued as two integer atomics per block and image.  No float anywhere.
#include "ggc_internal.h"
#include "ggc_ccl.h"
#include "ggc_wand.h"
#include <algorithm>
#include <climits>

namespace ggc {
namespace {

constexpr int WD_THREADS = 256;
constexpr size_t WD_MAPS_MAX = size_t(1) << 30;   // bytes of parent maps of one pass, unless one seed alone takes more
constexpr int64_t WD_FLAT_MAX = int64_t(1) << 38; // S P of a pass, whatever the knob says: the labelling grid stays below 2^31 blocks
constexpr uint8_t WD_NONE = 0, WD_BG = 1, WD_FG = 2;   // the decision plane

struct WDims { int B, H, W, P, n, n2, reach; };   // n = sample, n2 = n n, reach = n2 tolerance
struct WandSpan { int32_t image, j0, j1; };       // seeds j0 .. j1 - 1 of the table it comes with belong to `image`

__global__ void __launch_bounds__(WD_THREADS) k_wand_refs(WDims d, int n_seeds, const uint8_t* __restrict__ bgr, WandSeed* seeds) {
    const int k = blockIdx.x * WD_THREADS + threadIdx.x;
    if (k >= n_seeds) return;
    const WandSeed s = seeds[k];
    int32_t ref[3];
    wand_ref_sums(bgr + 3 * (size_t)s.image * d.P, d.H, d.W, s.pixel / d.W, s.pixel % d.W, d.n, ref);
    seeds[k].ref[0] = ref[0]; seeds[k].ref[1] = ref[1]; seeds[k].ref[2] = ref[2];
}

// The labelling kernels run over the flat index i = j P + p: seed j of the pass, pixel p.  A wave covers 64 consecutive i: it
// may straddle two rows, two planes or two images; same_left is false at x == 0, so no run crosses any of them.
__global__ void __launch_bounds__(WD_THREADS) k_wand_init(WDims d, int S, const WandSeed* __restrict__ seeds,
                                                          const uint8_t* __restrict__ bgr, int32_t* __restrict__ parent) {
    const size_t n = (size_t)S * d.P;
    const size_t i = (size_t)blockIdx.x * WD_THREADS + threadIdx.x;
    bool on = false, same_left = false;
    int p = 0;
    if (i < n) {
        const size_t j = i / d.P;
        p = (int)(i - j * d.P);
        const WandSeed s = seeds[j];
        const uint8_t* px = bgr + 3 * ((size_t)s.image * d.P + p);
        on = wand_match(px, s.ref, d.n2, d.reach);
        same_left = on && (p % d.W) > 0 && wand_match(px - 3, s.ref, d.n2, d.reach);
    }
    const int first = ccl_run_first(on, same_left, p);
    if (i < n) parent[i] = on ? first : -1;
}

template <int CONN>
__global__ void __launch_bounds__(WD_THREADS) k_wand_merge(WDims d, int S, int32_t* __restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * WD_THREADS + threadIdx.x;
    if (i >= (size_t)S * d.P) return;
    const size_t base = (i / d.P) * d.P;
    int32_t* par = parent + base;
    const int p = (int)(i - base), x = p % d.W;
    if (par[p] < 0) return;
    ccl_merge_pixel<CONN>(par, p, x, p >= d.W, d.W, i, [par](int q) { return par[q] >= 0; });
}

__global__ void __launch_bounds__(WD_THREADS) k_wand_compress(WDims d, int S, int32_t* __restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * WD_THREADS + threadIdx.x;
    if (i >= (size_t)S * d.P || parent[i] < 0) return;
    const size_t base = (i / d.P) * d.P;
    ccl_compress(parent + base, (int)(i - base));
}

// grid (blocks, spans of the pass): the pixels of one image that owns seeds of this pass
__global__ void __launch_bounds__(WD_THREADS) k_wand_decide(WDims d, const WandSpan* __restrict__ spans,
                                                            const WandSeed* __restrict__ seeds, const int32_t* __restrict__ parent,
                                                            uint8_t* __restrict__ decision) {
    const WandSpan sp = spans[blockIdx.y];
    uint8_t* dec = decision + (size_t)sp.image * d.P;
    for (int64_t p = (int64_t)blockIdx.x * WD_THREADS + threadIdx.x; p < d.P; p += (int64_t)gridDim.x * WD_THREADS)
        for (int j = sp.j1 - 1; j >= sp.j0; --j) {
            const int32_t* par = parent + (size_t)j * d.P;
            const int root = par[seeds[j].pixel];                               // negative: the seed's own pixel does not match
            if (root >= 0 && par[p] == root) { dec[p] = seeds[j].label ? WD_FG : WD_BG; break; }
        }
}

// The outputs of image blockIdx.y from decide(p) in {WD_NONE, WD_BG, WD_FG}, by every thread of the block: mask where decided,
// select everywhere, counts per block in LDS and then two integer atomics.
template <class Decide>
__device__ __forceinline__ void wand_emit(const WDims& d, Decide decide, uint8_t* __restrict__ mask, uint8_t* __restrict__ select,
                                          int32_t* __restrict__ counts) {
    __shared__ int s[2][WD_THREADS];
    const size_t base = (size_t)blockIdx.y * d.P;
    int v[2] = {0, 0};
    for (int64_t p = (int64_t)blockIdx.x * WD_THREADS + threadIdx.x; p < d.P; p += (int64_t)gridDim.x * WD_THREADS) {
        const uint8_t dec = decide((int)p);
        if (select) select[base + p] = dec == WD_FG ? 255 : 0;
        if (dec == WD_NONE) continue;
        if (mask) mask[base + p] = dec == WD_FG ? GGC_FGD : GGC_BGD;
        v[dec == WD_FG ? 0 : 1] += 1;
    }
    if (!counts) return;                                                        // uniform
    s[0][threadIdx.x] = v[0]; s[1][threadIdx.x] = v[1];
    __syncthreads();
    for (int h = WD_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { s[0][threadIdx.x] += s[0][threadIdx.x + h]; s[1][threadIdx.x] += s[1][threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x < 2 && s[threadIdx.x][0]) atomicAdd(&counts[(size_t)blockIdx.y * 2 + threadIdx.x], s[threadIdx.x][0]);
}

// grid (blocks, B)
__global__ void __launch_bounds__(WD_THREADS) k_wand_emit(WDims d, const uint8_t* __restrict__ decision, uint8_t* __restrict__ mask,
                                                          uint8_t* __restrict__ select, int32_t* __restrict__ counts) {
    const uint8_t* dec = decision + (size_t)blockIdx.y * d.P;
    wand_emit(d, [dec](int p) { return dec[p]; }, mask, select, counts);
}

// grid (blocks, B); spans[b] = the live seeds of image b
__global__ void __launch_bounds__(WD_THREADS) k_wand_similar(WDims d, const WandSpan* __restrict__ spans,
                                                             const WandSeed* __restrict__ seeds, const uint8_t* __restrict__ bgr,
                                                             uint8_t* __restrict__ mask, uint8_t* __restrict__ select,
                                                             int32_t* __restrict__ counts) {
    const WandSpan sp = spans[blockIdx.y];
    const uint8_t* img = bgr + 3 * (size_t)blockIdx.y * d.P;
    wand_emit(d, [&](int p) -> uint8_t {
        for (int j = sp.j1 - 1; j >= sp.j0; --j)
            if (wand_match(img + 3 * (size_t)p, seeds[j].ref, d.n2, d.reach)) return seeds[j].label ? WD_FG : WD_BG;
        return WD_NONE;
    }, mask, select, counts);
}

// seeds of table[lo .. hi) grouped by image (the table is in image order), indices relative to lo
void spans_of(const std::vector<WandSeed>& table, int lo, int hi, std::vector<WandSpan>& out) {
    for (int k = lo; k < hi;) {
        int e = k + 1;
        while (e < hi && table[e].image == table[k].image) ++e;
        out.push_back({table[k].image, k - lo, e - lo});
        k = e;
    }
}

} // namespace
} // namespace ggc

extern "C" int ggc_wand_select(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const int32_t* seeds,
                               const int32_t* seed_ptr, int tolerance, int connectivity, int sample, uint8_t* mask,
                               uint8_t* select, int32_t* counts) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (int64_t)H * W <= INT_MAX, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d (each 1..65535, H*W within int32)", B, H, W);
    GGC_REQUIRE(ctx, tolerance >= 0 && tolerance <= 255, GGC_E_INVALID_ARG, "wand tolerance %d outside 0..255", tolerance);
    GGC_REQUIRE(ctx, connectivity == 0 || connectivity == 4 || connectivity == 8, GGC_E_INVALID_ARG,
                "wand connectivity %d is not 4, 8 or 0 (not contiguous)", connectivity);
    GGC_REQUIRE(ctx, sample == 1 || sample == 3 || sample == 5, GGC_E_INVALID_ARG, "wand sample %d is not 1, 3 or 5", sample);
    GGC_REQUIRE(ctx, bgr && seed_ptr, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, mask || select || counts, GGC_E_INVALID_ARG, "no output requested");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::vector<int32_t> sp, hs;
    int rc = read_offsets(ctx, st, seed_ptr, B, "seed_ptr", "image", 0, sp);
    if (rc) return rc;
    const int K = sp[B];
    if (K == 0) return GGC_OK;
    GGC_REQUIRE(ctx, seeds, GGC_E_INVALID_ARG, "null seeds with %d seeds", K);
    GGC_REQUIRE(ctx, K <= INT_MAX / 3, GGC_E_INVALID_ARG, "%d seeds are too many", K);
    if ((rc = read_i32(ctx, st, seeds, 3 * K, hs))) return rc;

    const WDims d{B, H, W, H * W, sample, sample * sample, sample * sample * tolerance};
    std::vector<WandSeed> table;                                               // the live seeds, in seed order
    for (int b = 0; b < B; ++b)
        for (int k = sp[b]; k < sp[b + 1]; ++k) {
            const int r = hs[3 * (size_t)k], c = hs[3 * (size_t)k + 1];
            if (r < 0 || r >= H || c < 0 || c >= W) continue;                  // outside its image: ignored
            table.push_back({b, r * W + c, hs[3 * (size_t)k + 2] != 0, {0, 0, 0}});
        }
    const int n_live = (int)table.size();
    const size_t BP = (size_t)B * d.P;
    if (counts) GGC_HIP(ctx, hipMemsetAsync(counts, 0, sizeof(int32_t) * 2 * (size_t)B, st));
    if (n_live == 0) {                                                         // nothing decides anything
        if (select) GGC_HIP(ctx, hipMemsetAsync(select, 0, BP, st));
        return GGC_OK;
    }

    // the passes, and the spans of every pass in one table
    const bool contiguous = connectivity != 0;
    int S = knobs().wand_seeds_per_pass;
    if (S == 0) S = (int)std::max<size_t>(1, WD_MAPS_MAX / (sizeof(int32_t) * (size_t)d.P));
    S = (int)std::min<int64_t>(std::min(S, n_live), std::max<int64_t>(1, WD_FLAT_MAX / d.P));
    std::vector<WandSpan> spans;
    std::vector<int> pass_span0;                                               // pass k owns spans[pass_span0[k] .. pass_span0[k+1])
    if (contiguous) {
        for (int s0 = 0; s0 < n_live; s0 += S) {
            pass_span0.push_back((int)spans.size());
            spans_of(table, s0, std::min(n_live, s0 + S), spans);
        }
        pass_span0.push_back((int)spans.size());
    } else {
        int k = 0;
        for (int b = 0; b < B; ++b) {
            const int k0 = k;
            while (k < n_live && table[k].image == b) ++k;
            spans.push_back({b, k0, k});
        }
    }
    static_assert(sizeof(WandSeed) == 24 && sizeof(WandSpan) == 12, "the upload is packed int32");
    const size_t seed_words = 6 * (size_t)n_live, span_words = 3 * spans.size();
    std::vector<int32_t> up(seed_words + span_words);
    std::memcpy(up.data(), table.data(), sizeof(int32_t) * seed_words);
    std::memcpy(up.data() + seed_words, spans.data(), sizeof(int32_t) * span_words);

    // 4 bytes per pixel per seed of a pass and one per pixel of the batch (contiguous only), 24 per seed, 12 per span
    int32_t *parent = nullptr, *dev_up = nullptr;
    uint8_t* decision = nullptr;
    if (!carve_scratch(ctx, S_WAND, [&](Carve& c) {
            parent = c.take<int32_t>(contiguous ? (size_t)S * d.P : 0);
            decision = c.take<uint8_t>(contiguous ? BP : 0);
            dev_up = c.take<int32_t>(up.size());
        }))
        return GGC_E_OOM;
    WandSeed* dev_seeds = reinterpret_cast<WandSeed*>(dev_up);
    const WandSpan* dev_spans = reinterpret_cast<const WandSpan*>(dev_up + seed_words);
    GGC_HIP(ctx, hipMemcpyAsync(dev_up, up.data(), sizeof(int32_t) * up.size(), hipMemcpyHostToDevice, st));
    if (contiguous) GGC_HIP(ctx, hipMemsetAsync(decision, WD_NONE, BP, st));
    GGC_HIP(ctx, hipStreamSynchronize(st));                                    // `up` is pageable: the copy has left it

    const dim3 blk(WD_THREADS);
    const auto px_blocks = [&](int images) {                                   // blocks per image of a grid-stride launch
        return std::min(cdiv(d.P, WD_THREADS), std::max(8, cdiv(64 * (int64_t)std::max(ctx->n_cu, 1), images)));
    };
    {
        ProfScope prof(ctx, st, "wand_refs");
        hipLaunchKernelGGL(k_wand_refs, dim3(cdiv(n_live, WD_THREADS)), blk, 0, st, d, n_live, bgr, dev_seeds);
    }
    GGC_LAUNCH_CHECK(ctx);
    if (!contiguous) {
        ProfScope prof(ctx, st, "wand_similar");
        hipLaunchKernelGGL(k_wand_similar, dim3(px_blocks(B), B), blk, 0, st, d, dev_spans, dev_seeds, bgr, mask, select, counts);
        GGC_LAUNCH_CHECK(ctx);
        return GGC_OK;
    }
    for (int s0 = 0, k = 0; s0 < n_live; s0 += S, ++k) {
        const int Sp = std::min(S, n_live - s0), n_spans = pass_span0[k + 1] - pass_span0[k];
        const dim3 g_lab(cdiv((int64_t)Sp * d.P, WD_THREADS));
        {
            ProfScope prof(ctx, st, "wand_init");
            hipLaunchKernelGGL(k_wand_init, g_lab, blk, 0, st, d, Sp, dev_seeds + s0, bgr, parent);
        }
        {
            ProfScope prof(ctx, st, "wand_merge");
            if (connectivity == 4) hipLaunchKernelGGL(k_wand_merge<4>, g_lab, blk, 0, st, d, Sp, parent);
            else hipLaunchKernelGGL(k_wand_merge<8>, g_lab, blk, 0, st, d, Sp, parent);
        }
        {
            ProfScope prof(ctx, st, "wand_compress");
            hipLaunchKernelGGL(k_wand_compress, g_lab, blk, 0, st, d, Sp, parent);
        }
        {
            ProfScope prof(ctx, st, "wand_decide");
            hipLaunchKernelGGL(k_wand_decide, dim3(px_blocks(n_spans), n_spans), blk, 0, st, d, dev_spans + pass_span0[k],
                               dev_seeds + s0, parent, decision);
        }
        GGC_LAUNCH_CHECK(ctx);
    }
    {
        ProfScope prof(ctx, st, "wand_emit");
        hipLaunchKernelGGL(k_wand_emit, dim3(px_blocks(B), B), blk, 0, st, d, decision, mask, select, counts);
    }
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
