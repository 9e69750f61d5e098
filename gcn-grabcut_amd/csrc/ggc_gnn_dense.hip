// ggc_gnn_dense.hip — the dense per-node and per-graph algebra that more than one trimap network launches.
//
// Kernel map:
//   k_gemm<D, MODE>   out[N,D] = op(A)[N,D] @ W^T on f32 MFMA (v_mfma_f32_32x32x2_f32); the modes (GemmArgs, ggc_gnn.h)
//                     are ResGCNNet's GCN XW / SAGE / head products, the plain product of GCNTrimapNet and GATTrimapNet
//                     and GATTrimapNet's head
//   k_graph_ctx<D>    per-graph softmax readout, compress/expand MLP (ResGCNNet, GATTrimapNet)
//
// The build is not relocatable device code, so a kernel is launched from the file that defines it: the launchers are
// declared in ggc_gnn.h and every (D, MODE) the library uses is instantiated under its launcher here.
#include "ggc_gnn.h"
#include <cmath>

namespace ggc {

// ---------------------------------------------------------------- MFMA GEMM
// out[N,D] = op(A)[N,D] @ W^T, f32 in / f32 accumulate on v_mfma_f32_32x32x2_f32.
// A block is 4 waves; each wave owns 32 rows x D columns (T = D/32 accumulator
// tiles).  The k index is permuted so that lane half hk = lane>>5 covers
// k in [hk*D/2, (hk+1)*D/2): each lane then reads one contiguous half-row of A
// (float4 loads) and W is pre-packed on the host as Wp[s/4][t][lane][s%4] =
// W[32t + (lane&31)][hk*D/2 + s], staged once per block into LDS and read with
// conflict-free ds_read_b128.  The modes and their arguments (GemmArgs) are listed in ggc_gnn.h.
template <int D, int MODE>
__global__ void __launch_bounds__(256) k_gemm(int N, GemmArgs g) {
    constexpr int T = D / 32, KH = D / 2;
    extern __shared__ float4 smem4[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hk = lane >> 5, li = lane & 31;
    const int r0 = (blockIdx.x * 4 + wave) * 32;
    const int row = min(r0 + li, N - 1);

    f32x16 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    constexpr int PHASES = (MODE == 1) ? 2 : 1;
    if constexpr (D <= 128) {
#pragma unroll
    for (int ph = 0; ph < PHASES; ++ph) {
        const float* Wp = ph ? g.Wp2 : g.Wp1;
        const float* A = ph ? g.A2 : g.A1;
        // the wave's rows are requested first: their latency runs under the staging of W
        float4 av[KH / 4];
        {
            const float4* ap = reinterpret_cast<const float4*>(A + (size_t)row * D + hk * KH);
#pragma unroll
            for (int q = 0; q < KH / 4; ++q) av[q] = ap[q];
        }
        if (ph) __syncthreads();
        {   // all D * D / 1024 loads of a thread in flight at once (rolled, the loop paid one memory round trip per 4 KB: 17 k cycles at D = 128)
            float4 wv[D * D / 1024];
#pragma unroll
            for (int q = 0; q < D * D / 1024; ++q) wv[q] = reinterpret_cast<const float4*>(Wp)[tid + q * 256];
#pragma unroll
            for (int q = 0; q < D * D / 1024; ++q) smem4[tid + q * 256] = wv[q];
        }
        __syncthreads();

        float a[KH];
#pragma unroll
        for (int q = 0; q < KH / 4; ++q) {
            const float4 v = av[q];
            a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
        }
        if (MODE == 2 || MODE == 4) {
            const float* gv = g.gvec + (size_t)g.batch[row] * D + hk * KH;
#pragma unroll
            for (int s = 0; s < KH; ++s) a[s] *= gv[s];
        }
        if (MODE == 0 || MODE == 2) {
            float s1 = 0.0f;
#pragma unroll
            for (int s = 0; s < KH; ++s) s1 += a[s];
            s1 += __shfl_xor(s1, 32, 64);
            const int dt = g.Dt > 0 ? g.Dt : D, nv = min(max(dt - hk * KH, 0), KH);   // this lane's channels below the true width
            const float mean = s1 / (float)dt;
            float s2 = 0.0f;
#pragma unroll
            for (int s = 0; s < KH; ++s) { const float d = a[s] - mean; s2 += (s < nv) ? d * d : 0.0f; }
            s2 += __shfl_xor(s2, 32, 64);
            const float rstd = 1.0f / sqrtf(s2 / (float)dt + 1e-5f);
            const float* lw = g.ln_w + hk * KH;
            const float* lb = g.ln_b + hk * KH;
#pragma unroll
            for (int s = 0; s < KH; ++s) a[s] = (a[s] - mean) * rstd * lw[s] + lb[s];
        }
        // Consecutive MFMAs go to different accumulators (the T column tiles of one k step); each accumulator still sees its
        // k steps in the same order.  (Per-wave phase stamps of a since-removed trace build, DESIGN.md "second stamp build":
        // the MFMA loops of the two waves of a SIMD never overlap, in this order or with the four k steps of a B fragment
        // back to back on one accumulator, and the other wave's LayerNorm crawls meanwhile — the f32 MFMA runs at the vector
        // rate and leaves the SIMD's vector issue little room.)
#pragma unroll
        for (int s4 = 0; s4 < KH / 4; ++s4) {
            float bq[T][4];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float4 b = smem4[(s4 * T + t) * 64 + lane];
                bq[t][0] = b.x; bq[t][1] = b.y; bq[t][2] = b.z; bq[t][3] = b.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < T; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * s4 + j], bq[t][j], acc[t], 0, 0, 0);
        }
    }
    } else {
        // D > 128: the packed W (100-256 KiB) no longer fits the LDS whole, and a lane cannot hold its KH-float half-row
        // beside T accumulators.  W is staged KC k-steps at a time (its packed form is k-major, so a chunk is contiguous)
        // and the row is read chunk by chunk; the LayerNorm statistics take a pass over the row first.  Every output
        // still sees its products in the same k order.
        constexpr int KC = 16, NCH = KH / KC, WQ = KC * T / 16;           // k-steps per chunk, chunks, float4 per thread
        static_assert(KH % KC == 0, "KH must be a multiple of the chunk");
        const float* gv = nullptr;
        if (MODE == 2 || MODE == 4) gv = g.gvec + (size_t)g.batch[row] * D + hk * KH;
        float mean = 0.0f, rstd = 1.0f;
        const int dt = g.Dt > 0 ? g.Dt : D, nv = min(max(dt - hk * KH, 0), KH);
        if (MODE == 0 || MODE == 2) {
            const float4* ar4 = reinterpret_cast<const float4*>(g.A1 + (size_t)row * D + hk * KH);
            const float4* gv4 = reinterpret_cast<const float4*>(gv);
            auto row4 = [&](int q) {                           // four channels of the (gated) row, in channel order
                float4 v = ar4[q];
                if (MODE == 2) { const float4 u = gv4[q]; v.x *= u.x; v.y *= u.y; v.z *= u.z; v.w *= u.w; }
                return v;
            };
            float s1 = 0.0f;
#pragma unroll 2
            for (int q = 0; q < KH / 4; ++q) { const float4 v = row4(q); s1 += v.x; s1 += v.y; s1 += v.z; s1 += v.w; }
            s1 += __shfl_xor(s1, 32, 64);
            mean = s1 / (float)dt;
            float s2 = 0.0f;
#pragma unroll 2
            for (int q = 0; q < KH / 4; ++q) {
                const float4 v = row4(q);
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) { const float d = e[u] - mean; s2 += (4 * q + u < nv) ? d * d : 0.0f; }
            }
            s2 += __shfl_xor(s2, 32, 64);
            rstd = 1.0f / sqrtf(s2 / (float)dt + 1e-5f);
        }
        for (int ph = 0; ph < PHASES; ++ph) {
            const float4* Wp4 = reinterpret_cast<const float4*>(ph ? g.Wp2 : g.Wp1);
            const float4* ap = reinterpret_cast<const float4*>((ph ? g.A2 : g.A1) + (size_t)row * D + hk * KH);
            for (int c = 0; c < NCH; ++c) {
                float4 av[KC / 4];
#pragma unroll
                for (int q = 0; q < KC / 4; ++q) av[q] = ap[c * (KC / 4) + q];
                __syncthreads();                                            // the previous chunk has been read
#pragma unroll
                for (int q = 0; q < WQ; ++q) smem4[tid + q * 256] = Wp4[(size_t)c * WQ * 256 + tid + q * 256];
                __syncthreads();
                float a[KC];
#pragma unroll
                for (int q = 0; q < KC / 4; ++q) {
                    const float4 v = av[q];
                    a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
                }
                if (MODE == 2 || MODE == 4) {
#pragma unroll
                    for (int s = 0; s < KC; ++s) a[s] *= gv[c * KC + s];
                }
                if (MODE == 0 || MODE == 2) {
                    const float* lw = g.ln_w + hk * KH + c * KC;
                    const float* lb = g.ln_b + hk * KH + c * KC;
#pragma unroll
                    for (int s = 0; s < KC; ++s) a[s] = (a[s] - mean) * rstd * lw[s] + lb[s];
                }
#pragma unroll
                for (int s4 = 0; s4 < KC / 4; ++s4) {
                    float bq[T][4];
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const float4 b = smem4[(s4 * T + t) * 64 + lane];
                        bq[t][0] = b.x; bq[t][1] = b.y; bq[t][2] = b.z; bq[t][3] = b.w;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int t = 0; t < T; ++t)
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * s4 + j], bq[t][j], acc[t], 0, 0, 0);
                }
            }
        }
    }

    // C/D layout: col = 32 t + (lane & 31), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if (MODE == 3) {                 // plain product (GCNTrimapNet: no prologue norm), optionally accumulated
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int grow = r0 + (r & 3) + 8 * (r >> 2) + 4 * hk;
            if (grow < N) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    float* o = g.out + (size_t)grow * D + 32 * t + li;
                    *o = g.accumulate ? *o + acc[t][r] : acc[t][r];
                }
            }
        }
    } else if (MODE == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int grow = r0 + (r & 3) + 8 * (r >> 2) + 4 * hk;
            if (grow < N) {
#pragma unroll
                for (int t = 0; t < T; ++t) g.out[(size_t)grow * D + 32 * t + li] = acc[t][r];
            }
        }
    } else if (MODE == 1) {
        float bias[T], lw[T], lb[T];
#pragma unroll
        for (int t = 0; t < T; ++t) { bias[t] = g.bias[32 * t + li]; lw[t] = g.ep_w[32 * t + li]; lb[t] = g.ep_b[32 * t + li]; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float s1 = 0.0f;
#pragma unroll
            for (int t = 0; t < T; ++t) { acc[t][r] += bias[t]; s1 += acc[t][r]; }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) s1 += __shfl_xor(s1, o, 64);
            const int dt = g.Dt > 0 ? g.Dt : D;
            const float mean = s1 / (float)dt;
            float s2 = 0.0f;
#pragma unroll
            for (int t = 0; t < T; ++t) { const float d = acc[t][r] - mean; s2 += (32 * t + li < dt) ? d * d : 0.0f; }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
            const float rstd = 1.0f / sqrtf(s2 / (float)dt + 1e-5f);
            const int grow = r0 + (r & 3) + 8 * (r >> 2) + 4 * hk;
            if (grow < N) {
#pragma unroll
                for (int t = 0; t < T; ++t)
                    g.out[(size_t)grow * D + 32 * t + li] = gelu_f((acc[t][r] - mean) * rstd * lw[t] + lb[t]);
            }
        }
    } else {
        float bias[T], hw[N_CLS][T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            bias[t] = g.bias[32 * t + li];
#pragma unroll
            for (int c = 0; c < N_CLS; ++c) hw[c][t] = g.ep_w[c * D + 32 * t + li];
        }
        const float hb0 = g.ep_b[0], hb1 = g.ep_b[1], hb2 = g.ep_b[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float p[N_CLS] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float v = gelu_f(acc[t][r] + bias[t]);
#pragma unroll
                for (int c = 0; c < N_CLS; ++c) p[c] += v * hw[c][t];
            }
#pragma unroll
            for (int c = 0; c < N_CLS; ++c)
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) p[c] += __shfl_xor(p[c], o, 64);
            const int grow = r0 + (r & 3) + 8 * (r >> 2) + 4 * hk;
            if (li == 0 && grow < N) {
                const float l0 = p[0] + hb0, l1 = p[1] + hb1, l2 = p[2] + hb2;
                if (g.out) { g.out[(size_t)grow * 3 + 0] = l0; g.out[(size_t)grow * 3 + 1] = l1; g.out[(size_t)grow * 3 + 2] = l2; }
                if (g.out2) {
                    const float mx = fmaxf(l0, fmaxf(l1, l2));
                    const float e0 = ggc_expf(l0 - mx), e1 = ggc_expf(l1 - mx), e2 = ggc_expf(l2 - mx);
                    const float s = (e0 + e1) + e2;
                    g.out2[(size_t)grow * 3 + 0] = e0 / s; g.out2[(size_t)grow * 3 + 1] = e1 / s; g.out2[(size_t)grow * 3 + 2] = e2 / s;
                }
            }
        }
    }
}

template <int D, int MODE>
int launch_gemm(ggc_ctx* ctx, hipStream_t st, int N, const GemmArgs& a) {
    static DeviceOnce attr_set;                    // per device; contexts may live on other host threads
    // D > 128 stages W in chunks of 16 k-steps (k_gemm): T * 4 KiB
    const size_t lds = D <= 128 ? (size_t)D * D * sizeof(float) : (size_t)(D / 32) * 4096;
    if (attr_set.need(ctx->device) && lds > 48 * 1024) {
        GGC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm<D, MODE>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set.done(ctx->device);
    }
    ProfScope prof(ctx, st, MODE == 0 ? "gcn_gemm" : MODE == 1 ? "sage_gemm" : (MODE == 2 || MODE == 4) ? "head_gemm" : "plain_gemm");
    hipLaunchKernelGGL((k_gemm<D, MODE>), dim3(cdiv(N, 128)), dim3(256), lds, st, N, a);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

#define GGC_GEMM(D, MODE) template int launch_gemm<D, MODE>(ggc_ctx*, hipStream_t, int, const GemmArgs&);
#define GGC_GEMM_RESGCN(D) GGC_GEMM(D, 0) GGC_GEMM(D, 1) GGC_GEMM(D, 2)
// ResGCNNet: LayerNorm + XW of a GCN layer (0), SAGE (1), fuse + head (2) at each of its padded widths
GGC_GEMM_RESGCN(32) GGC_GEMM_RESGCN(64) GGC_GEMM_RESGCN(96) GGC_GEMM_RESGCN(128)
GGC_GEMM_RESGCN(160) GGC_GEMM_RESGCN(192) GGC_GEMM_RESGCN(224) GGC_GEMM_RESGCN(256)
// plain product: GCNTrimapNet (32, 64, 96, 128) and GATTrimapNet (32, 64, 128, 256)
GGC_GEMM(32, 3) GGC_GEMM(64, 3) GGC_GEMM(96, 3) GGC_GEMM(128, 3) GGC_GEMM(256, 3)
// GATTrimapNet: head without the LayerNorm
GGC_GEMM(32, 4) GGC_GEMM(64, 4) GGC_GEMM(128, 4) GGC_GEMM(256, 4)
#undef GGC_GEMM_RESGCN
#undef GGC_GEMM

// --------------------------------------------------------- per-graph readout
template <int D>
__global__ void __launch_bounds__(256) k_graph_ctx(const int32_t* __restrict__ node_ptr,
                                                   const float* __restrict__ score,
                                                   const float* __restrict__ hjk, CtxW w,
                                                   float* __restrict__ gvec) {
    constexpr int Dh = D / 2;
    constexpr int NG = 256 / D;  // column groups (D <= 128 -> >= 2; above 128 one, threads tid >= D add nothing)
    __shared__ float red[256];
    __shared__ float gsum[D];
    __shared__ float cbuf[Dh];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int beg = node_ptr[g], end = node_ptr[g + 1];
    float m = -INFINITY;
    for (int i = beg + tid; i < end; i += 256) m = fmaxf(m, score[i]);
    red[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]); __syncthreads(); }
    m = red[0];
    __syncthreads();
    float s = 0.0f;
    for (int i = beg + tid; i < end; i += 256) s += ggc_expf(score[i] - m);
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float tot = red[0] + 1e-12f;  // model.py:108
    __syncthreads();
    const int d = tid % D, grp = tid / D;
    float acc = 0.0f;
    if (grp < NG)
        for (int i = beg + grp; i < end; i += NG) acc += (ggc_expf(score[i] - m) / tot) * hjk[(size_t)i * D + d];
    red[tid] = (grp < NG) ? acc : 0.0f;
    __syncthreads();
    if (tid < D) {
        float v = 0.0f;
        for (int q = 0; q < NG; ++q) v += red[q * D + tid];
        gsum[tid] = v;
    }
    __syncthreads();
    if (tid < Dh) {
        float a = 0.0f;
        for (int k = 0; k < D; ++k) a += gsum[k] * w.wcT[k * Dh + tid];
        a += w.bc[tid];
        cbuf[tid] = a > 0.0f ? a : 0.0f;
    }
    __syncthreads();
    if (tid < D) {
        float a = 0.0f;
        for (int k = 0; k < Dh; ++k) a += cbuf[k] * w.weT[k * D + tid];
        gvec[(size_t)g * D + tid] = sigmoid_f(a + w.be[tid]);
    }
}

template <int D>
int launch_graph_ctx(ggc_ctx* ctx, hipStream_t st, int G, const int32_t* node_ptr, const float* score, const float* hjk,
                     const CtxW& w, float* gvec) {
    hipLaunchKernelGGL((k_graph_ctx<D>), dim3(G), dim3(256), 0, st, node_ptr, score, hjk, w, gvec);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

#define GGC_CTX(D) template int launch_graph_ctx<D>(ggc_ctx*, hipStream_t, int, const int32_t*, const float*, const float*, const CtxW&, float*);
GGC_CTX(32) GGC_CTX(64) GGC_CTX(128) GGC_CTX(256)       // ResGCNNet and GATTrimapNet
GGC_CTX(96) GGC_CTX(160) GGC_CTX(192) GGC_CTX(224)      // ResGCNNet alone
#undef GGC_CTX

} // namespace ggc
