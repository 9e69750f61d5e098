
// ggc_gat.hip — GATTrimapNet (reference model.py:323-414; SURVEY.md section 8(f), last rank): GATv2 attention with edge features.
//   h0 = GELU(LN(Linear(BN(x))));  skip = skip_proj(h0)
//   5 x { GATv2Conv(h) -> LN -> GELU -> EdgeInjectionLayer }   ;   h + skip -> GlobalContextModule -> head
// GATv2Conv (PyG 2.x semantics, restated from its documentation — the library is absent, parity with it unpinned):
// x_l = lin_l(x), x_r = lin_r(x) (both with bias), one self loop per node whose edge attribute is the MEAN of the node's
// incoming edge attributes (fill_value="mean"); for an edge j -> i and head h
//     m = leaky_relu(x_r[i] + x_l[j] + lin_edge(e_ij), 0.2);   a = att[h] . m[h];   alpha = softmax over the edges into i
//     out_i[h] = sum_j alpha_ij x_l[j][h];   concat heads, + bias.
// One wave per destination node (lane l holds channels l + 64 j): the per-head dot product is a butterfly over the head's
// C = D / heads consecutive lanes; the softmax is two passes over the node's incoming edges in CSR (= edge) order, the
// self loop last.  LayerNorm + GELU of the block are fused in (the wave holds the whole output row).  The per-block edge
// gate is the fused MFMA kernel of GCNTrimapNet with a multiply-only epilogue; the D x D products run on k_gemm.
#include "ggc_gnn.h"
#include <cmath>

namespace ggc {

template <int D>
__global__ void __launch_bounds__(256) k_gat_input(int N, const float* __restrict__ x, BnW bn_in, const float* __restrict__ w_inT,
                                                   const float* __restrict__ b_in, const float* __restrict__ ln_w,
                                                   const float* __restrict__ ln_b, float* __restrict__ h) {
    constexpr int NC = (D + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (int node = wave; node < N; node += n_waves) {
        float xn[IN_CH];
#pragma unroll
        for (int k = 0; k < IN_CH; ++k) xn[k] = bn_apply(x[(size_t)node * IN_CH + k], bn_in, k);
        float a[NC];
        float s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            float acc = 0.0f;
            if (c < D) {
#pragma unroll
                for (int k = 0; k < IN_CH; ++k) acc += xn[k] * w_inT[k * D + c];
                acc += b_in[c];
                s1 += acc;
            }
            a[j] = acc;
        }
        const float mean = wave_sum(s1) / (float)D;
        float s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j) { const int c = lane + 64 * j; if (c < D) { const float dv = a[j] - mean; s2 += dv * dv; } }
        const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)D + 1e-5f);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < D) h[(size_t)node * D + c] = gelu_f((a[j] - mean) * rstd * ln_w[c] + ln_b[c]);
        }
    }
}

struct GatW { const float *bl, *br, *weT /*[5][D]*/, *att /*[D]*/, *bias, *ln_w, *ln_b; };

template <int D, int HEADS>
__global__ void __launch_bounds__(256) k_gat_attn(int N, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                  const int32_t* __restrict__ eid, const float* __restrict__ edge_attr,
                                                  const float* __restrict__ xl, const float* __restrict__ xr, GatW w,
                                                  float* __restrict__ out) {
    constexpr int NC = (D + 63) / 64, C = D / HEADS;          // a head is C consecutive channels: C <= 64 consecutive lanes of one
                                                              // register, or (C > 64) all lanes of C / 64 consecutive registers
    static_assert(C >= 4 && (C & (C - 1)) == 0 && (C <= 64 || C % 64 == 0), "head width: a power of two from 4 to 256");
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    float bl[NC], att[NC], we[NC][EDGE_CH];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = lane + 64 * j;
        bl[j] = c < D ? w.bl[c] : 0.0f; att[j] = c < D ? w.att[c] : 0.0f;
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) we[j][k] = c < D ? w.weT[k * D + c] : 0.0f;
    }
    for (int node = wave; node < N; node += n_waves) {
        const int beg = row_ptr[node], end = row_ptr[node + 1], cnt = end - beg;
        float xri[NC], xli[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            xri[j] = c < D ? xr[(size_t)node * D + c] + w.br[c] : 0.0f;
            xli[j] = c < D ? xl[(size_t)node * D + c] + bl[j] : 0.0f;
        }
        // the self loop's edge attribute: mean of the incoming ones (sum in edge order / count; zeros without edges)
        float am[EDGE_CH] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = beg; p < end; ++p) {
            const float* a = edge_attr + (size_t)eid[p] * EDGE_CH;
#pragma unroll
            for (int k = 0; k < EDGE_CH; ++k) am[k] += a[k];
        }
        const float cf = (float)(cnt > 0 ? cnt : 1);
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) am[k] = am[k] / cf;
        // attention logit of one edge for this lane's head(s): every lane of a head ends with the head's value
        auto logit = [&](const float* a, const float (&xlj)[NC], float (&lg)[NC]) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                float ev = 0.0f;
#pragma unroll
                for (int k = 0; k < EDGE_CH; ++k) ev += a[k] * we[j][k];
                float m = (xri[j] + xlj[j]) + ev;
                m = m > 0.0f ? m : 0.2f * m;
                float v = m * att[j];
#pragma unroll
                for (int o = (C < 64 ? C : 64) / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                lg[j] = v;
            }
            if (C == 128 && NC == 2) { const float t = lg[0] + lg[NC - 1]; lg[0] = t; lg[NC - 1] = t; }     // one head across both registers: low half + high half
            if constexpr (C > 64 && NC > 2) {                 // D = 256: a head spans R registers, their partial sums added in order
                constexpr int R = C / 64;
#pragma unroll
                for (int j0 = 0; j0 < NC; j0 += R) {
                    float t = lg[j0];
#pragma unroll
                    for (int r = 1; r < R; ++r) t += lg[j0 + r];
#pragma unroll
                    for (int r = 0; r < R; ++r) lg[j0 + r] = t;
                }
            }
        };
        float mx[NC], lgs[NC];
        logit(am, xli, lgs);                                   // self loop
#pragma unroll
        for (int j = 0; j < NC; ++j) mx[j] = lgs[j];
        for (int p = beg; p < end; ++p) {
            const int src = col[p];
            float xlj[NC], lg[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) { const int c = lane + 64 * j; xlj[j] = c < D ? xl[(size_t)src * D + c] + bl[j] : 0.0f; }
            logit(edge_attr + (size_t)eid[p] * EDGE_CH, xlj, lg);
#pragma unroll
            for (int j = 0; j < NC; ++j) mx[j] = fmaxf(mx[j], lg[j]);
        }
        float ssum[NC], acc[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) { ssum[j] = 0.0f; acc[j] = 0.0f; }
        for (int p = beg; p < end; ++p) {                      // the edges in order ...
            const int src = col[p];
            float xlj[NC], lg[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) { const int c = lane + 64 * j; xlj[j] = c < D ? xl[(size_t)src * D + c] + bl[j] : 0.0f; }
            logit(edge_attr + (size_t)eid[p] * EDGE_CH, xlj, lg);
#pragma unroll
            for (int j = 0; j < NC; ++j) { const float e = ggc_expf(lg[j] - mx[j]); ssum[j] += e; acc[j] += e * xlj[j]; }
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) { const float e = ggc_expf(lgs[j] - mx[j]); ssum[j] += e; acc[j] += e * xli[j]; }    // ... the self loop last
        // + bias, LayerNorm, GELU
        float o[NC];
        float s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            o[j] = c < D ? acc[j] / (ssum[j] + 1e-16f) + w.bias[c] : 0.0f;
            if (c < D) s1 += o[j];
        }
        const float mean = wave_sum(s1) / (float)D;
        float s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j) { const int c = lane + 64 * j; if (c < D) { const float dv = o[j] - mean; s2 += dv * dv; } }
        const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)D + 1e-5f);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < D) out[(size_t)node * D + c] = gelu_f((o[j] - mean) * rstd * w.ln_w[c] + w.ln_b[c]);
        }
    }
}

// h + skip and the readout score attn . (h + skip) + b
template <int D>
__global__ void __launch_bounds__(256) k_gat_score(int N, const float* __restrict__ h, const float* __restrict__ skip,
                                                   const float* __restrict__ attn_w, const float* __restrict__ attn_b,
                                                   float* __restrict__ hs, float* __restrict__ score) {
    constexpr int NC = (D + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (int node = wave; node < N; node += n_waves) {
        float dot = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < D) {
                const float v = h[(size_t)node * D + c] + skip[(size_t)node * D + c];
                hs[(size_t)node * D + c] = v;
                dot += v * attn_w[c];
            }
        }
        dot = wave_sum(dot);
        if (lane == 0) score[node] = dot + attn_b[0];
    }
}

static std::vector<Need> needed_gat(const WeightSet& m) {
    const int D = m.D, n = m.n_layers;
    std::vector<Need> v;
    auto add = [&](const std::string& k, int r, int c, char layout = 0) { v.push_back({k, (int64_t)r * c, r, c, r, c, layout}); };
    for (const char* k : BN_KEYS) add(std::string("in_norm.norm.") + k, IN_CH, 1);
    add("input_proj.0.weight", D, IN_CH, 'T'); add("input_proj.0.bias", D, 1);
    add("input_proj.1.weight", D, 1); add("input_proj.1.bias", D, 1);
    for (int i = 0; i < n; ++i) {
        const std::string s = std::to_string(i), c = "convs." + s + ".", g = "edge_gates." + s + ".";
        add(c + "att", D, 1);
        add(c + "lin_l.weight", D, D, 'P'); add(c + "lin_l.bias", D, 1);
        add(c + "lin_r.weight", D, D, 'P'); add(c + "lin_r.bias", D, 1);
        add(c + "lin_edge.weight", D, EDGE_CH, 'T'); add(c + "bias", D, 1);
        add("lns." + s + ".weight", D, 1); add("lns." + s + ".bias", D, 1);
        add(g + "proj.0.weight", D, EDGE_CH, 'T'); add(g + "proj.0.bias", D, 1);
        add(g + "proj.2.weight", D, D, 'P'); add(g + "proj.2.bias", D, 1);
    }
    add("skip_proj.weight", D, D, 'P');
    add("ctx.attn.weight", D, 1); add("ctx.attn.bias", 1, 1);
    add("ctx.compress.weight", D / 2, D, 'T'); add("ctx.compress.bias", D / 2, 1);
    add("ctx.expand.weight", D, D / 2, 'T'); add("ctx.expand.bias", D, 1);
    add("head.0.weight", D, D, 'P'); add("head.0.bias", D, 1);
    add("head.3.weight", N_CLS, D); add("head.3.bias", N_CLS, 1);
    return v;
}

static const NetSpec GAT{"GATTrimapNet", "gat", &ggc_ctx::gat, true, needed_gat, nullptr};

template <int D>
static int forward_gat_t(ggc_ctx* ctx, hipStream_t st, int G, int N, int E, const float* x, const int32_t* edge_src,
                         const int32_t* edge_dst, const float* edge_attr, const int32_t* node_ptr, float* logits, float* probs) {
    WeightSet& m = ctx->gat;
    const int heads = m.heads;
    const int n = m.n_layers;
    const size_t ND = (size_t)N * D;
    Csr csr;
    int rc = prepare_csr(ctx, st, G, N, E, edge_src, edge_dst, node_ptr, true, csr);
    if (rc) return rc;
    float* buf = scratch_t<float>(ctx, S_STATES, ND * 4);        // h (ping) | h (pong) | skip | gelu(LN(conv))
    float* xl = scratch_t<float>(ctx, S_XW, ND);
    float* xr = scratch_t<float>(ctx, S_AGG, ND);
    float* hs = scratch_t<float>(ctx, S_HJK, ND);
    float* score = scratch_t<float>(ctx, S_SCORE, (size_t)N);
    float* gvec = scratch_t<float>(ctx, S_GVEC, (size_t)G * D);
    if (!buf || !xl || !xr || !hs || !score || !gvec) return GGC_E_OOM;
    const int wave_blocks = min(cdiv(N, 4), 8 * ctx->n_cu);
    float *h = buf, *h2 = buf + ND, *skip = buf + 2 * ND, *act = buf + 3 * ND;
    hipLaunchKernelGGL((k_gat_input<D>), dim3(wave_blocks), dim3(256), 0, st, N, x, bn_of(m, "in_norm.norm."),
                       devp(m, "#input_proj.0.weightT"), devp(m, "input_proj.0.bias"), devp(m, "input_proj.1.weight"),
                       devp(m, "input_proj.1.bias"), h);
    GGC_LAUNCH_CHECK(ctx);
    {
        GemmArgs a{};
        a.A1 = h; a.Wp1 = devp(m, "#skip_proj.weight.p"); a.out = skip;
        if ((rc = launch_gemm<D, 3>(ctx, st, N, a))) return rc;
    }
    for (int l = 0; l < n; ++l) {
        const std::string c = "convs." + std::to_string(l) + ".", g = "edge_gates." + std::to_string(l) + ".", ln = "lns." + std::to_string(l) + ".";
        GemmArgs a{};
        a.A1 = h; a.Wp1 = devp(m, "#" + c + "lin_l.weight.p"); a.out = xl;
        if ((rc = launch_gemm<D, 3>(ctx, st, N, a))) return rc;
        a.Wp1 = devp(m, "#" + c + "lin_r.weight.p"); a.out = xr;
        if ((rc = launch_gemm<D, 3>(ctx, st, N, a))) return rc;
        GatW w{devp(m, c + "lin_l.bias"), devp(m, c + "lin_r.bias"), devp(m, "#" + c + "lin_edge.weightT"), devp(m, c + "att"),
               devp(m, c + "bias"), devp(m, ln + "weight"), devp(m, ln + "bias")};
        {
            ProfScope prof(ctx, st, "gat_attention");
            with_width<8, 4, 2, 1>(heads, rc, [&](auto hc) {
                hipLaunchKernelGGL((k_gat_attn<D, decltype(hc)::value>), dim3(wave_blocks), dim3(256), 0, st, N, csr.row_ptr, csr.col, csr.eid,
                                   edge_attr, xl, xr, w, act);
                return GGC_OK; });
        }
        GGC_LAUNCH_CHECK(ctx);
        if ((rc = launch_edge_gate<D, true>(ctx, st, N, csr.row_ptr, csr.eid, csr.dst, edge_attr, devp(m, "#" + g + "proj.0.weightT"),
                                            devp(m, g + "proj.0.bias"), devp(m, "#" + g + "proj.2.weight.p"), devp(m, g + "proj.2.bias"),
                                            act, BnW{}, nullptr, h2)))
            return rc;
        std::swap(h, h2);
    }
    hipLaunchKernelGGL((k_gat_score<D>), dim3(wave_blocks), dim3(256), 0, st, N, h, skip, devp(m, "ctx.attn.weight"),
                       devp(m, "ctx.attn.bias"), hs, score);
    GGC_LAUNCH_CHECK(ctx);
    if ((rc = launch_graph_ctx<D>(ctx, st, G, node_ptr, score, hs, {devp(m, "#ctx.compress.weightT"), devp(m, "ctx.compress.bias"),
                                                                    devp(m, "#ctx.expand.weightT"), devp(m, "ctx.expand.bias")}, gvec)))
        return rc;
    {
        GemmArgs a{};
        a.A1 = hs; a.Wp1 = devp(m, "#head.0.weight.p"); a.bias = devp(m, "head.0.bias");
        a.batch = csr.batch; a.gvec = gvec;
        a.ep_w = devp(m, "head.3.weight"); a.ep_b = devp(m, "head.3.bias");
        a.out = logits; a.out2 = probs;
        if ((rc = launch_gemm<D, 4>(ctx, st, N, a))) return rc;
    }
    return GGC_OK;
}

} // namespace ggc

using namespace ggc;

extern "C" {

int ggc_gat_configure(ggc_ctx* ctx, int hidden, int n_heads, int n_layers) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, hidden == 32 || hidden == 64 || hidden == 128 || hidden == 256, GGC_E_UNSUPPORTED,
                "hidden_channels=%d unsupported: GATTrimapNet runs at 32, 64, 128 or 256 (a head must span a power-of-two number of lanes)", hidden);
    GGC_REQUIRE(ctx, n_heads == 1 || n_heads == 2 || n_heads == 4 || n_heads == 8, GGC_E_UNSUPPORTED,
                "n_heads=%d unsupported: 1, 2, 4 or 8 (the reference's default is 8)", n_heads);
    if (int rc = configure(ctx, GAT, hidden, hidden, n_layers)) return rc;
    ctx->gat.heads = n_heads;                // (the head count changes no weight shape: att is [1, H, D / H] = D values)
    return GGC_OK;
}

int ggc_gat_load_weight(ggc_ctx* ctx, const char* name, const float* data, int64_t numel) {
    return load_weight(ctx, GAT, name, data, numel);
}

int ggc_gat_ready(ggc_ctx* ctx) { return check_ready(ctx, GAT); }

int ggc_gat_forward(ggc_ctx* ctx, ggc_stream stream, int G, int N, int E, const float* x, const int32_t* edge_src,
                    const int32_t* edge_dst, const float* edge_attr, const int32_t* node_ptr, float* logits, float* probs) {
    int rc = begin_forward(ctx, GAT, G, N, E, x, edge_src, edge_dst, edge_attr, node_ptr, logits, probs);
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (with_width<32, 64, 128, 256>(ctx->gat.D, rc, [&](auto w) {
            return forward_gat_t<decltype(w)::value>(ctx, st, G, N, E, x, edge_src, edge_dst, edge_attr, node_ptr, logits, probs); }))
        return rc;
    return set_err(ctx, GGC_E_STATE, "model not configured");
}

} // extern "C"
