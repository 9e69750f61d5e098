// ggc_gcnnet.hip — GCNTrimapNet (reference model.py:239-316), eval mode.
//   in_norm -> Linear(19, D) + BatchNorm + ReLU -> n x ResGCNBlock -> head on the concatenated block outputs
//   ResGCNBlock (:216-232): h' = (relu(bn(GCNConv(h))) + h) * scatter_mean_dst(sigmoid(W2 relu(W1 e + b1) + b2))
// Reuses the destination CSR, the f32-MFMA product (k_gemm mode 3, no prologue norm) and the GCNConv gather of the
// ResGCNNet path.  The per-edge gate MLP, its scatter-mean and the block's BatchNorm / ReLU / residual epilogue are one
// kernel (k_gn_edge_gate, below).  BatchNorm1d(eval) = (x - mean) / sqrt(var + 1e-5) * w + b.
#include "ggc_gnn.h"
#include <cmath>

namespace ggc {

// in_norm + input_proj: one wave per node
template <int D>
__global__ void __launch_bounds__(256) k_gn_input(int N, const float* __restrict__ x, BnW bn_in, const float* __restrict__ w_inT,
                                                  const float* __restrict__ b_in, BnW bn1, float* __restrict__ h) {
    constexpr int NC = (D + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (int node = wave; node < N; node += n_waves) {
        float xn[IN_CH];
#pragma unroll
        for (int k = 0; k < IN_CH; ++k) xn[k] = bn_apply(x[(size_t)node * IN_CH + k], bn_in, k);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < D) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < IN_CH; ++k) acc += xn[k] * w_inT[k * D + c];
                const float v = bn_apply(acc + b_in[c], bn1, c);
                h[(size_t)node * D + c] = v > 0.0f ? v : 0.0f;
            }
        }
    }
}

// head tail: z = relu(bn(z0 + b0)) -> Linear(D, D/2) + ReLU -> Linear(D/2, 3) (+ softmax); one wave per node
template <int D>
__global__ void __launch_bounds__(256) k_gn_head(int N, const float* __restrict__ z0, const float* __restrict__ b0, BnW bn,
                                                 const float* __restrict__ w4T /*[D][D/2]*/, const float* __restrict__ b4,
                                                 const float* __restrict__ w6 /*[3][D/2]*/, const float* __restrict__ b6,
                                                 float* __restrict__ logits, float* __restrict__ probs) {
    constexpr int DH = D / 2, NC = (D + 63) / 64;
    __shared__ float s_z[4][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (int node = wave; node < N; node += n_waves) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < D) {
                const float v = bn_apply(z0[(size_t)node * D + c] + b0[c], bn, c);
                s_z[wv][c] = v > 0.0f ? v : 0.0f;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float a = 0.0f;                                    // hidden unit `lane` of the D/2 layer (D/2 <= 64)
        if (lane < DH) {
            for (int k = 0; k < D; ++k) a += s_z[wv][k] * w4T[k * DH + lane];
            a += b4[lane];
            a = a > 0.0f ? a : 0.0f;
        }
        float p[N_CLS];
#pragma unroll
        for (int c = 0; c < N_CLS; ++c) {
            // index-order sum like the oracle: lane k contributes a_k * w6[c][k], folded sequentially by lane 0
            p[c] = (lane < DH) ? a * w6[c * DH + lane] : 0.0f;
        }
        float lg[N_CLS] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < DH; ++k) {
#pragma unroll
            for (int c = 0; c < N_CLS; ++c) lg[c] += __shfl(p[c], k, 64);
        }
        if (lane == 0) {
            const float l0 = lg[0] + b6[0], l1 = lg[1] + b6[1], l2 = lg[2] + b6[2];
            if (logits) { logits[(size_t)node * 3 + 0] = l0; logits[(size_t)node * 3 + 1] = l1; logits[(size_t)node * 3 + 2] = l2; }
            if (probs) {
                const float mx = fmaxf(l0, fmaxf(l1, l2));
                const float e0 = ggc_expf(l0 - mx), e1 = ggc_expf(l1 - mx), e2 = ggc_expf(l2 - mx);
                const float s = (e0 + e1) + e2;
                probs[(size_t)node * 3 + 0] = e0 / s; probs[(size_t)node * 3 + 1] = e1 / s; probs[(size_t)node * 3 + 2] = e2 / s;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}


// ------------------------------------------------------------------------ fused edge gate
// GCNTrimapNet, fused edge gate.  The gate MLP of a block is 316 of the model's 350 GFLOP at batch 256, and done as
// separate passes its E x D intermediates (2 x 824 MB) cross HBM four times per block.  Here a wave owns a contiguous
// range of destination nodes — hence a contiguous range of CSR edge positions — and walks it in tiles of 32 edges:
//   * the first layer relu(W1 e + b1) is generated straight into the MFMA A operand (5 multiply-adds per value);
//   * the D x D layer runs on v_mfma_f32_32x32x2_f32 against W2 packed in LDS, like k_gemm;
//   * sigmoid(. + b2) goes through a small LDS tile and is summed per destination in CSR (= edge) order, and at the
//     end of a destination's edges the block epilogue out = (relu(bn(conv)) + h) * mean is written directly.
// Nothing of size E x D reaches memory.  Same sums in the same order as the unfused kernels.
constexpr int EG_WAVES = 8, EG_NODES = 32;     // waves per block, destination nodes per wave
constexpr int EG_STAGE = 66;                   // row stride of the sigmoid tile: two 32-column tiles + 2 words of padding

template <int D, bool MUL_ONLY>      // MUL_ONLY: out = conv * mean (GATTrimapNet: conv holds gelu(LayerNorm(GATv2)) already)
__global__ void __launch_bounds__(64 * EG_WAVES) k_gn_edge_gate(int N, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ eid,
                                                                const int32_t* __restrict__ csr_dst,
                                                                const float* __restrict__ edge_attr, const float* __restrict__ w1T,
                                                                const float* __restrict__ b1, const float* __restrict__ w2p,
                                                                const float* __restrict__ b2, const float* __restrict__ conv, BnW bn,
                                                                const float* __restrict__ h, float* __restrict__ out) {
    constexpr int T = D / 32, KH = D / 2;
    // Above 128 the packed W2 (256 KiB at 256) does not fit the LDS: the MFMA loop reads its B fragments from memory (W2 stays
    // in L2), and the A operand is generated four k-steps at a time next to them, in the same k order.
    constexpr bool W2_LDS = D <= 128;
    extern __shared__ float4 eg_smem4[];                       // W2 packed [D*D] (D <= 128) | W1T [5][D] | b1 [D] | per wave stage [32][EG_STAGE]
    float* s_w1 = reinterpret_cast<float*>(eg_smem4) + (W2_LDS ? (size_t)D * D : 0);
    float* s_b1 = s_w1 + EDGE_CH * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* stage = s_b1 + D + (size_t)wave * 32 * EG_STAGE;
    const int hk = lane >> 5, li = lane & 31;
    if constexpr (W2_LDS)
        for (int i = tid; i < D * D / 4; i += 64 * EG_WAVES) eg_smem4[i] = reinterpret_cast<const float4*>(w2p)[i];
    for (int i = tid; i < EDGE_CH * D; i += 64 * EG_WAVES) s_w1[i] = w1T[i];
    for (int i = tid; i < D; i += 64 * EG_WAVES) s_b1[i] = b1[i];
    __syncthreads();
    const int n0 = (blockIdx.x * EG_WAVES + wave) * EG_NODES;
    if (n0 >= N) return;                                        // (after the only block barrier)
    const int n1 = min(n0 + EG_NODES, N);
    const int e0 = row_ptr[n0], e1 = row_ptr[n1];

    // epilogue of one destination for this lane's column of column tile t
    auto flush = [&](int node, int t, float sum) {
        const int c = 32 * t + li;
        const int cnt = row_ptr[node + 1] - row_ptr[node];
        const float cf = (float)(cnt > 1 ? cnt : 1);
        float v = conv[(size_t)node * D + c];
        if (!MUL_ONLY) {
            v = bn_apply(v, bn, c);
            v = v > 0.0f ? v : 0.0f;
            v = v + h[(size_t)node * D + c];
        }
        out[(size_t)node * D + c] = v * (sum / cf);
    };
    float sums[T];
#pragma unroll
    for (int t = 0; t < T; ++t) sums[t] = 0.0f;
    int cur = n0;                                               // destination whose edges are being summed (wave-uniform)
    // the tile's inputs (edge attributes through eid, destination of every CSR position) are dependent global loads: the
    // next tile's are fetched while this tile's MFMAs run
    float ea_n[EDGE_CH] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int dnode_n = n1;
    auto fetch = [&](int base) {
        const int j = base + li;
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) ea_n[k] = 0.0f;
        dnode_n = n1;
        if (j < e1) {
            const float* a = edge_attr + (size_t)eid[j] * EDGE_CH;
#pragma unroll
            for (int k = 0; k < EDGE_CH; ++k) ea_n[k] = a[k];
            dnode_n = csr_dst[j];
        }
    };
    fetch(e0);
    for (int base = e0; base < e1; base += 32) {
        // ---- A operand: this lane's half row of relu(W1 e + b1) for edge position base + li
        const bool have = base + li < e1;
        float ea[EDGE_CH];
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) ea[k] = ea_n[k];
        const int dnode = dnode_n;
        if (base + 32 < e1) fetch(base + 32);
        float a[KH];
#pragma unroll
        for (int s = 0; s < (W2_LDS ? KH : 0); s += 4) {       // four values at a time on the packed-f32 pipe, same op order
            const int c = hk * KH + s;
            v4f acc4 = 0.0f;
#pragma unroll
            for (int k = 0; k < EDGE_CH; ++k) acc4 += ea[k] * *reinterpret_cast<const v4f*>(s_w1 + k * D + c);
            acc4 += *reinterpret_cast<const v4f*>(s_b1 + c);
            a[s + 0] = (have && acc4.x > 0.0f) ? acc4.x : 0.0f; a[s + 1] = (have && acc4.y > 0.0f) ? acc4.y : 0.0f;
            a[s + 2] = (have && acc4.z > 0.0f) ? acc4.z : 0.0f; a[s + 3] = (have && acc4.w > 0.0f) ? acc4.w : 0.0f;
        }
        f32x16 acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        if constexpr (W2_LDS) {
#pragma unroll
        for (int s4 = 0; s4 < KH / 4; ++s4) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float4 b = eg_smem4[(s4 * T + t) * 64 + lane];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * s4 + 0], b.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * s4 + 1], b.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * s4 + 2], b.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * s4 + 3], b.w, acc[t], 0, 0, 0);
            }
        }
        } else {
            const float4* w2p4 = reinterpret_cast<const float4*>(w2p);
#pragma unroll 1
            for (int s4 = 0; s4 < KH / 4; ++s4) {
                const int c = hk * KH + 4 * s4;
                v4f acc4 = 0.0f;
#pragma unroll
                for (int k = 0; k < EDGE_CH; ++k) acc4 += ea[k] * *reinterpret_cast<const v4f*>(s_w1 + k * D + c);
                acc4 += *reinterpret_cast<const v4f*>(s_b1 + c);
                const float a0 = (have && acc4.x > 0.0f) ? acc4.x : 0.0f, a1 = (have && acc4.y > 0.0f) ? acc4.y : 0.0f;
                const float a2 = (have && acc4.z > 0.0f) ? acc4.z : 0.0f, a3 = (have && acc4.w > 0.0f) ? acc4.w : 0.0f;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float4 b = w2p4[(s4 * T + t) * 64 + lane];
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b.x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b.y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b.z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b.w, acc[t], 0, 0, 0);
                }
            }
        }
        const int n_rows = min(32, e1 - base);
        const int cur_in = cur;
        // ---- two column tiles at a time: sigmoid through the LDS tile, then an ordered walk down the rows in which lane
        // (hk, li) owns column 32 (t + hk) + li
        int c_last = cur_in;
#pragma unroll
        for (int t = 0; t < T; t += 2) {
#pragma unroll
            for (int tt = 0; tt < 2 && t + tt < T; ++tt) {
                const float bias = b2[32 * (t + tt) + li];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // sigmoid as the shared IEEE sequence (include/ggc_fmath.h): the oracle produces the same bits
                    const float z = acc[t + tt][r] + bias;
                    stage[((r & 3) + 8 * (r >> 2) + 4 * hk) * EG_STAGE + 32 * tt + li] = ggc_sigmoid_nr(z);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int mt = t + hk;                              // this lane's column tile in the walk
            const bool mine = mt < T;
            float sum = 0.0f;
#pragma unroll
            for (int q = 0; q < T; ++q) if (q == mt) sum = sums[q];
            int c_node = cur_in;
            for (int row = 0; row < n_rows; ++row) {
                const int nd = __shfl(dnode, row, 64);          // wave-uniform
                if (nd != c_node) {
                    if (mine) {
                        flush(c_node, mt, sum);
                        for (int z = c_node + 1; z < nd; ++z) flush(z, mt, 0.0f);     // destinations without edges
                    }
                    c_node = nd; sum = 0.0f;
                }
                sum += stage[row * EG_STAGE + 32 * hk + li];
            }
#pragma unroll
            for (int q = 0; q < T; ++q) if (q == mt) sums[q] = sum;
            c_last = c_node;
            __builtin_amdgcn_wave_barrier();
        }
        cur = c_last;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if ((t & 1) == hk) {                                    // the lane half that summed this column tile
            flush(cur, t, sums[t]);
            for (int z = cur + 1; z < n1; ++z) flush(z, t, 0.0f);
        }
    }
}

template <int D, bool MUL_ONLY>
int launch_edge_gate(ggc_ctx* ctx, hipStream_t st, int N, const int32_t* row_ptr, const int32_t* eid, const int32_t* csr_dst,
                            const float* edge_attr, const float* w1T, const float* b1, const float* w2p, const float* b2,
                            const float* conv, const BnW& bn, const float* h, float* out) {
    const size_t lds = ((D <= 128 ? (size_t)D * D : 0) + (size_t)EDGE_CH * D + D + (size_t)EG_WAVES * 32 * EG_STAGE) * sizeof(float);
    static DeviceOnce attr_set;
    if (attr_set.need(ctx->device)) {
        GGC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gn_edge_gate<D, MUL_ONLY>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
        attr_set.done(ctx->device);
    }
    ProfScope prof(ctx, st, "gcnnet_edge_gate");
    hipLaunchKernelGGL((k_gn_edge_gate<D, MUL_ONLY>), dim3(cdiv(N, EG_WAVES * EG_NODES)), dim3(64 * EG_WAVES), lds, st, N, row_ptr, eid, csr_dst,
                       edge_attr, w1T, b1, w2p, b2, conv, bn, h, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
// the widths GATTrimapNet (ggc_gat.hip) runs the multiply-only gate at
#define GGC_EDGE_GATE(D) template int launch_edge_gate<D, true>(ggc_ctx*, hipStream_t, int, const int32_t*, const int32_t*, \
    const int32_t*, const float*, const float*, const float*, const float*, const float*, const float*, const BnW&, const float*, float*);
GGC_EDGE_GATE(32) GGC_EDGE_GATE(64) GGC_EDGE_GATE(128) GGC_EDGE_GATE(256)
#undef GGC_EDGE_GATE

static std::vector<Need> needed_gcnnet(const WeightSet& m) {
    const int D = m.D, n = m.n_layers;
    std::vector<Need> v;
    auto add = [&](const std::string& k, int r, int c, char layout = 0) { v.push_back({k, (int64_t)r * c, r, c, r, c, layout}); };
    auto bn = [&](const std::string& p, int len) { for (const char* k : BN_KEYS) add(p + k, len, 1); };
    bn("in_norm.norm.", IN_CH);
    add("input_proj.0.weight", D, IN_CH, 'T'); add("input_proj.0.bias", D, 1);
    bn("input_proj.1.", D);
    for (int i = 0; i < n; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        add(p + "conv.bias", D, 1); add(p + "conv.lin.weight", D, D, 'P');
        bn(p + "bn.", D);
        add(p + "edge_inject.proj.0.weight", D, EDGE_CH, 'T'); add(p + "edge_inject.proj.0.bias", D, 1);
        add(p + "edge_inject.proj.2.weight", D, D, 'P'); add(p + "edge_inject.proj.2.bias", D, 1);
    }
    add("head.0.weight", D, D * (n + 1)); add("head.0.bias", D, 1);
    bn("head.1.", D);
    add("head.4.weight", D / 2, D, 'T'); add("head.4.bias", D / 2, 1);
    add("head.6.weight", N_CLS, D / 2); add("head.6.bias", N_CLS, 1);
    return v;
}

// head.0 on the concatenated states [D][D (n+1)]: one packed D x D block per state, "#head.0.weight.p<s>"
static int derive_gcnnet(ggc_ctx* ctx, WeightSet& m, std::map<std::string, std::vector<float>>& w) {
    const int D = m.D, n = m.n_layers;
    const std::vector<float>& hw = w["head.0.weight"];
    for (int s = 0; s <= n; ++s) {
        std::vector<float> blk((size_t)D * D);
        for (int o = 0; o < D; ++o)
            for (int k = 0; k < D; ++k) blk[(size_t)o * D + k] = hw[(size_t)o * D * (n + 1) + (size_t)s * D + k];
        if (int rc = upload(ctx, m, "#head.0.weight.p" + std::to_string(s), pack_mfma(blk, D))) return rc;
    }
    return GGC_OK;
}

static const NetSpec GCNNET{"GCNTrimapNet", "gcnnet", &ggc_ctx::gcnnet, false, needed_gcnnet, derive_gcnnet};

template <int D>
static int forward_gcnnet_t(ggc_ctx* ctx, hipStream_t st, int N, int E, const float* x, const int32_t* edge_src,
                            const int32_t* edge_dst, const float* edge_attr, float* logits, float* probs) {
    WeightSet& m = ctx->gcnnet;
    const int n = m.n_layers, n_states = n + 1;
    const size_t ND = (size_t)N * D;
    Csr csr;
    int rc = prepare_csr(ctx, st, 1, N, E, edge_src, edge_dst, nullptr, true, csr);
    if (rc) return rc;
    float* states = scratch_t<float>(ctx, S_STATES, ND * n_states);
    float* xw = scratch_t<float>(ctx, S_XW, ND);
    float* conv = scratch_t<float>(ctx, S_AGG, ND);
    float* z0 = scratch_t<float>(ctx, S_HJK, ND);
    if (!states || !xw || !conv || !z0) return GGC_E_OOM;
    const int wave_blocks = min(cdiv(N, 4), 8 * ctx->n_cu);
    hipLaunchKernelGGL((k_gn_input<D>), dim3(wave_blocks), dim3(256), 0, st, N, x, bn_of(m, "in_norm.norm."),
                       devp(m, "#input_proj.0.weightT"), devp(m, "input_proj.0.bias"), bn_of(m, "input_proj.1."), states);
    GGC_LAUNCH_CHECK(ctx);
    for (int l = 0; l < n; ++l) {
        const std::string p = "blocks." + std::to_string(l) + ".";
        const float* h = states + ND * l;
        float* out = states + ND * (l + 1);
        GemmArgs a{};
        a.A1 = h; a.Wp1 = devp(m, "#" + p + "conv.lin.weight.p"); a.out = xw;
        if ((rc = launch_gemm<D, 3>(ctx, st, N, a))) return rc;
        if ((rc = launch_aggregate<D, 0>(ctx, st, N, xw, csr.row_ptr, csr.col, csr.dis, devp(m, p + "conv.bias"), nullptr, nullptr, conv))) return rc;
        // edge MLP + scatter-mean + block epilogue in one kernel (k_gn_edge_gate below)
        if ((rc = launch_edge_gate<D, false>(ctx, st, N, csr.row_ptr, csr.eid, csr.dst, edge_attr, devp(m, "#" + p + "edge_inject.proj.0.weightT"),
                                      devp(m, p + "edge_inject.proj.0.bias"), devp(m, "#" + p + "edge_inject.proj.2.weight.p"),
                                      devp(m, p + "edge_inject.proj.2.bias"), conv, bn_of(m, p + "bn."), h, out)))
            return rc;
    }
    for (int s = 0; s < n_states; ++s) {                       // head.0 on the concatenation = sum of per-state products
        GemmArgs a{};
        a.A1 = states + ND * s; a.Wp1 = devp(m, "#head.0.weight.p" + std::to_string(s)); a.out = z0; a.accumulate = s > 0;
        if ((rc = launch_gemm<D, 3>(ctx, st, N, a))) return rc;
    }
    hipLaunchKernelGGL((k_gn_head<D>), dim3(wave_blocks), dim3(256), 0, st, N, z0, devp(m, "head.0.bias"), bn_of(m, "head.1."),
                       devp(m, "#head.4.weightT"), devp(m, "head.4.bias"), devp(m, "head.6.weight"), devp(m, "head.6.bias"),
                       logits, probs);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

} // namespace ggc

using namespace ggc;

extern "C" {

int ggc_gcnnet_configure(ggc_ctx* ctx, int hidden, int n_layers) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, hidden == 32 || hidden == 64 || hidden == 96 || hidden == 128, GGC_E_UNSUPPORTED,
                "hidden_channels=%d unsupported: the MFMA tiling needs a multiple of 32 up to 128", hidden);
    return configure(ctx, GCNNET, hidden, hidden, n_layers);
}

int ggc_gcnnet_load_weight(ggc_ctx* ctx, const char* name, const float* data, int64_t numel) {
    return load_weight(ctx, GCNNET, name, data, numel);
}

int ggc_gcnnet_ready(ggc_ctx* ctx) { return check_ready(ctx, GCNNET); }

int ggc_gcnnet_forward(ggc_ctx* ctx, ggc_stream stream, int N, int E, const float* x, const int32_t* edge_src,
                       const int32_t* edge_dst, const float* edge_attr, float* logits, float* probs) {
    int rc = begin_forward(ctx, GCNNET, 0, N, E, x, edge_src, edge_dst, edge_attr, nullptr, logits, probs);
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (with_width<32, 64, 96, 128>(ctx->gcnnet.D, rc, [&](auto w) {
            return forward_gcnnet_t<decltype(w)::value>(ctx, st, N, E, x, edge_src, edge_dst, edge_attr, logits, probs); }))
        return rc;
    return set_err(ctx, GGC_E_STATE, "model not configured");
}

} // extern "C"
