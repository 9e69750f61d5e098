// ggc_resgcn.hip — ResGCNNet forward (reference model.py:421-546, eval mode) as
// hand-written gfx950 kernels: the kernels that are ResGCNNet's alone, its weight
// spec and the forward that strings them together with the shared ones.
//
// Kernel map:
//   k_input        M1  BatchNorm-eval -> Linear 19->D -> LayerNorm -> GELU -> prior booster
//   k_edge_gate    M2  EdgeContext: edge MLP, mean over incoming edges, LN, Linear, sigmoid
//                      (k_edge_gate_wide above D = 128: two context channels per lane, one gate column half per block)
//   k_jk           M5  softmax(jk_logits)-weighted sum of the n+2 states + attention score
// and, from the units the three networks share:
//   ggc_csr.hip         prepare_csr: the destination CSR, dis, the graph of every node
//   ggc_gnn_dense.hip   k_gemm<.,0> M3 LayerNorm(h) @ W^T, k_gemm<.,1> M4 lin_l(mean) + lin_r(h) -> LN -> GELU,
//                       k_gemm<.,2> M7 (h_jk * g) -> LN -> Linear -> GELU -> head -> softmax; k_graph_ctx M6
//   ggc_gnn_gather.hip  k_aggregate_graph / k_aggregate<.,0> M3 GCNConv gather with the fused epilogue
//                       h + gelu((agg + b) * gate), <.,1> M4 SAGEConv mean
//
// Data layout in HBM: node-major row vectors, f32, D contiguous (512 B rows at
// D=128).  Graphs of a batch are concatenated (PyG Batch semantics); node_ptr
// gives the per-graph ranges.  The destination CSR (row_ptr, col, eid) is
// built once per forward, stable in edge order, and reused by all 8 gathers.
#include "ggc_gnn.h"
#include <cmath>

namespace ggc {

// --------------------------------------------------------------- M1: input stage
// One wave per node; lane owns columns lane + 64 j.
struct InputW {
    const float *bn_w, *bn_b, *bn_rm, *bn_rv;
    const float *w_inT /*[19][D]*/, *b_in, *ln_w, *ln_b;
    const float *pb_w0 /*[Q,3]*/, *pb_b0, *pb_w2T /*[Q][D]*/, *pb_b2;
};

// Dt: the model's true width.  D is Dt rounded up to a multiple of 32 (MFMA tiling); the padded channels carry exact zeros
// through every layer (zero weight rows / columns, zero LayerNorm weights), so only the LayerNorm STATISTICS need to know
// Dt: the sum over D equals the sum over Dt, the mean divides by Dt, and the squared deviations of the padded channels
// (each mean^2) are left out.
template <int D>
__global__ void __launch_bounds__(256) k_input(int N, const float* __restrict__ x, InputW w, int Q, int Dt,
                                               float* __restrict__ h) {
    constexpr int NC = (D + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int n_waves = (gridDim.x * blockDim.x) >> 6;
    for (int node = wave; node < N; node += n_waves) {
        const float* xi = x + (size_t)node * IN_CH;
        float xn[IN_CH];
#pragma unroll
        for (int k = 0; k < IN_CH; ++k)
            xn[k] = (xi[k] - w.bn_rm[k]) / sqrtf(w.bn_rv[k] + 1e-5f) * w.bn_w[k] + w.bn_b[k];
        float a[NC];
        float s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            float acc = 0.0f;
            if (c < D) {
#pragma unroll
                for (int k = 0; k < IN_CH; ++k) acc += xn[k] * w.w_inT[k * D + c];
                acc += w.b_in[c];
                s1 += acc;
            }
            a[j] = acc;
        }
        const float mean = wave_sum(s1) / (float)Dt;
        float s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < Dt) { const float d = a[j] - mean; s2 += d * d; }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)Dt + 1e-5f);
        // prior booster hidden unit on lane q < Q
        const float p0 = xi[IN_CH - 3], p1 = xi[IN_CH - 2], p2 = xi[IN_CH - 1];
        float bq = 0.0f;
        if (lane < Q) {
            float acc = 0.0f;
            acc += p0 * w.pb_w0[lane * 3 + 0];
            acc += p1 * w.pb_w0[lane * 3 + 1];
            acc += p2 * w.pb_w0[lane * 3 + 2];
            bq = gelu_f(acc + w.pb_b0[lane]);
        }
        float g[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) g[j] = 0.0f;
        for (int q = 0; q < Q; ++q) {
            const float bv = __shfl(bq, q, 64);
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int c = lane + 64 * j;
                if (c < D) g[j] += bv * w.pb_w2T[q * D + c];
            }
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < D) {
                const float v = gelu_f((a[j] - mean) * rstd * w.ln_w[c] + w.ln_b[c]);
                h[(size_t)node * D + c] = v * (1.0f + sigmoid_f(g[j] + w.pb_b2[c]));
            }
        }
    }
}

// ------------------------------------------------------------- M2: edge context
struct EdgeW {
    const float *w0 /*[C,5]*/, *b0, *w2T /*[C][C] in-major*/, *b2;
    const float *ln_w, *ln_b, *wgT /*[C][D]*/, *bg;
};

// A wave owns EC_NODES consecutive nodes at a time, lane = context channel (C <= 64).  Both weight matrices are staged once
// per block in LDS and every k-step of the two matrix-vector products serves all EC_NODES nodes: one LDS read of the weight,
// a v_readlane broadcast of each node's value, and the same multiply-add sequence per output as the one-node-per-wave
// form (products added in k order from zero, bias last) — so the gate keeps its bits.  That form re-read the 48 KB of
// weights from the cache for every node: 0.76 ms per batch-256 forward.
constexpr int EC_NODES = 4;
template <int D>
__global__ void __launch_bounds__(256) k_edge_gate(int N, const int32_t* __restrict__ row_ptr,
                                                   const int32_t* __restrict__ eid,
                                                   const float* __restrict__ edge_attr, EdgeW w, int C,
                                                   float* __restrict__ gate) {
    constexpr int NC = (D + 63) / 64;
    extern __shared__ float s_w[];                  // w2T [C][C] | wgT [C][D]
    float* s_w2 = s_w;
    float* s_wg = s_w + C * C;
    for (int i = threadIdx.x; i < C * C; i += 256) s_w2[i] = w.w2T[i];
    for (int i = threadIdx.x; i < C * D; i += 256) s_wg[i] = w.wgT[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int n_waves = (gridDim.x * blockDim.x) >> 6;
    float w0[EDGE_CH] = {0, 0, 0, 0, 0};
    float b0 = 0.0f, b2 = 0.0f, lw = 0.0f, lb = 0.0f;
    if (lane < C) {
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) w0[k] = w.w0[lane * EDGE_CH + k];
        b0 = w.b0[lane]; b2 = w.b2[lane]; lw = w.ln_w[lane]; lb = w.ln_b[lane];
    }
    float bg[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) bg[j] = lane + 64 * j < D ? w.bg[lane + 64 * j] : 0.0f;
    for (int n0 = wave * EC_NODES; n0 < N; n0 += n_waves * EC_NODES) {
        float m[EC_NODES];
        int cnt[EC_NODES];
        // the nodes' incoming edges are one contiguous stretch of the CSR: a lane fetches one edge (index + 5 attributes, the
        // loads of a whole stretch in flight together), the per-edge loop then takes them from registers by v_readlane —
        // walking the edges one at a time through scalar loads was two dependent memory round trips per edge
        int rp[EC_NODES + 1];
#pragma unroll
        for (int r = 0; r <= EC_NODES; ++r) rp[r] = __builtin_amdgcn_readfirstlane(row_ptr[min(n0 + r, N)]);
        float sum[EC_NODES];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) sum[r] = 0.0f;
        for (int chunk = rp[0]; chunk < rp[EC_NODES]; chunk += 64) {
            const int p = chunk + lane;
            float a[EDGE_CH];
            {
                const bool valid = p < rp[EC_NODES];
                const size_t e = valid ? (size_t)eid[p] : 0;
#pragma unroll
                for (int k = 0; k < EDGE_CH; ++k) a[k] = valid ? edge_attr[e * EDGE_CH + k] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < EC_NODES; ++r) {
                const int q0 = max(rp[r], chunk) - chunk, q1 = min(rp[r + 1], chunk + 64) - chunk;      // this node's edges inside the chunk
                for (int q = q0; q < q1; ++q) {
                    float acc = 0.0f;
#pragma unroll
                    for (int k = 0; k < EDGE_CH; ++k) acc += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[k]), q)) * w0[k];
                    sum[r] += gelu_f(acc + b0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) {
            cnt[r] = rp[r + 1] - rp[r];
            // mean over incoming edges commutes with the second (linear) layer:
            // mean_e(W2 e1_e + b2) = W2 mean_e(e1_e) + b2  (model.py:138, _scatter_mean :69-74)
            m[r] = sum[r] / (float)(cnt[r] > 0 ? cnt[r] : 1);
        }
        float acc[EC_NODES];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) acc[r] = 0.0f;
        for (int k = 0; k < C; ++k) {
            const float wk = lane < C ? s_w2[k * C + lane] : 0.0f;
#pragma unroll
            for (int r = 0; r < EC_NODES; ++r)
                acc[r] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m[r]), k)) * wk;
        }
        float ln[EC_NODES];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) {
            const float cv = (lane < C && cnt[r] > 0) ? acc[r] + b2 : 0.0f;
            const float mean = wave_sum(lane < C ? cv : 0.0f) / (float)C;
            const float dv = (lane < C) ? cv - mean : 0.0f;
            const float rstd = 1.0f / sqrtf(wave_sum(dv * dv) / (float)C + 1e-5f);
            ln[r] = (lane < C) ? dv * rstd * lw + lb : 0.0f;
        }
        float g[EC_NODES][NC];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r)
#pragma unroll
            for (int j = 0; j < NC; ++j) g[r][j] = 0.0f;
        for (int k = 0; k < C; ++k) {
            float wk[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) wk[j] = lane + 64 * j < D ? s_wg[k * D + lane + 64 * j] : 0.0f;
#pragma unroll
            for (int r = 0; r < EC_NODES; ++r) {
                const float lk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ln[r]), k));
#pragma unroll
                for (int j = 0; j < NC; ++j) g[r][j] += lk * wk[j];
            }
        }
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) {
            if (n0 + r >= N) break;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int c = lane + 64 * j;
                if (c < D) gate[(size_t)(n0 + r) * D + c] = sigmoid_f(g[r][j] + bg[j]);
            }
        }
    }
}

// k_edge_gate at D > 128, where C = D/2 reaches 128 and the two matrices (C*C + C*D floats, 192 KiB at D = 256) no longer
// fit the LDS: a lane owns context channels lane and lane + 64, and a block computes one column half of the gate (blockIdx
// parity), so it stages w2T and that half of wgT (128 KiB at D = 256).  The two blocks of a node group both run the edge
// MLP, the mean and the LayerNorm.  Each output is still its products added in k order from zero, bias last.  With one
// block per CU at D = 256, the block is 16 waves (EGW_THREADS) so that the CU has work to switch between.
constexpr int EGW_THREADS = 1024;
template <int D>
__global__ void __launch_bounds__(EGW_THREADS) k_edge_gate_wide(int N, const int32_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ eid,
                                                        const float* __restrict__ edge_attr, EdgeW w, int C,
                                                        float* __restrict__ gate) {
    constexpr int DH = D / 2, NC = (DH + 63) / 64;
    static_assert(D > 128 && D <= 256, "the wide form is built for 160 ... 256");
    extern __shared__ float s_w[];                  // w2T [C][C] | wgT[:, half] [C][DH]
    const int c_off = (blockIdx.x & 1) * DH;
    float* s_w2 = s_w;
    float* s_wg = s_w + C * C;
    for (int i = threadIdx.x; i < C * C; i += EGW_THREADS) s_w2[i] = w.w2T[i];
    for (int i = threadIdx.x; i < C * DH; i += EGW_THREADS) s_wg[i] = w.wgT[(i / DH) * D + c_off + i % DH];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = ((blockIdx.x >> 1) * blockDim.x + threadIdx.x) >> 6;
    const int n_waves = ((gridDim.x >> 1) * blockDim.x) >> 6;
    const int C0 = min(C, 64);                      // channels k < C0 live in register 0 of lane k, the rest in register 1
    float w0[2][EDGE_CH], b0[2], b2[2], lw[2], lb[2];
    bool have[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        have[h] = c < C;
#pragma unroll
        for (int k = 0; k < EDGE_CH; ++k) w0[h][k] = have[h] ? w.w0[c * EDGE_CH + k] : 0.0f;
        b0[h] = have[h] ? w.b0[c] : 0.0f; b2[h] = have[h] ? w.b2[c] : 0.0f;
        lw[h] = have[h] ? w.ln_w[c] : 0.0f; lb[h] = have[h] ? w.ln_b[c] : 0.0f;
    }
    float bg[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) bg[j] = lane + 64 * j < DH ? w.bg[c_off + lane + 64 * j] : 0.0f;
    for (int n0 = wave * EC_NODES; n0 < N; n0 += n_waves * EC_NODES) {
        int rp[EC_NODES + 1];
#pragma unroll
        for (int r = 0; r <= EC_NODES; ++r) rp[r] = __builtin_amdgcn_readfirstlane(row_ptr[min(n0 + r, N)]);
        float sum[EC_NODES][2];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) sum[r][0] = sum[r][1] = 0.0f;
        for (int chunk = rp[0]; chunk < rp[EC_NODES]; chunk += 64) {
            const int p = chunk + lane;
            float a[EDGE_CH];
            {
                const bool valid = p < rp[EC_NODES];
                const size_t e = valid ? (size_t)eid[p] : 0;
#pragma unroll
                for (int k = 0; k < EDGE_CH; ++k) a[k] = valid ? edge_attr[e * EDGE_CH + k] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < EC_NODES; ++r) {
                const int q0 = max(rp[r], chunk) - chunk, q1 = min(rp[r + 1], chunk + 64) - chunk;
                for (int q = q0; q < q1; ++q) {
                    float ak[EDGE_CH];
#pragma unroll
                    for (int k = 0; k < EDGE_CH; ++k) ak[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[k]), q));
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float acc = 0.0f;
#pragma unroll
                        for (int k = 0; k < EDGE_CH; ++k) acc += ak[k] * w0[h][k];
                        sum[r][h] += gelu_f(acc + b0[h]);
                    }
                }
            }
        }
        float m[EC_NODES][2];
        int cnt[EC_NODES];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) {
            cnt[r] = rp[r + 1] - rp[r];
#pragma unroll
            for (int h = 0; h < 2; ++h) m[r][h] = sum[r][h] / (float)(cnt[r] > 0 ? cnt[r] : 1);
        }
        float acc[EC_NODES][2];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) acc[r][0] = acc[r][1] = 0.0f;
        for (int k = 0; k < C; ++k) {
            const int kr = k < C0 ? 0 : 1, kl = k - 64 * kr;
            float wk[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) wk[h] = have[h] ? s_w2[k * C + lane + 64 * h] : 0.0f;
#pragma unroll
            for (int r = 0; r < EC_NODES; ++r) {
                const float mk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(kr ? m[r][1] : m[r][0]), kl));
#pragma unroll
                for (int h = 0; h < 2; ++h) acc[r][h] += mk * wk[h];
            }
        }
        float ln[EC_NODES][2];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) {
            float cv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) cv[h] = (have[h] && cnt[r] > 0) ? acc[r][h] + b2[h] : 0.0f;
            const float mean = wave_sum(cv[0] + cv[1]) / (float)C;
            float dv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) dv[h] = have[h] ? cv[h] - mean : 0.0f;
            const float rstd = 1.0f / sqrtf(wave_sum(dv[0] * dv[0] + dv[1] * dv[1]) / (float)C + 1e-5f);
#pragma unroll
            for (int h = 0; h < 2; ++h) ln[r][h] = have[h] ? dv[h] * rstd * lw[h] + lb[h] : 0.0f;
        }
        float g[EC_NODES][NC];
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r)
#pragma unroll
            for (int j = 0; j < NC; ++j) g[r][j] = 0.0f;
        for (int k = 0; k < C; ++k) {
            const int kr = k < C0 ? 0 : 1, kl = k - 64 * kr;
            float wk[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) wk[j] = lane + 64 * j < DH ? s_wg[k * DH + lane + 64 * j] : 0.0f;
#pragma unroll
            for (int r = 0; r < EC_NODES; ++r) {
                const float lk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(kr ? ln[r][1] : ln[r][0]), kl));
#pragma unroll
                for (int j = 0; j < NC; ++j) g[r][j] += lk * wk[j];
            }
        }
#pragma unroll
        for (int r = 0; r < EC_NODES; ++r) {
            if (n0 + r >= N) break;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int c = lane + 64 * j;
                if (c < DH) gate[(size_t)(n0 + r) * D + c_off + c] = sigmoid_f(g[r][j] + bg[j]);
            }
        }
    }
}

// ----------------------------------------------------------------- M5: JK fusion
// h_jk = sum_k softmax(jk_logits)_k * states[k]; score = attn . h_jk + b.
template <int D>
__global__ void __launch_bounds__(256) k_jk(int N, int n_states, const float* __restrict__ states,
                                            const float* __restrict__ jk_w /*[n_states] softmaxed*/,
                                            const float* __restrict__ attn_w, const float* __restrict__ attn_b,
                                            float* __restrict__ hjk, float* __restrict__ score) {
    constexpr int LPR = AggCfg<D>::LPR, RPW = AggCfg<D>::RPW, RPB = AggCfg<D>::RPB, D4 = D / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, sl = lane % LPR;
    const int row = blockIdx.x * RPB + wave * RPW + sub;
    const bool act = row < N && sl * 4 < D;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float dot = 0.0f;
    if (act) {
        const size_t o4 = (size_t)row * D4 + sl;
        const size_t stride4 = (size_t)N * D4;
        for (int k = 0; k < n_states; ++k) {
            const float wk = jk_w[k];
            const float4 v = reinterpret_cast<const float4*>(states)[o4 + stride4 * k];
            acc.x += v.x * wk; acc.y += v.y * wk; acc.z += v.z * wk; acc.w += v.w * wk;
        }
        reinterpret_cast<float4*>(hjk)[o4] = acc;
        const float4 aw = reinterpret_cast<const float4*>(attn_w)[sl];
        dot = ((acc.x * aw.x + acc.y * aw.y) + acc.z * aw.z) + acc.w * aw.w;
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (act && sl == 0) score[row] = dot + attn_b[0];
}

// ------------------------------------------------------------- weights

static std::vector<Need> needed_resgcn(const WeightSet& m) {
    const int D = m.D, Dt = m.Dt, Q = m.Q, C = m.C, n = m.n_layers;
    std::vector<Need> v;
    auto add = [&](const std::string& k, int r, int c, int rp, int cp, char layout = 0) {
        v.push_back({k, (int64_t)r * c, r, c, rp, cp, layout});
    };
    auto vec = [&](const std::string& k, int len) { add(k, len, 1, len, 1); };
    auto vecD = [&](const std::string& k) { add(k, Dt, 1, D, 1); };
    vec("in_norm.norm.weight", IN_CH); vec("in_norm.norm.bias", IN_CH);
    vec("in_norm.norm.running_mean", IN_CH); vec("in_norm.norm.running_var", IN_CH);
    add("input_proj.0.weight", Dt, IN_CH, D, IN_CH, 'T'); vecD("input_proj.0.bias");
    vecD("input_proj.1.weight"); vecD("input_proj.1.bias");
    add("prior_booster.0.weight", Q, N_PRIOR, Q, N_PRIOR); vec("prior_booster.0.bias", Q);
    add("prior_booster.2.weight", Dt, Q, D, Q, 'T'); vecD("prior_booster.2.bias");
    add("edge_ctx.encode.0.weight", C, EDGE_CH, C, EDGE_CH); vec("edge_ctx.encode.0.bias", C);
    add("edge_ctx.encode.2.weight", C, C, C, C, 'T'); vec("edge_ctx.encode.2.bias", C);
    vec("edge_ctx.to_gate.0.weight", C); vec("edge_ctx.to_gate.0.bias", C);
    add("edge_ctx.to_gate.1.weight", Dt, C, D, C, 'T'); vecD("edge_ctx.to_gate.1.bias");
    add("sage.lin_l.weight", Dt, Dt, D, D, 'P'); vecD("sage.lin_l.bias"); add("sage.lin_r.weight", Dt, Dt, D, D, 'P');
    vecD("sage_norm.weight"); vecD("sage_norm.bias"); vec("jk_logits", n + 2);
    vecD("ctx.attn.weight"); vec("ctx.attn.bias", 1);
    add("ctx.compress.weight", Dt / 2, Dt, D / 2, D, 'T'); add("ctx.compress.bias", Dt / 2, 1, D / 2, 1);
    add("ctx.expand.weight", Dt, Dt / 2, D, D / 2, 'T'); vecD("ctx.expand.bias");
    vecD("fuse.0.weight"); vecD("fuse.0.bias"); add("fuse.1.weight", Dt, Dt, D, D, 'P'); vecD("fuse.1.bias");
    add("head.weight", N_CLS, Dt, N_CLS, D); vec("head.bias", N_CLS);
    for (int i = 0; i < n; ++i) {
        const std::string s = std::to_string(i);
        vecD("gcn_layers." + s + ".bias");
        add("gcn_layers." + s + ".lin.weight", Dt, Dt, D, D, 'P');
        vecD("norms." + s + ".weight");
        vecD("norms." + s + ".bias");
    }
    return v;
}

// softmax(jk_logits) on the host (model.py:532), same op order as the oracle
static int derive_resgcn(ggc_ctx* ctx, WeightSet& m, std::map<std::string, std::vector<float>>& pw) {
    const std::vector<float>& jl = pw["jk_logits"];
    std::vector<float> w(jl.size());
    float mx = jl[0];
    for (float v : jl) mx = v > mx ? v : mx;
    float s = 0.0f;
    for (size_t k = 0; k < jl.size(); ++k) { w[k] = ggc_expf(jl[k] - mx); s += w[k]; }
    for (size_t k = 0; k < jl.size(); ++k) w[k] = w[k] / s;
    return upload(ctx, m, "#jk_w", w);
}

static const NetSpec RESGCN{"ResGCNNet", "resgcn", &ggc_ctx::resgcn, true, needed_resgcn, derive_resgcn};

// ------------------------------------------------------------ forward

template <int D>
static int forward_t(ggc_ctx* ctx, hipStream_t st, int G, int N, int E, const float* x,
                     const int32_t* edge_src, const int32_t* edge_dst, const float* edge_attr,
                     const int32_t* node_ptr, float* logits, float* probs) {
    WeightSet& m = ctx->resgcn;
    const int n = m.n_layers, n_states = n + 2;
    const size_t ND = (size_t)N * D;
    Csr csr;
    int rc = prepare_csr(ctx, st, G, N, E, edge_src, edge_dst, node_ptr, false, csr);
    if (rc) return rc;
    float* states = scratch_t<float>(ctx, S_STATES, ND * n_states);
    float* gate = scratch_t<float>(ctx, S_GATE, ND);
    float* xw = scratch_t<float>(ctx, S_XW, ND);
    float* agg = scratch_t<float>(ctx, S_AGG, ND);
    float* hjk = scratch_t<float>(ctx, S_HJK, ND);
    float* score = scratch_t<float>(ctx, S_SCORE, (size_t)N);
    float* gvec = scratch_t<float>(ctx, S_GVEC, (size_t)G * D);
    if (!states || !gate || !xw || !agg || !hjk || !score || !gvec) return GGC_E_OOM;
    AggGraphs ag;
    if ((rc = build_agg_pack(ctx, st, N, G, node_ptr, csr.batch, csr.row_ptr, csr.col, ag))) return rc;

    const int wave_blocks = min(cdiv(N, 4), 8 * ctx->n_cu);
    {
        InputW w{devp(m, "in_norm.norm.weight"), devp(m, "in_norm.norm.bias"),
                 devp(m, "in_norm.norm.running_mean"), devp(m, "in_norm.norm.running_var"),
                 devp(m, "#input_proj.0.weightT"), devp(m, "input_proj.0.bias"),
                 devp(m, "input_proj.1.weight"), devp(m, "input_proj.1.bias"),
                 devp(m, "prior_booster.0.weight"), devp(m, "prior_booster.0.bias"),
                 devp(m, "#prior_booster.2.weightT"), devp(m, "prior_booster.2.bias")};
        hipLaunchKernelGGL((k_input<D>), dim3(wave_blocks), dim3(256), 0, st, N, x, w, m.Q, m.Dt, states);
        GGC_LAUNCH_CHECK(ctx);
    }
    {
        EdgeW w{devp(m, "edge_ctx.encode.0.weight"), devp(m, "edge_ctx.encode.0.bias"),
                devp(m, "#edge_ctx.encode.2.weightT"), devp(m, "edge_ctx.encode.2.bias"),
                devp(m, "edge_ctx.to_gate.0.weight"), devp(m, "edge_ctx.to_gate.0.bias"),
                devp(m, "#edge_ctx.to_gate.1.weightT"), devp(m, "edge_ctx.to_gate.1.bias")};
        if constexpr (D <= 128) {
            const size_t eg_lds = sizeof(float) * ((size_t)m.C * m.C + (size_t)m.C * D);            // <= 48 KB (C <= 64, D <= 128)
            hipLaunchKernelGGL((k_edge_gate<D>), dim3(min(cdiv(N, 4 * EC_NODES), 3 * ctx->n_cu)), dim3(256), eg_lds, st, N, csr.row_ptr, csr.eid,
                               edge_attr, w, m.C, gate);
        } else {
            const size_t eg_lds = sizeof(float) * ((size_t)m.C * m.C + (size_t)m.C * (D / 2));      // <= 128 KiB (C <= 128)
            static DeviceOnce attr_set;
            if (attr_set.need(ctx->device)) {
                GGC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_edge_gate_wide<D>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
                attr_set.done(ctx->device);
            }
            hipLaunchKernelGGL((k_edge_gate_wide<D>), dim3(2 * min(cdiv(N, (EGW_THREADS / 64) * EC_NODES), ctx->n_cu)), dim3(EGW_THREADS), eg_lds, st, N,
                               csr.row_ptr, csr.eid, edge_attr, w, m.C, gate);
        }
        GGC_LAUNCH_CHECK(ctx);
    }
    for (int l = 0; l < n; ++l) {
        const std::string s = std::to_string(l);
        const float* h_in = states + ND * l;
        float* h_out = states + ND * (l + 1);
        GemmArgs a{};
        a.A1 = h_in; a.Wp1 = devp(m, "#gcn_layers." + s + ".lin.weight.p");
        a.ln_w = devp(m, "norms." + s + ".weight"); a.ln_b = devp(m, "norms." + s + ".bias");
        a.out = xw; a.Dt = m.Dt;
        if ((rc = launch_gemm<D, 0>(ctx, st, N, a))) return rc;
        if ((rc = launch_aggregate<D, 0>(ctx, st, N, xw, csr.row_ptr, csr.col, csr.dis, devp(m, "gcn_layers." + s + ".bias"),
                                         gate, h_in, h_out, ag)))
            return rc;
    }
    {
        const float* hl = states + ND * n;
        if ((rc = launch_aggregate<D, 1>(ctx, st, N, hl, csr.row_ptr, csr.col, nullptr, nullptr, nullptr, nullptr, agg, ag)))
            return rc;
        GemmArgs a{};
        a.A1 = agg; a.A2 = hl;
        a.Wp1 = devp(m, "#sage.lin_l.weight.p"); a.Wp2 = devp(m, "#sage.lin_r.weight.p");
        a.bias = devp(m, "sage.lin_l.bias");
        a.ep_w = devp(m, "sage_norm.weight"); a.ep_b = devp(m, "sage_norm.bias");
        a.out = states + ND * (n + 1); a.Dt = m.Dt;
        if ((rc = launch_gemm<D, 1>(ctx, st, N, a))) return rc;
    }
    hipLaunchKernelGGL((k_jk<D>), dim3(cdiv(N, AggCfg<D>::RPB)), dim3(256), 0, st, N, n_states, states,
                       devp(m, "#jk_w"), devp(m, "ctx.attn.weight"), devp(m, "ctx.attn.bias"), hjk, score);
    GGC_LAUNCH_CHECK(ctx);
    if ((rc = launch_graph_ctx<D>(ctx, st, G, node_ptr, score, hjk, {devp(m, "#ctx.compress.weightT"), devp(m, "ctx.compress.bias"),
                                                                     devp(m, "#ctx.expand.weightT"), devp(m, "ctx.expand.bias")}, gvec)))
        return rc;
    {
        GemmArgs a{};
        a.A1 = hjk; a.Wp1 = devp(m, "#fuse.1.weight.p");
        a.ln_w = devp(m, "fuse.0.weight"); a.ln_b = devp(m, "fuse.0.bias");
        a.bias = devp(m, "fuse.1.bias");
        a.batch = csr.batch; a.gvec = gvec;
        a.ep_w = devp(m, "head.weight"); a.ep_b = devp(m, "head.bias");
        a.out = logits; a.out2 = probs; a.Dt = m.Dt;
        if ((rc = launch_gemm<D, 2>(ctx, st, N, a))) return rc;
    }
    return GGC_OK;
}

} // namespace ggc

using namespace ggc;

extern "C" {

int ggc_resgcn_configure(ggc_ctx* ctx, int hidden, int n_layers) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, hidden >= 8 && hidden <= 256, GGC_E_UNSUPPORTED,
                "hidden_channels=%d unsupported: the kernels are built for widths from 8 to 256", hidden);
    // widths that are not a multiple of 32 run zero-padded to the next one (k_input: only the LayerNorm statistics see Dt)
    if (int rc = configure(ctx, RESGCN, (hidden + 31) / 32 * 32, hidden, n_layers)) return rc;
    ctx->resgcn.Q = hidden / 4 > 8 ? hidden / 4 : 8;   // model.py:472
    ctx->resgcn.C = hidden / 2 > 8 ? hidden / 2 : 8;   // model.py:123
    return GGC_OK;
}

int ggc_resgcn_load_weight(ggc_ctx* ctx, const char* name, const float* data, int64_t numel) {
    return load_weight(ctx, RESGCN, name, data, numel);
}

int ggc_resgcn_ready(ggc_ctx* ctx) { return check_ready(ctx, RESGCN); }

int ggc_resgcn_forward(ggc_ctx* ctx, ggc_stream stream, int G, int N, int E, const float* x,
                       const int32_t* edge_src, const int32_t* edge_dst, const float* edge_attr,
                       const int32_t* node_ptr, float* logits, float* probs) {
    int rc = begin_forward(ctx, RESGCN, G, N, E, x, edge_src, edge_dst, edge_attr, node_ptr, logits, probs);
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (with_width<32, 64, 96, 128, 160, 192, 224, 256>(ctx->resgcn.D, rc, [&](auto w) {
            return forward_t<decltype(w)::value>(ctx, st, G, N, E, x, edge_src, edge_dst, edge_attr, node_ptr, logits, probs); }))
        return rc;
    return set_err(ctx, GGC_E_UNSUPPORTED, "hidden=%d", ctx->resgcn.D);
}

} // extern "C"
