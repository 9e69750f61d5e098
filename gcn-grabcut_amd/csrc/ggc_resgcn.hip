// ggc_resgcn.hip — ResGCNNet forward (reference model.py:421-546, eval mode) as
// hand-written gfx950 kernels.
//
// Kernel map:
//   k_input        M1  BatchNorm-eval -> Linear 19->D -> LayerNorm -> GELU -> prior booster
//   k_edge_gate    M2  EdgeContext: edge MLP, mean over incoming edges, LN, Linear, sigmoid
//                      (k_edge_gate_wide above D = 128: two context channels per lane, one gate column half per block)
//   k_gemm<.,0>    M3  LayerNorm(h) @ W^T on f32 MFMA (v_mfma_f32_32x32x2_f32)
//   k_aggregate<.,0>  M3  GCNConv scatter-gather over the destination CSR with the
//                      fused epilogue h + gelu((agg + b) * gate)       <- graded kernel
//   k_aggregate<.,1>  M4  SAGEConv mean aggregation
//   k_gemm<.,1>    M4  lin_l(mean) + lin_r(h), LayerNorm, GELU (two MFMA phases)
//   k_jk           M5  softmax(jk_logits)-weighted sum of the n+2 states + attention score
//   k_graph_ctx    M6  per-graph softmax readout, compress/expand MLP
//   k_gemm<.,2>    M7  (h_jk * g) -> LN -> Linear -> GELU -> head -> softmax
//
// Data layout in HBM: node-major row vectors, f32, D contiguous (512 B rows at
// D=128).  Graphs of a batch are concatenated (PyG Batch semantics); node_ptr
// gives the per-graph ranges.  The destination CSR (row_ptr, col, eid) is
// built once per forward, stable in edge order, and reused by all 8 gathers.
#include "ggc_gnn.h"
#include <atomic>
#include <cmath>

namespace ggc {

// ------------------------------------------------------------------ CSR build

__global__ void k_count_dst(int E, const int32_t* __restrict__ dst, int32_t* __restrict__ cnt) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x)
        atomicAdd(&cnt[dst[e]], 1);
}

// Exclusive scan of cnt[0..n) into out[0..n], out[n] = total, in three small launches: per-block totals of SCAN_BLOCK
// elements, a one-block scan of the totals, and the scan of each block from its base.  (One block over all 154 k rows of a
// batch-256 forward took 233 us; this is a few microseconds per launch.)  part: cdiv(n, SCAN_BLOCK) + 1 words.
constexpr int SCAN_BLOCK = 2048;       // 256 threads x 8 elements
__global__ void __launch_bounds__(256) k_scan_totals(int n, const int32_t* __restrict__ cnt, int32_t* __restrict__ part) {
    __shared__ int32_t red[4];
    const int base = blockIdx.x * SCAN_BLOCK + threadIdx.x * 8;
    int32_t s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (base + j < n) s += cnt[base + j];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(1024) k_scan_parts(int m, int32_t* __restrict__ part) {      // exclusive, in place; part[m] = total
    __shared__ int32_t sh[1024];
    const int tid = threadIdx.x;
    const int chunk = (m + 1023) / 1024, beg = tid * chunk, end = min(beg + chunk, m);
    int32_t s = 0;
    for (int i = beg; i < end; ++i) s += part[i];
    sh[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int32_t v = (tid >= off) ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    int32_t run = (tid == 0) ? 0 : sh[tid - 1];
    for (int i = beg; i < end; ++i) { const int32_t c = part[i]; part[i] = run; run += c; }
    if (tid == 1023) part[m] = sh[1023];
}
__global__ void __launch_bounds__(256) k_scan_blocks(int n, const int32_t* __restrict__ cnt, const int32_t* __restrict__ part,
                                                     int m, int32_t* __restrict__ out) {
    __shared__ int32_t wsum[4];
    const int base = blockIdx.x * SCAN_BLOCK + threadIdx.x * 8, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t c[8], s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = base + j < n ? cnt[base + j] : 0; s += c[j]; }
    int32_t incl = s;                                      // inclusive scan of the threads' sums inside the wave
    for (int o = 1; o < 64; o <<= 1) { const int32_t v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int32_t run = part[blockIdx.x] + (incl - s);
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (int j = 0; j < 8; ++j) { if (base + j < n) out[base + j] = run; run += c[j]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = part[m];
}
static void exclusive_scan(hipStream_t st, int n, const int32_t* cnt, int32_t* part, int32_t* out) {
    const int m = cdiv(std::max(n, 1), SCAN_BLOCK);
    hipLaunchKernelGGL(k_scan_totals, dim3(m), dim3(256), 0, st, n, cnt, part);
    hipLaunchKernelGGL(k_scan_parts, dim3(1), dim3(1024), 0, st, m, part);
    hipLaunchKernelGGL(k_scan_blocks, dim3(m), dim3(256), 0, st, n, cnt, part, m, out);
}

__global__ void k_fill_eid(int E, const int32_t* __restrict__ dst, const int32_t* __restrict__ row_ptr,
                           int32_t* __restrict__ cursor, int32_t* __restrict__ eid) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        const int d = dst[e];
        const int pos = row_ptr[d] + atomicAdd(&cursor[d], 1);
        eid[pos] = e;
    }
}

// One thread per row: restore edge order inside the row (stable CSR), emit col and dis.
__global__ void k_sort_rows(int N, const int32_t* __restrict__ row_ptr, int32_t* __restrict__ eid,
                            const int32_t* __restrict__ src, int32_t* __restrict__ col,
                            float* __restrict__ dis) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < N; r += gridDim.x * blockDim.x) {
        const int beg = row_ptr[r], end = row_ptr[r + 1];
        for (int i = beg + 1; i < end; ++i) {
            const int v = eid[i];
            int j = i - 1;
            while (j >= beg && eid[j] > v) { eid[j + 1] = eid[j]; --j; }
            eid[j + 1] = v;
        }
        for (int i = beg; i < end; ++i) col[i] = src[eid[i]];
        if (dis) dis[r] = 1.0f / sqrtf((float)(end - beg) + 1.0f);
    }
}

// destination (row) of every CSR position: row_ptr[r] <= j < row_ptr[r + 1]
__global__ void __launch_bounds__(256) k_csr_dst(int N, int E, const int32_t* __restrict__ row_ptr, int32_t* __restrict__ csr_dst) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= E) return;
    int lo = 0, hi = N;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (row_ptr[mid] <= j) lo = mid; else hi = mid; }
    csr_dst[j] = lo;
}

__global__ void k_fill_batch(int G, int N, const int32_t* __restrict__ node_ptr, int32_t* __restrict__ batch) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        int lo = 0, hi = G; // find g with node_ptr[g] <= i < node_ptr[g+1]
        while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (node_ptr[mid] <= i) lo = mid; else hi = mid; }
        batch[i] = lo;
    }
}

int build_csr(ggc_ctx* ctx, hipStream_t st, int N, int E, const int32_t* src, const int32_t* dst,
                     int32_t* row_ptr, int32_t* col, int32_t* eid, int32_t* cursor, float* dis) {
    GGC_HIP(ctx, hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)(N + 1), st));
    if (E > 0) {
        hipLaunchKernelGGL(k_count_dst, dim3(min(cdiv(E, 256), 4096)), dim3(256), 0, st, E, dst, cursor);
        GGC_LAUNCH_CHECK(ctx);
    }
    int32_t* scan_part = scratch_t<int32_t>(ctx, S_CSR_SCAN, (size_t)cdiv(std::max(N, 1), SCAN_BLOCK) + 2);
    if (!scan_part) return GGC_E_OOM;
    exclusive_scan(st, N, cursor, scan_part, row_ptr);
    GGC_LAUNCH_CHECK(ctx);
    GGC_HIP(ctx, hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)(N + 1), st));
    if (E > 0) {
        hipLaunchKernelGGL(k_fill_eid, dim3(min(cdiv(E, 256), 4096)), dim3(256), 0, st, E, dst, row_ptr, cursor, eid);
        GGC_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(k_sort_rows, dim3(min(cdiv(N, 256), 4096)), dim3(256), 0, st, N, row_ptr, eid, src, col, dis);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

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

// ---------------------------------------------------------- M3/M4/M7: MFMA GEMM
// out[N,D] = op(A)[N,D] @ W^T, f32 in / f32 accumulate on v_mfma_f32_32x32x2_f32.
// A block is 4 waves; each wave owns 32 rows x D columns (T = D/32 accumulator
// tiles).  The k index is permuted so that lane half hk = lane>>5 covers
// k in [hk*D/2, (hk+1)*D/2): each lane then reads one contiguous half-row of A
// (float4 loads) and W is pre-packed on the host as Wp[s/4][t][lane][s%4] =
// W[32t + (lane&31)][hk*D/2 + s], staged once per block into LDS and read with
// conflict-free ds_read_b128.  The modes and their arguments (GemmArgs) are listed in ggc_gnn.h.

#ifdef GEMM_TRACE     // experiment build: per-wave phase stamps of k_gemm<128, 0> kept in SGPRs (no scheduling fences)
__device__ unsigned long long g_gemm_trace[8192 * 8];
#define GEMM_STAMP(i) do { if (D == 128 && MODE == 0) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[i]) :: "memory"); } while (0)
#else
#define GEMM_STAMP(i) do {} while (0)
#endif
template <int D, int MODE>
__global__ void __launch_bounds__(256) k_gemm(int N, GemmArgs g) {
#ifdef GEMM_TRACE
    unsigned long long stamp[7] = {0, 0, 0, 0, 0, 0, 0};
#endif
    constexpr int T = D / 32, KH = D / 2;
    extern __shared__ float4 smem4[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hk = lane >> 5, li = lane & 31;
    const int r0 = (blockIdx.x * 4 + wave) * 32;
    const int row = min(r0 + li, N - 1);
    GEMM_STAMP(0);

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
        GEMM_STAMP(1);

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
#ifdef GEMM_TRACE
            if (D == 128 && MODE == 0) asm volatile("s_nop 0" :: "v"(s1));       // the stamp below waits for the row sum, i.e. for the loads
#endif
            GEMM_STAMP(2);
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
#ifdef GEMM_TRACE
        if (D == 128 && MODE == 0) asm volatile("s_nop 0" :: "v"(a[0]), "v"(a[KH - 1]));
#endif
        GEMM_STAMP(3);
        // Consecutive MFMAs go to different accumulators (the T column tiles of one k step); each accumulator still sees its
        // k steps in the same order.  (Phase stamps, GEMM_TRACE: the MFMA loops of the two waves of a SIMD never overlap, in this
        // order or with the four k steps of a B fragment back to back on one accumulator, and the other wave's LayerNorm
        // crawls meanwhile — the f32 MFMA runs at the vector rate and leaves the SIMD's vector issue little room.)
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

#ifdef GEMM_TRACE
    if (D == 128 && MODE == 0) asm volatile("s_nop 0" :: "v"(acc[0][0]), "v"(acc[T - 1][15]));
#endif
    GEMM_STAMP(4);
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
#ifdef GEMM_TRACE
    GEMM_STAMP(5);
    __builtin_amdgcn_s_waitcnt(0);
    GEMM_STAMP(6);
    if (D == 128 && MODE == 0 && lane == 0 && blockIdx.x * 4 + wave < 8192) {
        unsigned long long* o = g_gemm_trace + (blockIdx.x * 4 + wave) * 8;
        for (int i = 0; i < 7; ++i) o[i] = stamp[i];
        o[7] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |
               ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32);
    }
#endif
}

// ------------------------------------------------- M3/M4: CSR scatter-gather
// Destination-major gather: LPR lanes x float4 cover one D-wide row, a wave
// handles 64/LPR rows, a block of 4 waves handles RPB consecutive rows.  Blocks
// are remapped so each XCD walks a contiguous range of rows (= whole images):
// the ~11 re-reads of every xw row then hit that XCD's L2.  Neighbours are
// summed in CSR (= edge) order with one rounding per multiply and per add, the
// self loop last, exactly like the oracle.
//   MODE 0 (GCNConv): out = sum dis[j] dis[i] xw[j] + dis[i]^2 xw[i] + bias,
//                     fused epilogue h + gelu(out * gate) when gate != null.
//   MODE 1 (SAGE mean): out = sum xw[j] / max(cnt, 1).
template <int D> struct AggCfg {
    static constexpr int LPR = (D <= 32) ? 8 : (D <= 64) ? 16 : (D <= 128) ? 32 : 64;    // D > 128: a wave per row
    static constexpr int RPW = 64 / LPR;
    static constexpr int RPB = 4 * RPW;
};

__device__ __forceinline__ void fma4(float4& acc, float w, const float4& v) {
    acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
}

template <int D, int MODE>
__global__ void __launch_bounds__(1024) k_aggregate(int N, const float* __restrict__ xw,
                                                   const int32_t* __restrict__ row_ptr,
                                                   const int32_t* __restrict__ col,
                                                   const float* __restrict__ dis,
                                                   const float* __restrict__ bias,
                                                   const float* __restrict__ gate,
                                                   const float* __restrict__ h,
                                                   float* __restrict__ out) {
    constexpr int LPR = AggCfg<D>::LPR, RPW = AggCfg<D>::RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, sl = lane % LPR;
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int row = blk * (RPW * (int)(blockDim.x >> 6)) + wave * RPW + sub;
    // The sub-group of LPR lanes that owns a row first loads up to LPR column indices (and their
    // dis weights) with ONE coalesced load each, then broadcasts them by shuffle: the dependent
    // chain per row is row_ptr -> col -> dis -> rows instead of one col/dis round trip per
    // neighbour, and up to 8 neighbour rows are in flight per lane.  Summation order is unchanged
    // (CSR = edge order, self loop last).
    const bool rvalid = row < N, cvalid = sl * 4 < D;
    const int rowc = rvalid ? row : 0, slc = cvalid ? sl : 0;
    const int beg = rvalid ? row_ptr[rowc] : 0, end = rvalid ? row_ptr[rowc + 1] : 0;
    const float di = (MODE == 0) ? dis[rowc] : 1.0f;
    constexpr int D4 = D / 4;
    const float4* xw4 = reinterpret_cast<const float4*>(xw) + slc;
    const size_t o4 = (size_t)rowc * D4 + slc;
    float4 self = make_float4(0.f, 0.f, 0.f, 0.f), gt = self, hv = self;
    if (MODE == 0) {                     // epilogue operands: issue their loads before the gather
        self = xw4[(size_t)rowc * D4];
        if (gate) { gt = reinterpret_cast<const float4*>(gate)[o4]; hv = reinterpret_cast<const float4*>(h)[o4]; }
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = beg; base < end; base += LPR) {
        const int n = min(LPR, end - base);
        int c = 0;
        float w = 0.0f;
        if (sl < n) { c = col[base + sl]; if (MODE == 0) w = dis[c] * di; }
        for (int k = 0; k < n; k += 8) {
            float4 v[8];
            float wk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int kk = min(k + u, n - 1);
                const int j = __shfl(c, kk, LPR);
                wk[u] = __shfl(w, kk, LPR);
                if (k + u < n) v[u] = xw4[(size_t)j * D4];     // predicated: no duplicate row fetches in the tail
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (k + u < n) {
                    if (MODE == 0) fma4(acc, wk[u], v[u]);
                    else { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
                }
            }
        }
    }
    if (MODE == 0) {
        fma4(acc, di * di, self);
        if (bias) {
            const float4 b = reinterpret_cast<const float4*>(bias)[slc];
            acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
        }
        if (gate) {
            acc.x = hv.x + gelu_f(acc.x * gt.x); acc.y = hv.y + gelu_f(acc.y * gt.y);
            acc.z = hv.z + gelu_f(acc.z * gt.z); acc.w = hv.w + gelu_f(acc.w * gt.w);
        }
    } else {
        const int cnt = end - beg;
        const float c = (float)(cnt > 0 ? cnt : 1);
        acc.x /= c; acc.y /= c; acc.z /= c; acc.w /= c;
    }
    if (rvalid && cvalid) reinterpret_cast<float4*>(out)[o4] = acc;
}

// Graph-resident form of the gather (the one the forward pass uses).  PMC profiling of the kernel
// above shows ideal HBM traffic (FETCH+WRITE == algorithmic bytes) but the per-CU L1/texture path
// ~76 % busy and two thirds of the L2 requests being re-reads: every neighbour row costs a 16-cycle
// slot of the 64 B/clk vector-memory pipe.  The graphs of a batch are independent and small (about
// 600 superpixels), so a block owns ONE graph and a SW-float column slice of the feature matrix:
// it copies its [n_g, SW] slice of xw (and the graph's dis) into LDS once by LDS-DMA (128-B segments,
// every byte of xw is read from memory exactly once) and then serves every neighbour row and the
// self loop by ds_read_b128 on the 256 B/clk LDS pipe.  Two blocks share a CU (80 KiB each), so one
// block's fill overlaps the other's gather.  The D/SW slices of one graph run on the same XCD and
// share the CSR through its L2.  A graph with more than CAP nodes, or an edge that leaves its graph,
// falls back to global loads per block / per row.  Arithmetic and summation order are those of
// k_aggregate.

// Block shape of the 32-float slices (round 3, bench batch, us per launch of the gated kernel on one box): 512 threads with 8
// neighbour rows per batch of LDS reads and the epilogue operands two rows ahead (116 VGPRs, 16 waves per CU) 60.3-62.0;
// 256 threads 72-75 whatever the prefetch depth (2 / 4 / 6 rows): the kernel is short of WAVES, not of bytes in flight;
// 768 threads, 2 rows per batch (76 VGPRs, 24 waves) 59.3-59.5; 1024 threads, 2 rows per batch, one row ahead (62 VGPRs, the
// full 32 waves per CU) 57.6-58.0.  Anything that spills (768 / 1024 threads with 4 or 8 rows per batch) loses 15 us.
#ifndef AGG_THREADS
#define AGG_THREADS 1024
#endif
#ifndef AGG_PF
#define AGG_PF 1
#endif
#ifndef AGG_UB
#define AGG_UB 2
#endif
// (16-float slices — 64-byte fill segments, three 52-KB blocks per CU, meant for graphs of 620-782 nodes — took 143-150 us on
// the same batch against 96 us for the direct gather k_aggregate: that route is gone, such batches gather directly.)
template <int SW> struct AggGraph {
    static_assert(SW == 32, "one slice width is built");
    static constexpr int T = AGG_THREADS, NW = T / 64;                         // threads per block
    static constexpr int PF = AGG_PF;                                          // epilogue rows in flight ahead of the gather
    static constexpr int UB = AGG_UB;                                          // neighbour rows per batch of LDS reads
    static constexpr int LPR = SW / 4, RPW = 64 / LPR, RPP = NW * RPW;         // rows per pass of the block
    static constexpr int LDS = 80 * 1024;                                      // 2 blocks per CU
    static constexpr int OCC = 2 * T / 256 < 8 ? 2 * T / 256 : 8;              // waves per SIMD the blocks of a CU need
    static constexpr int CAP_LDS = (LDS - SW * 4 - 4) / (SW * 4 + 4);          // tile row + dis entry, one zero row
    static constexpr int CAP = CAP_LDS < 1023 ? CAP_LDS : 1023;                // 10-bit row offsets in the packed columns
    static constexpr int K = (CAP + RPP - 1) / RPP;                            // passes for a full tile
    static constexpr int FILL = (CAP * LPR + T - 1) / T;                       // LDS-DMA pieces per thread
};

// broadcast lane U of every group of W lanes (W = 4 or 8): ds_swizzle, no address VGPR and no VALU
template <int W, int U> __device__ __forceinline__ int group_bcast(int v) {
    return __builtin_amdgcn_ds_swizzle(v, (0x1f & ~(W - 1)) | (U << 5));
}
template <int W, int U> __device__ __forceinline__ float group_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (0x1f & ~(W - 1)) | (U << 5)));
}
template <int W, int U0, int NU, typename F> __device__ __forceinline__ void unroll_bcast(F&& f) {
    if constexpr (NU > 0) { f(std::integral_constant<int, U0>{}); unroll_bcast<W, U0 + 1, NU - 1>(f); }
}

// Per (row, lane) column words of the graph-resident gather, built once per forward pass and shared by
// every layer (7 aggregations read the same CSR): for lane sl of the LPR lanes that own a row,
//   bits 0-9 / 10-19: tile row (offset inside the graph) of neighbours sl and LPR + sl, ZROW when there is none
//   bits 20+        : n + 1, or 0 for an irregular row (more than 2 * LPR neighbours, or an edge that leaves
//                     the graph) which the kernel handles by the generic route
// One coalesced load per row replaces the dependent row_ptr -> col hops in the gather kernel.
template <int SW>
__global__ void __launch_bounds__(256) k_agg_pack(int N, const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ batch,
                                                  const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                  int32_t* __restrict__ pack) {
    constexpr int LPR = AggGraph<SW>::LPR, ZROW = AggGraph<SW>::CAP;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // N * LPR is a multiple of LPR: whole groups stay together
    const int row = min(i / LPR, N - 1), sl = i % LPR;
    const int g = batch[row];
    const int g0 = node_ptr[g], n_g = node_ptr[g + 1] - g0;
    const int beg = row_ptr[row], n = row_ptr[row + 1] - beg;
    bool regular = n <= 2 * LPR;
    int pk = 0;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const bool have = nb * LPR + sl < n;
        const int off = have ? col[beg + nb * LPR + sl] - g0 : 0;
        regular = regular && (unsigned)off < (unsigned)n_g;
        pk |= (have ? off & 1023 : ZROW) << (10 * nb);
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
        const int other = __shfl_xor((int)regular, o, LPR);     // every lane takes part: no short-circuit around the shuffle
        regular = regular && other != 0;
    }
    if (i < N * LPR) pack[i] = regular ? pk | (n + 1) << 20 : (ZROW | ZROW << 10);
}

// One row of the column slice by the generic route (columns, weights and out-of-tile rows from global memory).
template <int D, int MODE, int SW>
__device__ __forceinline__ void agg_row_generic(int row, int g0, int n_g, const float4* tile, const float4* __restrict__ xw4g,
                                                const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                const float* __restrict__ dis, const float4& bias4,
                                                const float* __restrict__ gate, const float* __restrict__ h,
                                                float* __restrict__ out, int s, int sl) {
    constexpr int LPR = SW / 4, D4 = D / 4;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    const float di = (MODE == 0) ? dis[row] : 1.0f;
    const size_t o4 = (size_t)row * D4 + s * LPR + sl;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = beg; base < end; base += LPR) {
        const int m = min(LPR, end - base);
        int c = g0;
        float w = 0.0f;
        if (sl < m) { c = col[base + sl]; if (MODE == 0) w = dis[c] * di; }
        for (int u = 0; u < m; ++u) {
            const int j = __shfl(c, u, LPR);
            const float wu = __shfl(w, u, LPR);
            const int off = j - g0;
            const float4 v = (tile && (unsigned)off < (unsigned)n_g) ? tile[off * LPR + sl] : xw4g[(size_t)j * D4 + sl];
            if (MODE == 0) fma4(acc, wu, v);
            else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
        }
    }
    if (MODE == 0) {
        fma4(acc, di * di, tile ? tile[(row - g0) * LPR + sl] : xw4g[(size_t)row * D4 + sl]);
        acc.x += bias4.x; acc.y += bias4.y; acc.z += bias4.z; acc.w += bias4.w;
        if (gate) {
            const float4 gt = reinterpret_cast<const float4*>(gate)[o4], hv = reinterpret_cast<const float4*>(h)[o4];
            acc.x = hv.x + gelu_f(acc.x * gt.x); acc.y = hv.y + gelu_f(acc.y * gt.y);
            acc.z = hv.z + gelu_f(acc.z * gt.z); acc.w = hv.w + gelu_f(acc.w * gt.w);
        }
    } else {
        const int cnt = end - beg;
        const float cf = (float)(cnt > 0 ? cnt : 1);
        acc.x /= cf; acc.y /= cf; acc.z /= cf; acc.w /= cf;
    }
    reinterpret_cast<float4*>(out)[o4] = acc;
}

// Every byte of this kernel is touched once: the tile fill (LDS-DMA), the gate / h stream of the epilogue and the output are
// issued NON-TEMPORAL (bit 4 / 2 / 1).  Measured on configs[1] at batch 256, us per launch: 0: 56.6-57.1, 1: 55.9, 2: 57.6,
// 3: 55.3, 4: 55.8, 7: 55.2 (the forward as a whole is unchanged: the next kernel finds h' in HBM either way).
#ifndef AGG_NT
#define AGG_NT 7
#endif
template <int D, int MODE, int SW, bool GATED>
__global__ void __launch_bounds__(AggGraph<SW>::T, AggGraph<SW>::OCC) k_aggregate_graph(int G, const int32_t* __restrict__ node_ptr,
                                                            const float* __restrict__ xw,
                                                            const int32_t* __restrict__ row_ptr,
                                                            const int32_t* __restrict__ col,
                                                            const int32_t* __restrict__ pack,
                                                            const float* __restrict__ dis,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ gate,
                                                            const float* __restrict__ h,
                                                            float* __restrict__ out) {
    using C = AggGraph<SW>;
    constexpr int LPR = C::LPR, RPW = C::RPW, RPP = C::RPP, CAP = C::CAP, K = C::K, FILL = C::FILL, NS = D / SW, D4 = D / 4, T = C::T;
    constexpr int NB = 2;                                  // column batches kept in registers (NB * LPR neighbours)
    constexpr int PF = C::PF;                              // epilogue rows kept in flight ahead of the gather
    constexpr int ZROW = CAP;                              // all-zero tile row (and dis entry) the padding lanes point at
    static_assert(D % SW == 0, "slice width must divide D");
    static_assert(!GATED || MODE == 0, "the gated epilogue belongs to GCNConv");
    extern __shared__ float4 tile[];                       // [CAP + 1][LPR] float4, then dis_l[CAP + 1]
    float* dis_l = reinterpret_cast<float*>(tile + (CAP + 1) * LPR);
    const v4f* tile4 = reinterpret_cast<const v4f*>(tile);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);                    // tells the compiler it is wave-uniform
    const int sub = lane / LPR, sl = lane % LPR;
    const int s = ((int)blockIdx.x >> 3) % NS;                                  // blocks b, b+8, ... share an XCD
    const int g = ((int)blockIdx.x / (8 * NS)) * 8 + ((int)blockIdx.x & 7);
    if (g >= G) return;
    const int g0 = node_ptr[g], n_g = node_ptr[g + 1] - g0;
    if (n_g <= 0) return;
    const float4* xw4g = reinterpret_cast<const float4*>(xw) + s * LPR;         // column slice
    const v4f* gate4 = reinterpret_cast<const v4f*>(gate) + s * LPR + sl;
    const v4f* h4 = reinterpret_cast<const v4f*>(h) + s * LPR + sl;
    const int r0 = wave * RPW + sub;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == 0 && bias) bias4 = reinterpret_cast<const float4*>(bias)[s * LPR + sl];
    if (n_g > CAP) {                                       // graph larger than the tile: everything from global memory
        for (int r = r0; r < n_g; r += RPP)
            agg_row_generic<D, MODE, SW>(g0 + r, g0, n_g, nullptr, xw4g, row_ptr, col, dis, bias4, gate, h, out, s, sl);
        return;
    }
    // ---- preamble: the packed column words of this block's rows (k_agg_pack) and the tile fill are independent
    // loads, so the block waits for one memory round trip; the gather then touches LDS only.
    int cp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int r = r0 + k * RPP;
        cp[k] = (r < n_g) ? pack[(size_t)(g0 + r) * LPR + sl] : (ZROW | ZROW << 10 | 1 << 20);
    }
    // tile + dis fill: LDS-DMA, no registers; a wave instruction writes 64 consecutive elements
#pragma unroll
    for (int f = 0; f < FILL; ++f) {
        const int i = tid + f * T;
        if (i < n_g * LPR)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xw4g + (size_t)(g0 + i / LPR) * D4 + i % LPR),
                                             (__attribute__((address_space(3))) void*)(tile + f * T + wave * 64), 16, 0, (AGG_NT & 4) ? 2 : 0);
    }
    if (MODE == 0) {
#pragma unroll
        for (int f = 0; f < (CAP + T - 1) / T; ++f) {
            const int i = tid + f * T;
            if (i < n_g)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(dis + g0 + i),
                                                 (__attribute__((address_space(3))) void*)(dis_l + f * T + wave * 64), 4, 0, 0);
        }
    }
    if (tid < LPR) tile[ZROW * LPR + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid == LPR) dis_l[ZROW] = 0.0f;
    // The gated epilogue streams gate and h from HBM: PF rows ahead are kept in flight, unconditionally (row
    // clamped into the graph) so that the main loop is straight-line code and its waits stay counted.
    v4f gtq[K], hvq[K];
    if (GATED) {
#pragma unroll
        for (int k = 0; k < PF && k < K; ++k) {
            const size_t p4 = (size_t)(g0 + min(r0 + k * RPP, n_g - 1)) * D4;
            if (AGG_NT & 2) { gtq[k] = __builtin_nontemporal_load(&gate4[p4]); hvq[k] = __builtin_nontemporal_load(&h4[p4]); }
            else { gtq[k] = gate4[p4]; hvq[k] = h4[p4]; }
        }
    }
    __syncthreads();
    // ---- gather: LDS only, no global load besides the epilogue prefetch; no predication either, a padding
    // lane adds 0 * 0 from the zero row (acc starts at +0 and x + (+-0) == x, so the sum is unchanged)
    bool irregular = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k * RPP + wave_s * RPW >= n_g) break;          // scalar: no exec-masked region around the body, waits stay counted
        {
            const int r = r0 + k * RPP;
            const bool valid = r < n_g;
            const int rc = valid ? r : n_g - 1;
            if (GATED && k + PF < K) {
                const size_t p4 = (size_t)(g0 + min(r + PF * RPP, n_g - 1)) * D4;
                if (AGG_NT & 2) { gtq[k + PF] = __builtin_nontemporal_load(&gate4[p4]); hvq[k + PF] = __builtin_nontemporal_load(&h4[p4]); }
                else { gtq[k + PF] = gate4[p4]; hvq[k + PF] = h4[p4]; }
            }
            const float di = (MODE == 0) ? dis_l[rc] : 1.0f;
            const int code = cp[k] >> 20;
            const int n = code > 0 ? code - 1 : 0;
            v4f acc = 0.0f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if (nb == 0 || nb * LPR < n) {
                    const int myoff = (cp[k] >> (10 * nb)) & 1023;
                    const float myw = (MODE == 0) ? dis_l[myoff] * di : 0.0f;
                    constexpr int UB = C::UB < LPR ? C::UB : LPR;
                    unroll_bcast<1, 0, LPR / UB>([&](auto ub) {
                        v4f v[UB];
                        float wk[UB];
                        unroll_bcast<LPR, 0, UB>([&](auto u) {
                            v[u] = tile4[group_bcast<LPR, ub * UB + u>(myoff) * LPR + sl];
                            if (MODE == 0) wk[u] = group_bcast<LPR, ub * UB + u>(myw);
                        });
#pragma unroll
                        for (int u = 0; u < UB; ++u) {
                            if (MODE == 0) acc += wk[u] * v[u];
                            else acc += v[u];
                        }
                    });
                }
            }
            if (MODE == 0) {
                acc += (di * di) * tile4[rc * LPR + sl];
                acc += (v4f){bias4.x, bias4.y, bias4.z, bias4.w};
                if (GATED) acc = hvq[k] + gelu4_f(acc * gtq[k]);
            } else {
                acc /= (float)(n > 0 ? n : 1);
            }
            if (valid && code > 0) {
                v4f* o4p = reinterpret_cast<v4f*>(out) + (size_t)(g0 + r) * D4 + s * LPR + sl;
                if (AGG_NT & 1) __builtin_nontemporal_store(acc, o4p); else *o4p = acc;
            }
            irregular = irregular || (valid && code == 0);
        }
    }
    if (__any(irregular)) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int r = r0 + k * RPP;
            if (r < n_g && (cp[k] >> 20) == 0)
                agg_row_generic<D, MODE, SW>(g0 + r, g0, n_g, tile, xw4g, row_ptr, col, dis, bias4, GATED ? gate : nullptr, h, out, s, sl);
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

// ------------------------------------------------------ M6: per-graph readout
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

// ------------------------------------------------------------ launch helpers

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
#ifdef GEMM_TRACE
    if (D == 128 && MODE == 0 && std::getenv("GGC_GEMM_TRACE")) {
        static std::vector<unsigned long long> host(8192 * 8);
        int occ = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(&k_gemm<D, MODE>), 256, lds);
        (void)hipDeviceSynchronize();
        (void)hipMemcpyFromSymbol(host.data(), HIP_SYMBOL(g_gemm_trace), host.size() * 8);
        if (FILE* f = std::fopen(std::getenv("GGC_GEMM_TRACE"), "ab")) {
            const long long n = std::min(cdiv(N, 128) * 4, 8192);
            std::fwrite(&n, 8, 1, f); std::fwrite(host.data(), 8, (size_t)n * 8, f); std::fclose(f);
        }
        std::fprintf(stderr, "k_gemm<128,0> trace: blocks per CU %d\n", occ);
    }
#endif
    return GGC_OK;
}

template <int D, int MODE, int SW, bool GATED>
static int launch_aggregate_graph_t(ggc_ctx* ctx, hipStream_t st, int G, const int32_t* node_ptr, const int32_t* pack,
                                    const float* xw, const int32_t* row_ptr, const int32_t* col, const float* dis,
                                    const float* bias, const float* gate, const float* h, float* out) {
    static DeviceOnce attr_set;
    if (attr_set.need(ctx->device)) {
        GGC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_aggregate_graph<D, MODE, SW, GATED>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, AggGraph<SW>::LDS));
        attr_set.done(ctx->device);
    }
    hipLaunchKernelGGL((k_aggregate_graph<D, MODE, SW, GATED>), dim3(cdiv(G, 8) * 8 * (D / SW)), dim3(AggGraph<SW>::T), AggGraph<SW>::LDS, st,
                       G, node_ptr, xw, row_ptr, col, pack, dis, bias, gate, h, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

// Column-slice width of the graph-resident gather for G graphs with N nodes in total: 32 when the [nodes-per-graph, 32]
// tile fits half a CU's LDS with a little head-room over the mean graph size (a larger graph falls back per block);
// 0 = use the direct gather.
static int agg_graph_slice(int N, int G) {
    if (G <= 0 || knobs().agg_direct) return 0;
    const double want = 1.02 * (double)N / G;
    return want <= AggGraph<32>::CAP ? 32 : 0;
}

static int build_agg_pack(ggc_ctx* ctx, hipStream_t st, int N, int G, const int32_t* node_ptr, const int32_t* batch,
                          const int32_t* row_ptr, const int32_t* col, AggGraphs& ag) {
    ag = AggGraphs{};
    const int sw = agg_graph_slice(N, G);
    if (!sw || N <= 0) return GGC_OK;
    const int lpr = sw / 4;
    int32_t* pack = scratch_t<int32_t>(ctx, S_AGG_PACK, (size_t)N * lpr);
    if (!pack) return GGC_E_OOM;
    hipLaunchKernelGGL(k_agg_pack<32>, dim3(cdiv(N * lpr, 256)), dim3(256), 0, st, N, node_ptr, batch, row_ptr, col, pack);
    GGC_LAUNCH_CHECK(ctx);
    ag.G = G; ag.sw = sw; ag.node_ptr = node_ptr; ag.pack = pack;
    return GGC_OK;
}

template <int D, int MODE, int SW>
static int launch_aggregate_graph(ggc_ctx* ctx, hipStream_t st, const AggGraphs& ag, const float* xw,
                                  const int32_t* row_ptr, const int32_t* col, const float* dis, const float* bias,
                                  const float* gate, const float* h, float* out) {
    if constexpr (MODE == 0) {
        if (gate)
            return launch_aggregate_graph_t<D, MODE, SW, true>(ctx, st, ag.G, ag.node_ptr, ag.pack, xw, row_ptr, col, dis, bias, gate, h, out);
    }
    return launch_aggregate_graph_t<D, MODE, SW, false>(ctx, st, ag.G, ag.node_ptr, ag.pack, xw, row_ptr, col, dis, bias, nullptr, nullptr, out);
}

template <int D, int MODE>
int launch_aggregate(ggc_ctx* ctx, hipStream_t st, int N, const float* xw, const int32_t* row_ptr, const int32_t* col,
                     const float* dis, const float* bias, const float* gate, const float* h, float* out, const AggGraphs& ag) {
    ProfScope prof(ctx, st, MODE == 0 ? "gcn_aggregate" : "sage_aggregate");
    if (ag.sw == 32) return launch_aggregate_graph<D, MODE, 32>(ctx, st, ag, xw, row_ptr, col, dis, bias, gate, h, out);
    constexpr int threads = 256;
    const int rows_per_block = AggCfg<D>::RPW * (threads / 64);
    hipLaunchKernelGGL((k_aggregate<D, MODE>), dim3(cdiv(N, rows_per_block)), dim3(threads), 0, st,
                       N, xw, row_ptr, col, dis, bias, gate, h, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

template <int D>
int launch_graph_ctx(ggc_ctx* ctx, hipStream_t st, int G, const int32_t* node_ptr, const float* score, const float* hjk,
                     const CtxW& w, float* gvec) {
    hipLaunchKernelGGL((k_graph_ctx<D>), dim3(G), dim3(256), 0, st, node_ptr, score, hjk, w, gvec);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

int prepare_csr(ggc_ctx* ctx, hipStream_t st, int G, int N, int E, const int32_t* edge_src, const int32_t* edge_dst,
                const int32_t* node_ptr, bool with_dst, Csr& g) {
    g = Csr{};
    g.row_ptr = scratch_t<int32_t>(ctx, S_CSR_ROWPTR, (size_t)N + 1);
    g.col = scratch_t<int32_t>(ctx, S_CSR_COL, (size_t)E);
    g.eid = scratch_t<int32_t>(ctx, S_CSR_EID, (size_t)E);
    int32_t* cursor = scratch_t<int32_t>(ctx, S_CSR_CURSOR, (size_t)N + 1);
    g.dis = scratch_t<float>(ctx, S_DIS, (size_t)N);
    if (node_ptr) g.batch = scratch_t<int32_t>(ctx, S_BATCH, (size_t)N);
    if (with_dst) g.dst = scratch_t<int32_t>(ctx, S_AGG_PACK, (size_t)E);
    if (!g.row_ptr || !g.col || !g.eid || !cursor || !g.dis || (node_ptr && !g.batch) || (with_dst && !g.dst)) return GGC_E_OOM;
    int rc = build_csr(ctx, st, N, E, edge_src, edge_dst, g.row_ptr, g.col, g.eid, cursor, g.dis);
    if (rc) return rc;
    if (with_dst && E > 0) {
        hipLaunchKernelGGL(k_csr_dst, dim3(cdiv(E, 256)), dim3(256), 0, st, N, E, g.row_ptr, g.dst);
        GGC_LAUNCH_CHECK(ctx);
    }
    if (node_ptr) {
        hipLaunchKernelGGL(k_fill_batch, dim3(min(cdiv(N, 256), 4096)), dim3(256), 0, st, G, N, node_ptr, g.batch);
        GGC_LAUNCH_CHECK(ctx);
    }
    return GGC_OK;
}

// the (D, MODE) pairs GCNTrimapNet (ggc_gcnnet.hip) and GATTrimapNet (ggc_gat.hip) launch
#define GGC_GEMM(D, MODE) template int launch_gemm<D, MODE>(ggc_ctx*, hipStream_t, int, const GemmArgs&);
GGC_GEMM(32, 3) GGC_GEMM(64, 3) GGC_GEMM(96, 3) GGC_GEMM(128, 3) GGC_GEMM(256, 3)
GGC_GEMM(32, 4) GGC_GEMM(64, 4) GGC_GEMM(128, 4) GGC_GEMM(256, 4)
#undef GGC_GEMM
#define GGC_AGG(D) template int launch_aggregate<D, 0>(ggc_ctx*, hipStream_t, int, const float*, const int32_t*, const int32_t*, \
                                                       const float*, const float*, const float*, const float*, float*, const AggGraphs&);
GGC_AGG(32) GGC_AGG(64) GGC_AGG(96) GGC_AGG(128)
#undef GGC_AGG
#define GGC_CTX(D) template int launch_graph_ctx<D>(ggc_ctx*, hipStream_t, int, const int32_t*, const float*, const float*, const CtxW&, float*);
GGC_CTX(32) GGC_CTX(64) GGC_CTX(128) GGC_CTX(256)
#undef GGC_CTX

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

int ggc_build_csr(ggc_ctx* ctx, ggc_stream stream, int N, int E, const int32_t* edge_src,
                  const int32_t* edge_dst, int32_t* row_ptr, int32_t* col, float* dis) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && E >= 0 && row_ptr && (E == 0 || (edge_src && edge_dst && col)), GGC_E_INVALID_ARG,
                "bad arguments");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* eid = scratch_t<int32_t>(ctx, S_CSR_EID, (size_t)E);
    int32_t* cursor = scratch_t<int32_t>(ctx, S_CSR_CURSOR, (size_t)N + 1);
    if (!eid || !cursor) return GGC_E_OOM;
    return build_csr(ctx, reinterpret_cast<hipStream_t>(stream), N, E, edge_src, edge_dst, row_ptr, col, eid,
                     cursor, dis);
}

int ggc_gcn_aggregate(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* xw,
                      const int32_t* row_ptr, const int32_t* col, const float* dis, const float* bias,
                      const float* gate, const float* h, float* h_out) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && xw && row_ptr && col && dis && h_out, GGC_E_INVALID_ARG, "bad arguments");
    GGC_REQUIRE(ctx, (gate == nullptr) == (h == nullptr), GGC_E_INVALID_ARG, "gate and h must be given together");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if (with_width<32, 64, 96, 128, 160, 192, 224, 256>(D, rc, [&](auto w) {
            return launch_aggregate<decltype(w)::value, 0>(ctx, st, N, xw, row_ptr, col, dis, bias, gate, h, h_out); }))
        return rc;
    return set_err(ctx, GGC_E_UNSUPPORTED, "D=%d unsupported (a multiple of 32 from 32 to 256)", D);
}

} // extern "C"
