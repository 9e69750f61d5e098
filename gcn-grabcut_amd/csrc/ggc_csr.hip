// ggc_csr.hip — graph structure shared by the three trimap networks and by training: the destination CSR of an edge
// list (build_csr, stable in edge order) and what a forward derives from it (prepare_csr: dis, the graph of every node,
// the destination of every CSR position).
//
// Kernel map:
//   k_count_dst                                    in-degree of every node
//   k_scan_totals / k_scan_parts / k_scan_blocks   exclusive scan of the degrees -> row_ptr, three small launches
//   k_fill_eid                                     edge ids into their rows, in arrival order
//   k_sort_rows                                    restores edge order inside a row; emits col and dis
//   k_csr_dst                                      destination (row) of every CSR position
//   k_fill_batch                                   graph of every node, from node_ptr
#include "ggc_gnn.h"
#include <algorithm>
#include <cmath>

namespace ggc {

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

} // namespace ggc

using namespace ggc;

extern "C" int ggc_build_csr(ggc_ctx* ctx, ggc_stream stream, int N, int E, const int32_t* edge_src,
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
