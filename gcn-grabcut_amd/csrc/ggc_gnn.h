// ggc_gnn.h — shared host plumbing of the three trimap networks (ggc_resgcn.hip: ResGCNNet, ggc_gcnnet.hip:
// GCNTrimapNet, ggc_gat.hip: GATTrimapNet): the weight registry, the host-side weight layouts and the launchers of the
// kernels more than one network uses (ggc_csr.hip: graph structure, ggc_gnn_dense.hip: MFMA GEMM and per-graph readout,
// ggc_gnn_gather.hip: the CSR gather; ggc_gcnnet.hip: the edge gate of the other two).  The build is not relocatable
// device code, so a kernel can only be launched from the file that defines it: the launchers are declared here and
// explicitly instantiated there, one entry per user.
#pragma once
#include "ggc_internal.h"

namespace ggc {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int IN_CH = 19, EDGE_CH = 5, N_PRIOR = 3, N_CLS = 3;

// ------------------------------------------------------------- weight registry

// A state_dict entry: true shape [rows, cols] (cols = 1: a vector) and the shape of its device copy, where every dimension
// that is the hidden width Dt is zero-padded to D (the multiple of 32 the kernels are built for).  GCNTrimapNet and
// GATTrimapNet run at Dt == D: their device copies are the arrays as loaded.  layout asks for a second device copy:
// 'T' = "#<key>T", the [cp][rp] transpose; 'P' = "#<key>.p", the D x D matrix packed for k_gemm (pack_mfma).
struct Need { std::string key; int64_t numel; int r = 0, c = 1, rp = 0, cp = 1; char layout = 0; };

static const char* const BN_KEYS[4] = {"weight", "bias", "running_mean", "running_var"};   // BatchNorm1d

// One network's weights: its spec, and the layouts it derives from the padded arrays beyond 'T' and 'P' (may be null).
struct NetSpec {
    const char* name;                      // "ResGCNNet": error messages
    const char* entry;                     // "resgcn": the ggc_<entry>_* entries
    WeightSet ggc_ctx::*weights;           // where the context keeps them
    bool batched;                          // the forward takes the batch structure (G graphs, node_ptr)
    std::vector<Need> (*needed)(const WeightSet& m);
    int (*derive)(ggc_ctx* ctx, WeightSet& m, std::map<std::string, std::vector<float>>& padded);
};

inline const float* devp(const WeightSet& m, const std::string& k) {
    auto it = m.dev.find(k);
    return it == m.dev.end() ? nullptr : reinterpret_cast<const float*>(it->second.p);
}

inline int upload(ggc_ctx* ctx, WeightSet& m, const std::string& key, const std::vector<float>& v) {
    Buf& b = m.dev[key];
    const size_t bytes = v.size() * sizeof(float);
    if (b.bytes < bytes) {
        if (b.p) GGC_HIP(ctx, hipFree(b.p));
        b.p = nullptr; b.bytes = 0;
        GGC_HIP(ctx, hipMalloc(&b.p, bytes ? bytes : 16));
        b.bytes = bytes;
    }
    if (bytes) GGC_HIP(ctx, hipMemcpy(b.p, v.data(), bytes, hipMemcpyHostToDevice));
    return GGC_OK;
}

inline std::vector<float> transpose(const std::vector<float>& w, int out, int in) {
    std::vector<float> t((size_t)out * in);
    for (int o = 0; o < out; ++o)
        for (int k = 0; k < in; ++k) t[(size_t)k * out + o] = w[(size_t)o * in + k];
    return t;
}

// Wp[s/4][t][lane][s%4] = W[32 t + (lane & 31)][(lane >> 5) * D/2 + s]
inline std::vector<float> pack_mfma(const std::vector<float>& w, int D) {
    const int T = D / 32, KH = D / 2;
    std::vector<float> p((size_t)D * D);
    for (int s = 0; s < KH; ++s)
        for (int t = 0; t < T; ++t)
            for (int l = 0; l < 64; ++l)
                p[(((size_t)(s / 4) * T + t) * 64 + l) * 4 + (s % 4)] =
                    w[(size_t)(32 * t + (l & 31)) * D + (l >> 5) * KH + s];
    return p;
}

// zero-padded copy [rp, cp] of a row-major [r, c] array
inline std::vector<float> pad2(const std::vector<float>& w, const Need& nd) {
    if (nd.r == nd.rp && nd.c == nd.cp) return w;
    std::vector<float> p((size_t)nd.rp * nd.cp, 0.0f);
    for (int i = 0; i < nd.r; ++i)
        for (int j = 0; j < nd.c; ++j) p[(size_t)i * nd.cp + j] = w[(size_t)i * nd.c + j];
    return p;
}

// The end of every ggc_<entry>_configure, after its width checks: a new shape drops the loaded weights.
inline int configure(ggc_ctx* ctx, const NetSpec& s, int D, int Dt, int n_layers) {
    GGC_REQUIRE(ctx, n_layers >= 1 && n_layers <= 30, GGC_E_INVALID_ARG, "n_layers=%d out of range [1,30]", n_layers);
    WeightSet& m = ctx->*s.weights;
    if (m.Dt != Dt || m.n_layers != n_layers) m.host.clear();
    m.D = D; m.Dt = Dt; m.n_layers = n_layers; m.dev_ok = false;
    return GGC_OK;
}

// ggc_<entry>_load_weight: num_batches_tracked is accepted and ignored; any other key must be in the spec, at its size.
inline int load_weight(ggc_ctx* ctx, const NetSpec& s, const char* name, const float* data, int64_t numel) {
    if (!ctx) return GGC_E_INVALID_ARG;
    WeightSet& m = ctx->*s.weights;
    GGC_REQUIRE(ctx, name && (data || numel == 0) && numel >= 0, GGC_E_INVALID_ARG, "bad weight arguments");
    GGC_REQUIRE(ctx, m.D > 0, GGC_E_STATE, "ggc_%s_configure has not been called", s.entry);
    const std::string key(name), tail = "num_batches_tracked";
    if (key.size() >= tail.size() && key.compare(key.size() - tail.size(), tail.size(), tail) == 0) return GGC_OK;
    bool known = false;
    for (const Need& nd : s.needed(m))
        if (nd.key == key) {
            GGC_REQUIRE(ctx, nd.numel == numel, GGC_E_SHAPE, "weight '%s' has %lld elements, expected %lld", name,
                        (long long)numel, (long long)nd.numel);
            known = true;
            break;
        }
    GGC_REQUIRE(ctx, known, GGC_E_INVALID_ARG, "unexpected state_dict key '%s' for %s(D=%d, n=%d)", name, s.name, m.Dt,
                m.n_layers);
    m.host[key].assign(data, data + numel);
    m.dev_ok = false;
    return GGC_OK;
}

// ggc_<entry>_ready: configured, and every key of the spec loaded at its size.
inline int check_ready(ggc_ctx* ctx, const NetSpec& s) {
    if (!ctx) return GGC_E_INVALID_ARG;
    const WeightSet& m = ctx->*s.weights;
    GGC_REQUIRE(ctx, m.D > 0, GGC_E_STATE, "ggc_%s_configure has not been called", s.entry);
    for (const Need& nd : s.needed(m)) {
        auto it = m.host.find(nd.key);
        GGC_REQUIRE(ctx, it != m.host.end(), GGC_E_STATE, "missing weight '%s'", nd.key.c_str());
        GGC_REQUIRE(ctx, (int64_t)it->second.size() == nd.numel, GGC_E_SHAPE, "weight '%s' has %zu elements, expected %lld",
                    nd.key.c_str(), it->second.size(), (long long)nd.numel);
    }
    return GGC_OK;
}

// Device copies of the weights, built once after every change: the zero-padded arrays under their state_dict keys (a width
// that is a multiple of 32 pads nothing; m.host keeps what was loaded), then the layouts derived from them.
inline int prepare_weights(ggc_ctx* ctx, const NetSpec& s) {
    WeightSet& m = ctx->*s.weights;
    if (m.dev_ok) return GGC_OK;
    int rc = check_ready(ctx, s);
    if (rc) return rc;
    // The device copies are about to be overwritten in place by blocking copies on the null stream, which does not wait for
    // the (non-blocking) stream a previous forward may still be running on: drain the device first.  Weight changes are rare.
    GGC_HIP(ctx, hipDeviceSynchronize());
    const std::vector<Need> spec = s.needed(m);
    std::map<std::string, std::vector<float>> pw;
    for (const Need& nd : spec) pw[nd.key] = pad2(m.host.at(nd.key), nd);
    for (auto& kv : pw) { if ((rc = upload(ctx, m, kv.first, kv.second))) return rc; }
    for (const Need& nd : spec) {
        if (nd.layout == 'T') rc = upload(ctx, m, "#" + nd.key + "T", transpose(pw[nd.key], nd.rp, nd.cp));
        if (nd.layout == 'P') rc = upload(ctx, m, "#" + nd.key + ".p", pack_mfma(pw[nd.key], nd.rp));
        if (rc) return rc;
    }
    if (s.derive && (rc = s.derive(ctx, m, pw))) return rc;
    m.dev_ok = true;
    return GGC_OK;
}

// Argument checks of a ggc_<entry>_forward and the weight upload before it.  G and node_ptr are checked when the network
// takes the batch structure; GCNTrimapNet does not.
inline int begin_forward(ggc_ctx* ctx, const NetSpec& s, int G, int N, int E, const float* x,
                         const int32_t* edge_src, const int32_t* edge_dst, const float* edge_attr, const int32_t* node_ptr,
                         const float* logits, const float* probs) {
    if (!ctx) return GGC_E_INVALID_ARG;
    if (s.batched)
        GGC_REQUIRE(ctx, G >= 1 && N >= 1 && E >= 0, GGC_E_SHAPE, "bad sizes G=%d N=%d E=%d", G, N, E);
    else
        GGC_REQUIRE(ctx, N >= 1 && E >= 0, GGC_E_SHAPE, "bad sizes N=%d E=%d", N, E);
    GGC_REQUIRE(ctx, x && (node_ptr || !s.batched) && (E == 0 || (edge_src && edge_dst && edge_attr)), GGC_E_INVALID_ARG,
                "null input pointer");
    GGC_REQUIRE(ctx, logits || probs, GGC_E_INVALID_ARG, "both outputs are NULL");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    return prepare_weights(ctx, s);
}

// ------------------------------------------------- launchers shared across files

// out[N,D] = op(A)[N,D] @ W^T on f32 MFMA (k_gemm, ggc_gnn_dense.hip)
//   MODE 0: A = LayerNorm(A1); store                                   (GCN XW)
//   MODE 1: A1 @ W1^T + A2 @ W2^T + bias -> LayerNorm -> GELU          (SAGE)
//   MODE 2: A = LayerNorm(A1 * gvec[batch]); + bias -> GELU -> head -> softmax
//   MODE 3: A1 @ W1^T, no prologue (GCNTrimapNet, GATTrimapNet)
//   MODE 4: as MODE 2 without the LayerNorm (GATTrimapNet head)
struct GemmArgs {
    const float *A1, *A2, *Wp1, *Wp2;
    const float *ln_w, *ln_b;        // prologue LayerNorm
    const float *bias;               // [D]
    const int32_t* batch;            // MODE 2
    const float* gvec;               // MODE 2: [G,D]
    const float *ep_w, *ep_b;        // MODE 1: LN weight/bias; MODE 2: head weight [3,D] / bias [3]
    float *out, *out2;               // MODE 2: logits / probs (either may be null)
    int accumulate = 0;              // MODE 3: out += A W^T instead of out = A W^T
    int Dt = 0;                      // true width for the LayerNorm statistics (0: D), see k_input
};
template <int D, int MODE>
int launch_gemm(ggc_ctx* ctx, hipStream_t st, int N, const GemmArgs& a);

// The forward pass hands over the batch structure (G graphs, node_ptr) and the packed column words built by
// build_agg_pack for the slice width agg_graph_slice chose; without them (ggc_gcn_aggregate) the direct gather runs.
struct AggGraphs { int G = 0, sw = 0; const int32_t* node_ptr = nullptr; const int32_t* pack = nullptr; };
int build_agg_pack(ggc_ctx* ctx, hipStream_t st, int N, int G, const int32_t* node_ptr, const int32_t* batch,
                   const int32_t* row_ptr, const int32_t* col, AggGraphs& ag);
// GCNConv (MODE 0) / SAGE-mean (MODE 1) gather over the destination CSR (ggc_gnn_gather.hip)
template <int D, int MODE>
int launch_aggregate(ggc_ctx* ctx, hipStream_t st, int N, const float* xw, const int32_t* row_ptr, const int32_t* col,
                     const float* dis, const float* bias, const float* gate, const float* h, float* out,
                     const AggGraphs& ag = AggGraphs{});
// Lane layout of a D-wide row in the direct gather (k_aggregate) and in k_jk: LPR lanes x float4 cover the row, a wave
// handles RPW rows, a block of 4 waves RPB.
template <int D> struct AggCfg {
    static constexpr int LPR = (D <= 32) ? 8 : (D <= 64) ? 16 : (D <= 128) ? 32 : 64;    // D > 128: a wave per row
    static constexpr int RPW = 64 / LPR;
    static constexpr int RPB = 4 * RPW;
};

// per-graph softmax readout and compress/expand MLP (k_graph_ctx, ggc_gnn_dense.hip)
struct CtxW { const float *wcT /*[D][D/2]*/, *bc, *weT /*[D/2][D]*/, *be; };
template <int D>
int launch_graph_ctx(ggc_ctx* ctx, hipStream_t st, int G, const int32_t* node_ptr, const float* score, const float* hjk,
                     const CtxW& w, float* gvec);

// Graph structure of one forward, in the context's scratch (ggc_csr.hip): the destination CSR of the edge list and dis
// (build_csr); with node_ptr, the graph of every node (batch); with_dst, the destination of every CSR position (dst).
struct Csr { int32_t *row_ptr, *col, *eid, *batch, *dst; float* dis; };
int prepare_csr(ggc_ctx* ctx, hipStream_t st, int G, int N, int E, const int32_t* edge_src, const int32_t* edge_dst,
                const int32_t* node_ptr, bool with_dst, Csr& g);

// BatchNorm1d(eval) parameters, (x - mean) / sqrt(var + 1e-5) * w + b
struct BnW { const float *w, *b, *rm, *rv; };
__device__ __forceinline__ float bn_apply(float x, const BnW& p, int k) {
    return (x - p.rm[k]) / sqrtf(p.rv[k] + 1e-5f) * p.w[k] + p.b[k];
}
inline BnW bn_of(const WeightSet& m, const std::string& prefix) {
    return BnW{devp(m, prefix + "weight"), devp(m, prefix + "bias"), devp(m, prefix + "running_mean"), devp(m, prefix + "running_var")};
}

// fused edge MLP + scatter-mean + block epilogue (k_gn_edge_gate, ggc_gcnnet.hip); MUL_ONLY = true for GATTrimapNet
template <int D, bool MUL_ONLY>
int launch_edge_gate(ggc_ctx* ctx, hipStream_t st, int N, const int32_t* row_ptr, const int32_t* eid, const int32_t* csr_dst,
                     const float* edge_attr, const float* w1T, const float* b1, const float* w2p, const float* b2,
                     const float* conv, const BnW& bn, const float* h, float* out);

} // namespace ggc
