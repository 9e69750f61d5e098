/*
 * ggc.h — C ABI of libggc_hip.so, the MI355X (gfx950) implementation of the
 * GCN-GrabCut per-image segmentation hot path
 *     SLIC -> superpixel graph -> residual GCN -> guided-filter trimap -> GrabCut
 *
 * The reference (HanielUlises/GCN-GrabCut) has no FFI of its own: its boundary
 * is the Python API of src/gcn_grabcut.  Every entry point below states which
 * reference symbol (file:line under the reference tree) it replaces; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and shipped
 * in gcn-grabcut_amd/gcn_grabcut/_native.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - Pointers marked [dev] are device pointers on the context's GPU; the
 *     caller owns them.  [host] pointers are ordinary host memory.
 *   - Every call is batched over B images of identical H x W and is
 *     asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream) unless the comment says it synchronises.
 *   - Return value: GGC_OK or a negative GGC_E_* code; ggc_last_error() gives
 *     the message.  No C++ exception crosses the boundary.
 *   - A context is bound to one device and must be used by one host thread at
 *     a time.  Scratch memory grows monotonically inside the context and is
 *     released by ggc_ctx_destroy().
 *
 * Environment switches (all optional; the library reads them ONCE per process,
 * through one function, ggc::knobs() in csrc/ggc_context.hip; none changes a
 * result — tests/test_maxflow_variants_gpu.py holds the max-flow ones to that):
 *   GGC_MF_TRACE=1                per-round max-flow diagnostics on stderr (blocking)
 *   GGC_MF_WARM=0                 cold max-flow start in every GrabCut iteration (default 1: keep the n-link flow)
 *   GGC_MF_ASYNC_PUSH_ACTIVE=n    push rounds with <= n active pixels run asynchronously (10000)
 *   GGC_MF_ASYNC_TILE=8|16|32     rows of the asynchronous push tile (8)
 *   GGC_MF_ASYNC_HOPS=n           longest chain of tile visits in an asynchronous push launch (24)
 *   GGC_MF_ASYNC_SWEEPS=n         sweeps per asynchronous push visit (12)
 *   GGC_MF_DENSE_LAUNCHES0=n / GGC_MF_DENSE_LAUNCHES=n   push launches of the first / a later dense round (8 / 12)
 *   GGC_MF_DENSE_SWEEPS=n         sweeps per dense push visit, one step each for up to 64 of the tile's active pixels (12)
 *   GGC_MF_RELAX_DENSE=n          work-list launches of a global relabel before the asynchronous launch takes over (3)
 *   GGC_MF_PARTIAL_ROUNDS=n       first rounds of a solve whose relabel stops after those launches (3; 0 = every relabel exact;
 *                                 0..64, larger values are clamped to 64: a partial round never closes an image)
 *   GGC_MF_LABEL_SLACK=n          label ceiling of the push phases: a pixel whose label reaches (the image's largest finite label
 *                                 after the round's relabel) + 1 + n keeps its excess until the next global relabel, as a pixel
 *                                 at label H * W does; negative = no ceiling (0)
 *   GGC_AGG_DIRECT=1              GCNConv gather straight from L2 instead of the graph-resident kernel
 *   GGC_SLIC_SEQ_CONNECTIVITY=1   literal one-thread-per-image replay of skimage's connectivity pass (A/B reference)
 *   GGC_SLIC_CN_TILES=0           SLIC connectivity by the rounds on a pending plane throughout (default 1: the first round labels
 *                                 64 x 16 tiles in LDS and replays the components below min_size from an on-chip queue of 256
 *                                 pixels).  Profiler scopes inside "slic_connectivity" tell what ran: "slic_cn_tiles" the tile
 *                                 round, "slic_cn_replay" the on-chip replay, "slic_cn_spill" the replay of small components
 *                                 above 256 pixels through global memory, "slic_cn_rounds" the rounds on the pending plane
 *                                 (the knob at 0, or a component of max_size pixels or more)
 *   GGC_GRAPH_ONCHIP=0|1|2       region-graph topology of ggc_graph_count from on-chip pair tables instead of the dense
 *                                 B x N x N matrix: 0 never, 1 (default) for batches of at least 24 images, 2 at any batch size;
 *                                 in each case only where an image has at most 704 regions, 6144 distinct adjacent pairs and
 *                                 n_nonlocal <= 8, else the dense kernels run (same outputs, byte for byte)
 *   GGC_GRAPH_BANDS=n             row bands (workgroups) per image of that on-chip scan, 1..8, clamped to the image's rows
 *                                 (default 0: min(8, CUs / batch, rows)); the profiler scope "graph_scan" counts its launches
 *                                 and "graph_dense" those of the dense matrix, so the two tell which path a call took
 *   GGC_MATTE_EVAL_LEVELS=1|2|5|10  threshold levels that ggc_matte_errors labels per pass (default: 10 while its maps fit 4 GiB, else 1)
 *   GGC_WAND_SEEDS_PER_PASS=n     seeds that ggc_wand_select labels per pass, 1..4096 (default: as many as keep its maps within 1 GiB)
 * The Python binding adds GGC_HIP_LIBRARY=<path> (load another build of the library, tools/build_variant.sh).
 */
#ifndef GGC_H
#define GGC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGC_VERSION 411 /* 0.4.11: ggc_composite_over, ggc_poisson_clone (a cut-out placed on a new background: integer alpha-over at an offset,
                                  and gradient-domain "seamless" cloning after Perez, Gangnet and Blake, PCG on the device; additive,
                                  no existing entry changes);
                           0.4.10: ggc_wand_select (magic wand: flood select by colour tolerance from seed pixels, contiguous or not, as
                                  GrabCut labels, a selection plane and counts; additive, no existing entry changes);
                           0.4.9: ggc_mask_distance, ggc_modify_mask (the exact squared Euclidean distance transform of a mask, signed, and
                                  grow / shrink / border / open / close / trimap as thresholds of it; additive, no existing entry changes);
                           0.4.8: ggc_mask_outlines (the exact vector contours of a mask: crack-following loops on the corner lattice, as
                                  vertices in ggc_apply_polygons' packing, with area, perimeter and outer loop; additive, no existing
                                  entry changes);
                           0.4.7: ggc_trace_paths (intelligent scissors: a few boundary anchors joined by the cheapest path along image
                                  edges, as vertices in ggc_apply_polygons' packing; additive, no existing entry changes);
                           0.4.6: ggc_apply_polygons (lassos and filled polygons as hard constraints: one exact integer point-in-polygon
                                  rule, even-odd with a closed boundary; additive, no existing entry changes);
                           0.4.5: ggc_apply_strokes, ggc_stroke_pixels (brush strokes as hard constraints: polylines painted as capsules by
                                  one exact integer rule, and their centre lines as a click list; additive, no existing entry changes);
                           0.4.4: ggc_geodesic_hints (clicks propagated by a capped, colour-aware shortest-path distance instead of a fixed
                                  disk; additive, ggc_apply_hints does not change);
                           0.4.3: ggc_lift_labels (a working-size mask carried to a larger size as GrabCut labels with an open band
                                  around its edge: the start of a banded graph cut on the full image; no existing entry changes);
                           0.4.2: ggc_lift_trimap, ggc_trimap_matte_warm, ggc_closed_form_band (a working-size closed-form matte carried to a
                                  larger image: lifted trimap and start, a stop rule that does not move with the start; the two
                                  existing closed-form entries do not change);
                           0.4.1: ggc_trimap_matte (closed-form alpha matte on the unknown region of a caller's trimap; one solver with
                                  ggc_closed_form_matte, whose results do not change);
                           0.4.0: ggc_matte_errors (SAD, MSE, gradient and connectivity error of an alpha matte against the true one);
                           0.3.9: ggc_estimate_foreground (foreground colours under an alpha matte: clean cut-outs, PCG on the device);
                           0.3.8: ggc_closed_form_matte (closed-form alpha matte: matting Laplacian solved by PCG on the device);
                           0.3.7: ggc_upsample_matte (the matte's mask and alpha at a larger resolution: fast guided filter);
                           0.3.6: ggc_alpha_matte (soft alpha matte of a binary mask: colour guided-filter feathering);
                           0.3.5: ggc_grid_maxflow (the GrabCut max-flow on a caller's network, a test hook);
                           0.3.4: ggc_next_click (the next simulated click of the NoC protocol);
                           0.3.3: ggc_apply_hints (user clicks as hard constraints on the GrabCut mask);
                           0.3.2: ResGCNNet (forward and ggc_train_*), GATTrimapNet and ggc_gcn_aggregate at widths up to 256;
                           0.3.1: ggc_train_* (graph operators of the ResGCNNet training forward and their backward) */

enum {
    GGC_OK            =  0,
    GGC_E_INVALID_ARG = -1,
    GGC_E_SHAPE       = -2,
    GGC_E_OOM         = -3,
    GGC_E_DEVICE      = -4,
    GGC_E_UNSUPPORTED = -5,
    GGC_E_STATE       = -6
};

/* GrabCut label space == cv2.GC_* == reference grabcut.py:22-27 (Label). */
enum { GGC_BGD = 0, GGC_FGD = 1, GGC_PR_BGD = 2, GGC_PR_FGD = 3 };

/* Feature widths: reference graph_builder.py:73-77. */
#define GGC_N_IMAGE_FEATS 16
#define GGC_N_PRIOR_FEATS 3
#define GGC_N_NODE_FEATS  19
#define GGC_N_EDGE_FEATS  5

typedef struct ggc_ctx ggc_ctx;
typedef void*          ggc_stream; /* hipStream_t */

/* ------------------------------------------------------------------ context */

int         ggc_version(void);
int         ggc_ctx_create(int device_id, ggc_ctx** out);
int         ggc_ctx_destroy(ggc_ctx* ctx);
const char* ggc_last_error(const ggc_ctx* ctx); /* ctx may be NULL: last create error */

/* Per-kernel timing for the roofline report (bench.py): while enabled, the
 * dominant kernels are bracketed by HIP events on their launch stream.
 * ggc_profile_enable(ctx, 1) clears earlier records and SYNCHRONISES the device;
 * ggc_profile_query sums the recorded durations of one kernel by name
 * ("gcn_aggregate", "gcn_gemm", "slic_assign", "maxflow", ...) and waits for them.
 * An event pair around nothing does not read zero (two queue packets), so enable
 * calibrates that offset with empty pairs and query subtracts it per scope; the
 * name "#event_pair_overhead" returns the offset itself (launches = 1).
 * on = 1: every instrumented scope; on = 2: only "gcn_aggregate", the kernel the
 * roofline grades (an event pair costs its stream ~10 us of idle time per scope, and a
 * step has several hundred scopes); on = 0: off. */
int ggc_profile_enable(ggc_ctx* ctx, int on);
int ggc_profile_query(ggc_ctx* ctx, const char* kernel, int* launches, double* total_ms);

/* Diagnostic hook for the parity tests: copy the first `bytes` of a named
 * scratch buffer ("slic_raw_labels", "slic_centers", "slic_image_a", ...) to
 * host memory.  SYNCHRONISES the device. */
int ggc_debug_read_scratch(ggc_ctx* ctx, const char* name, void* host_dst, size_t bytes);

/* --------------------------------------------------------------- G0 colour prep
 * Replaces GraphBuilder.__init__ (graph_builder.py:142-154): BGR->Lab (f64
 * arithmetic, stored f32), BGR->HSV (f64 -> f32), BGR->GRAY (8-bit fixed
 * point, stored f32), Sobel 3x3 gradient magnitude.
 *   bgr  [dev] u8  [B,H,W,3]
 *   lab  [dev] f32 [B,H,W,3]     hsv [dev] f32 [B,H,W,3]
 *   gray [dev] f32 [B,H,W]       grad [dev] f32 [B,H,W]
 */
int ggc_preprocess(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                   const uint8_t* bgr, float* lab, float* hsv, float* gray, float* grad);

/* --------------------------------------------------------------------- G1 SLIC
 * Replaces GraphBuilder._compute_superpixels (graph_builder.py:177-188), i.e.
 * skimage.segmentation.slic(lab_f32, n_segments, compactness, sigma,
 * start_label=0, channel_axis=-1): global min-max rescale (if rescale_input),
 * second rgb2lab in f32, Gaussian pre-smoothing, 10 k-means sweeps,
 * connectivity enforcement.  Labels are contiguous 0..n_nodes[b]-1.
 *   image    [dev] f32 [B,H,W,3]   (the Lab image from ggc_preprocess)
 *   segments [dev] i32 [B,H,W]
 *   n_nodes  [dev] i32 [B]
 */
int ggc_slic(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
             const float* image, int n_segments, float compactness, float sigma,
             int rescale_input, int32_t* segments, int32_t* n_nodes);

/* The same for SuperpixelGraphConfig(use_lab=False) (graph_builder.py:177-179): skimage.segmentation.slic on
 * `rgb.astype(float)`, i.e. the float64 instance of every stage (min-max rescale, rgb2lab, Gaussian, k-means).
 *   bgr      [dev] u8 [B,H,W,3]    (the image itself: the reference converts BGR -> RGB -> float64)
 */
int ggc_slic_rgb(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                 const uint8_t* bgr, int n_segments, double compactness, double sigma,
                 int32_t* segments, int32_t* n_nodes);

/* Step 7 of ggc_slic alone — skimage's _enforce_label_connectivity_cython
 * (SURVEY Appendix A.1): raw_labels, segments [dev] i32 [B,H,W]; n_nodes [dev] i32 [B].
 * SYNCHRONISES the stream once, and once more per carve round (components of >= max_size pixels). */
int ggc_slic_enforce_connectivity(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                                  const int32_t* raw_labels, int min_size, int max_size,
                                  int32_t* segments, int32_t* n_nodes);

/* ------------------------------------------------------------ G2-G8 graph build
 * Replaces GraphBuilder.build's tail (graph_builder.py:160-175):
 * _region_statistics, _assemble_node_features, _compute_edges (+_pair_features,
 * _nonlocal_pairs) and compute_auto_prior (graph_builder.py:357-444).
 *
 * Two-phase because N and E are data dependent.  ggc_graph_count runs the
 * whole construction into context scratch and returns the per-image offsets;
 * it SYNCHRONISES the stream once to read them back.  ggc_graph_fill copies
 * the result into caller buffers sized from those offsets.
 *   node_ptr [host] i64 [B+1]   prefix sums of n_nodes
 *   edge_ptr [host] i64 [B+1]   prefix sums of directed edge counts
 */
int ggc_graph_count(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                    const int32_t* segments, const int32_t* n_nodes,
                    const float* lab, const float* hsv, const float* grad,
                    int connectivity, int n_nonlocal,
                    int64_t* node_ptr, int64_t* edge_ptr);

/*   x          [dev] f32 [N_total,19]   node_input(): 16 image feats || 3 prior
 *   centroids  [dev] f32 [N_total,2]    (cy, cx) normalised
 *   area_ratio [dev] f32 [N_total]
 *   edge_src, edge_dst [dev] i32 [E_total]  LOCAL node ids (per image), in the
 *              reference's order: [adjacency pairs sorted, non-local pairs
 *              sorted] then the mirrored copy (graph_builder.py:303-306)
 *   edge_attr  [dev] f32 [E_total,5]
 * Any output pointer may be NULL to skip it.  global_ids != 0 adds each image's
 * node offset to the edge endpoints (PyG Batch collation), which is the form
 * ggc_resgcn_forward consumes.
 */
int ggc_graph_fill(ggc_ctx* ctx, ggc_stream stream,
                   float* x, float* centroids, float* area_ratio,
                   int32_t* edge_src, int32_t* edge_dst, float* edge_attr, int global_ids);

/* compute_auto_prior(segments, lab, centre_sigma=0.45, contrast_sigma=0.40) (graph_builder.py:357-362): the two sigmas of
 * the prior used by the NEXT ggc_graph_count calls of this context (defaults = the reference's). */
int ggc_graph_prior_sigmas(ggc_ctx* ctx, double centre_sigma, double contrast_sigma);

/* ------------------------------------------------------------ M0-M7 ResGCNNet
 * Replaces ResGCNNet (model.py:421-557), eval mode.
 * ggc_resgcn_configure fixes the architecture; ggc_resgcn_load_weight takes
 * one state_dict entry by its reference key, e.g.
 * "gcn_layers.3.lin.weight", as a contiguous f32 HOST array.  Integer buffers
 * ("...num_batches_tracked") are accepted and ignored.
 * hidden: any width from 8 to 256 (model.py:449-455 takes any; GGC_E_UNSUPPORTED above 256); the entries are given in their
 * TRUE shapes.  A width that is not a multiple of 32 runs zero-padded to the next one inside the library (LayerNorm
 * statistics on the true width).
 */
int ggc_resgcn_configure(ggc_ctx* ctx, int hidden, int n_layers);
int ggc_resgcn_load_weight(ggc_ctx* ctx, const char* name, const float* data /*[host]*/,
                           int64_t numel);
/* 0 when every tensor the forward pass needs has been loaded. */
int ggc_resgcn_ready(ggc_ctx* ctx);

/* Batched forward over G graphs (PyG Batch semantics, model.py:508-536):
 *   x         [dev] f32 [N,19]       edge_attr [dev] f32 [E,5]
 *   edge_src, edge_dst [dev] i32 [E] GLOBAL node ids (already offset per graph)
 *   node_ptr  [dev] i32 [G+1]        graph g owns nodes node_ptr[g]..node_ptr[g+1]
 *   logits    [dev] f32 [N,3]        (may be NULL)
 *   probs     [dev] f32 [N,3]        softmax(logits) (model.py:543-546; may be NULL)
 */
int ggc_resgcn_forward(ggc_ctx* ctx, ggc_stream stream, int G, int N, int E,
                       const float* x, const int32_t* edge_src, const int32_t* edge_dst,
                       const float* edge_attr, const int32_t* node_ptr,
                       float* logits, float* probs);

/* GCNTrimapNet, the reference's baseline model (`--model gcn`, model.py:239-316), eval mode.
 * Same protocol as the ResGCNNet entries: configure, load every float tensor of the state_dict by its key
 * ("in_norm.norm.weight", "blocks.0.conv.lin.weight", "blocks.0.edge_inject.proj.2.bias", "head.6.weight", ...;
 * *.num_batches_tracked is ignored), then forward.  The reference's forward takes no batch vector (the model has no
 * per-graph readout), so a batch is simply the concatenated graphs.
 *   x [dev] f32 [N,19]  edge_src, edge_dst [dev] i32 [E]  edge_attr [dev] f32 [E,5]
 *   logits, probs [dev] f32 [N,3] (either may be NULL) */
int ggc_gcnnet_configure(ggc_ctx* ctx, int hidden_channels, int n_layers);
int ggc_gcnnet_load_weight(ggc_ctx* ctx, const char* name, const float* data /*[host]*/, int64_t numel);
int ggc_gcnnet_ready(ggc_ctx* ctx);
int ggc_gcnnet_forward(ggc_ctx* ctx, ggc_stream stream, int N, int E,
                       const float* x, const int32_t* edge_src, const int32_t* edge_dst,
                       const float* edge_attr, float* logits, float* probs);

/* GATTrimapNet, the reference's attention variant (`--model gat`, model.py:323-414; SURVEY 8(f) last rank), eval mode: GATv2
 * attention with edge features (n_heads heads), LayerNorm + GELU, per-block edge gates, skip, per-graph attention readout, head.
 * Same protocol: configure, load every float tensor of the state_dict by its key ("convs.0.att", "convs.0.lin_l.weight",
 * "convs.0.lin_edge.weight", "lns.0.weight", "edge_gates.0.proj.2.bias", "skip_proj.weight", "ctx.attn.weight",
 * "head.3.weight", ...), then forward.  hidden_channels in {32, 64, 128, 256} with n_heads in {1, 2, 4, 8} (GGC_E_UNSUPPORTED
 * otherwise).  Arguments as ggc_resgcn_forward
 * (node_ptr delimits the graphs of the batch for the readout). */
int ggc_gat_configure(ggc_ctx* ctx, int hidden_channels, int n_heads, int n_layers);
int ggc_gat_load_weight(ggc_ctx* ctx, const char* name, const float* data /*[host]*/, int64_t numel);
int ggc_gat_ready(ggc_ctx* ctx);
int ggc_gat_forward(ggc_ctx* ctx, ggc_stream stream, int G, int N, int E,
                    const float* x, const int32_t* edge_src, const int32_t* edge_dst,
                    const float* edge_attr, const int32_t* node_ptr,
                    float* logits, float* probs);

/* M3 alone — the GCNConv scatter-gather the north star grades (PyG GCNConv
 * inside model.py:523-528).  CSR over destinations, self loops implicit.
 *   out_i = sum_{e: dst(e)=i} dis[src]*dis[i]*xw[src] + dis[i]*dis[i]*xw[i] + bias
 *   if gate != NULL:  h_out_i = h_i + gelu(out_i * gate_i)   (fused epilogue)
 *   else:             h_out_i = out_i
 *   xw [dev] f32 [N,D]  row_ptr [dev] i32 [N+1]  col [dev] i32 [E]
 *   dis [dev] f32 [N] = (1+indeg)^-1/2   bias [dev] f32 [D]
 * D: a multiple of 32 from 32 to 256 (GGC_E_UNSUPPORTED otherwise).
 */
int ggc_gcn_aggregate(ggc_ctx* ctx, ggc_stream stream, int N, int D,
                      const float* xw, const int32_t* row_ptr, const int32_t* col,
                      const float* dis, const float* bias,
                      const float* gate, const float* h, float* h_out);

/* Helper used with ggc_gcn_aggregate: build the destination CSR the forward
 * pass uses (stable in edge order) and dis = (1+indeg)^-1/2.
 *   row_ptr [dev] i32 [N+1]   col [dev] i32 [E]   dis [dev] f32 [N]
 */
int ggc_build_csr(ggc_ctx* ctx, ggc_stream stream, int N, int E,
                  const int32_t* edge_src, const int32_t* edge_dst,
                  int32_t* row_ptr, int32_t* col, float* dis);

/* ------------------------------------------------------------ training (ResGCNNet)
 * The graph operators of the ResGCNNet training forward (model.py:508-536, train mode) and their backward passes, f32.
 * The dense layers stay in the host's autograd.  No entry uses a float atomic: every sum runs in one fixed order, so two
 * runs give identical bits.  A scatter in a backward pass is a gather over the SOURCE CSR.  Node widths D: a multiple of
 * 32 from 32 to 256 (GGC_E_UNSUPPORTED otherwise).  All arrays are device arrays.
 *
 * Graph preparation, once per batch, shared by every layer: destination CSR (row_ptr [N+1], col = source [E],
 * eid = edge id [E]) and source CSR (srow_ptr [N+1], scol = destination [E], seid [E]), both stable in edge order;
 * dis [N] = (1+indeg)^-1/2 and inv_cnt [N] = 1/max(indeg, 1).  col/eid/scol/seid may be NULL when E == 0. */
int ggc_train_prepare(ggc_ctx* ctx, ggc_stream stream, int N, int E, const int32_t* edge_src, const int32_t* edge_dst,
                      int32_t* row_ptr, int32_t* col, int32_t* eid, int32_t* srow_ptr, int32_t* scol, int32_t* seid,
                      float* dis, float* inv_cnt);

/* GCNConv with the ResGCNNet residual epilogue, semantics as ggc_gcn_aggregate:
 *   out_i = sum_{e: dst(e)=i} dis[src]*dis[i]*xw[src] + dis[i]^2 xw[i] + bias
 *   y_i   = h_i + gelu(out_i * gate_i)      (y_i = gelu(out_i * gate_i) when h == NULL: the caller adds dropout + residual)
 *   xw, gate, h, out, y [N,D]  bias [D]  row_ptr/col/dis from ggc_train_prepare */
int ggc_train_gcn_forward(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* xw, const int32_t* row_ptr,
                          const int32_t* col, const float* dis, const float* bias, const float* gate, const float* h,
                          float* out, float* y);
/* Its backward, given g_y = dL/dy and the forward's out:
 *   g_out  = g_y * gelu'(out*gate) * gate      g_gate = g_y * gelu'(out*gate) * out        (both [N,D])
 *   g_xw_j = sum_{e: src(e)=j} dis[j]*dis[dst]*g_out[dst] + dis[j]^2 g_out[j]             (source CSR)
 * dL/dbias = column sums of g_out; dL/dh = g_y (the residual). */
int ggc_train_gcn_backward(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* g_y, const float* out,
                           const float* gate, const int32_t* srow_ptr, const int32_t* scol, const float* dis,
                           float* g_out, float* g_gate, float* g_xw);

/* SAGEConv mean: m_i = inv_cnt_i * sum_{e: dst(e)=i} x[src]   (x, m [N,D], destination CSR) */
int ggc_train_sage_mean(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* x, const int32_t* row_ptr,
                        const int32_t* col, const float* inv_cnt, float* out);
/* Its backward: g_x_j = sum_{e: src(e)=j} inv_cnt[dst] * g_m[dst]   (source CSR) */
int ggc_train_sage_mean_backward(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* g_m, const int32_t* srow_ptr,
                                 const int32_t* scol, const float* inv_cnt, float* g_x);

/* EdgeContext scatter-mean (model.py:128-139): ctx_i = inv_cnt_i * sum_{e: dst(e)=i} enc[e]
 *   enc [E,C]  ctx [N,C]  row_ptr/eid: destination CSR.  Any C >= 1. */
int ggc_train_edge_mean(ggc_ctx* ctx, ggc_stream stream, int N, int C, const float* enc, const int32_t* row_ptr,
                        const int32_t* eid, const float* inv_cnt, float* out);
/* Its backward, a gather: g_enc_e = inv_cnt[dst(e)] * g_ctx[dst(e)]   (edge_dst [E], g_ctx [N,C], g_enc [E,C]) */
int ggc_train_edge_mean_backward(ggc_ctx* ctx, ggc_stream stream, int E, int C, const int32_t* edge_dst,
                                 const float* inv_cnt, const float* g_ctx, float* g_enc);

/* GlobalContextModule readout (model.py:90-108, 176-188), one workgroup per graph; graphs are contiguous by node_ptr [G+1]:
 *   attn_i = exp(s_i - max_g s) / (sum_g exp(s - max_g s) + 1e-12)      (score, attn [N])
 *   hb_i   = sum_{j in graph(i)} attn_j h_j                              (h, hb [N,D]: pooled, broadcast to every node) */
int ggc_train_graph_pool(ggc_ctx* ctx, ggc_stream stream, int G, int N, int D, const int32_t* node_ptr, const float* h,
                         const float* score, float* attn, float* hb);
/* Its backward, given g_hb = dL/dhb: gp_g = sum_{i in g} g_hb_i, g_h_i = attn_i gp_g (the pooling term only),
 * ga_i = <gp_g, h_i>, g_score_i = attn_i (ga_i - sum_{j in g} attn_j ga_j). */
int ggc_train_graph_pool_backward(ggc_ctx* ctx, ggc_stream stream, int G, int N, int D, const int32_t* node_ptr,
                                  const float* h, const float* attn, const float* g_hb, float* g_h, float* g_score);

/* ------------------------------------------------------------ P0-P3 trimap
 * Replaces refine_trimap (pipeline.py:103-146) incl. guided_filter
 * (pipeline.py:71-100) and project_to_pixels (model.py:648-661) when
 * edge_aware != 0; replaces _probs_to_trimap (model.py:664-678) otherwise.
 *   probs    [dev] f32 [N_total,3]     node_ptr [dev] i32 [B+1]
 *   segments [dev] i32 [B,H,W]         bgr [dev] u8 [B,H,W,3]
 *   trimap   [dev] u8  [B,H,W]  values in {0,1,2,3}
 */
int ggc_refine_trimap(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                      const float* probs, const int32_t* node_ptr,
                      const int32_t* segments, const uint8_t* bgr,
                      float threshold_fg, float threshold_bg,
                      int radius, float eps, int edge_aware, uint8_t* trimap);

/* P1 alone — replaces guided_filter (pipeline.py:71-100) for callers that use it
 * directly.  guide, src, out [dev] f32 [B,H,W]. */
int ggc_guided_filter(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                      const float* guide, const float* src, int radius, float eps, float* out);

/* S0 — replaces _seed_from_prior (pipeline.py:149-186); in place on trimap.
 *   prior [dev] f32 [N_total,3] (columns 16..18 of x, contiguous copy) */
int ggc_seed_from_prior(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                        const float* prior, const int32_t* node_ptr,
                        const int32_t* segments, double seed_frac, uint8_t* trimap);

/* ------------------------------------------------------------ C0-C6 GrabCut
 * Replaces GrabCut.run_with_trimap / run_with_bbox / refine
 * (grabcut.py:81-163), i.e. cv2.grabCut: GMM init (seeded k-means++), n_iter x
 * {assign components, learn GMMs, build graph, max-flow, relabel}.
 *   mode: 0 = GC_INIT_WITH_MASK (mask holds the trimap, promotions and the
 *             degenerate guard of grabcut.py:127-140 applied here),
 *         1 = GC_INIT_WITH_RECT (rects [host] i32 [B,4] = x,y,w,h),
 *         2 = GC_EVAL (reuse models)
 *   image  [dev] u8  [B,H,W,3]  (already in the configured colour space)
 *   mask   [dev] u8  [B,H,W]    in/out GrabCut labels
 *   bgd_model, fgd_model [dev] f64 [B,65]  in/out (5 coefs | 15 means | 45 covs)
 *   binary [dev] u8  [B,H,W]    out: mask in {FGD, PR_FGD} (grabcut.py:165-168)
 */
int ggc_grabcut(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                const uint8_t* image, uint8_t* mask, const int32_t* rects,
                double* bgd_model, double* fgd_model, int n_iter, int mode,
                uint64_t seed, uint8_t* binary);

/* C5 — the max-flow of ggc_grabcut on a given network (additive; a test hook that runs the production solver).
 * Per image an 8-neighbour grid with int32 capacities, in k_build_graph's layout:
 *   tw  [dev] i32 [n_steps,B,H,W]  t-link difference, source minus sink (> 0: source link, < 0: sink link)
 *   nw  [dev] i32 [4,B,H,W]        undirected n-links of each pixel towards left, up-left, up, up-right; a link that points
 *                                  outside the image is ignored (never read, never checked)
 *   source_side [dev] u8 [n_steps,B,H,W]  out: 1 = the pixel cannot reach the sink in the final residual graph of that step
 *   residual    [dev] i32 [B,H,W,10] out, may be NULL: the final state of the last step — residual capacities of the 8 arcs
 *               (0 left, 1 right, 2 up, 3 down, 4 up-left, 5 down-right, 6 up-right, 7 down-left), excess, residual sink
 *               capacity (a maximum preflow: excess that cannot reach the sink stays where it is)
 * Step 0 solves cold; a later step changes only tw and starts from the previous step's flow as a GrabCut iteration does
 * (GGC_MF_WARM).  Bounds: |tw| <= 2^27 and 0 <= nw <= 2^24 for every in-image link (GrabCut's own t-links are at most
 * 117 964 800 < 2^27 and its n-links at most 13 107 200 < 2^24), which keeps the largest excess, about 3 * 2^27, inside
 * int32; a value outside them, B, H, W or n_steps < 1, or a NULL tw, nw or source_side is GGC_E_INVALID_ARG before any
 * solve.  SYNCHRONISES. */
int ggc_grid_maxflow(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, int n_steps,
                     const int32_t* tw, const int32_t* nw, uint8_t* source_side, int32_t* residual);

/* H0 — user clicks as hard constraints (additive; reference graph_builder.py:457-494, batched).
 *   hints    [dev] i32 [K,3] = (row, col, label) with label 0 = background, nonzero = foreground;
 *            grouped by image, click order kept within an image
 *   hint_ptr [dev] i32 [B+1]  image b owns hints[hint_ptr[b] .. hint_ptr[b+1]); hint_ptr[0] = 0, non-decreasing
 *   radius   disk radius in pixels: (dy*dy + dx*dx) <= radius*radius; 0 = the clicked pixel only
 *   region   0 = disks only; 1 = first the whole superpixel under a click, then the disks
 *   segments [dev] i32 [B,H,W] local labels, node_ptr [dev] i32 [B+1]  (both may be NULL when region == 0
 *            and node_hints == NULL)
 *   node_hints [dev] f32 [N_total,3] out, may be NULL: encode_user_hints of each image
 *   mask     [dev] u8 [B,H,W] in/out GrabCut labels (may be NULL when node_hints is not: only the table is written)
 * A click outside its image is ignored.  Disks: every pixel inside the disk of a click becomes GGC_FGD or GGC_BGD, clipped
 * to the image; where disks overlap, the last click of the image wins.  Regions (applied before the disks): a superpixel
 * whose in-bounds clicks are all foreground becomes GGC_FGD, all background GGC_BGD; one with both is left to the disks.
 * node_hints rows node_ptr[b].. get column 0 = foreground click, 1 = background click, 2 = neither.  Pixels no hint
 * touches keep their label.  No float atomics: the result does not depend on launch order.  K = hint_ptr[B] == 0 or B == 0
 * is a no-op (node_hints is not written).  A malformed hint_ptr / node_ptr or a negative radius is GGC_E_INVALID_ARG.
 * SYNCHRONISES the stream to read hint_ptr (and node_ptr when the superpixels are used). */
int ggc_apply_hints(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* hints, const int32_t* hint_ptr,
                    int radius, int region, const int32_t* segments, const int32_t* node_ptr,
                    float* node_hints, uint8_t* mask);

/* H1 — geodesic click hints (additive): a click labels the pixels that are close to it along paths that do not cross colour
 * edges, instead of ggc_apply_hints' fixed disk.  One exact integer definition; no float is involved anywhere.
 *   bgr      [dev] u8  [B,H,W,3] the images (the guide)
 *   hints, hint_ptr             ggc_apply_hints' packing: rows (row, col, label != 0 = foreground), image b owns
 *                               hints[hint_ptr[b] .. hint_ptr[b+1]); hint_ptr[0] = 0, non-decreasing
 *   radius   0 .. 16384: limit = 80 * radius          gamma   0 .. 64: weight of the colour term
 *   segments [dev] i32 [B,H,W] local labels, node_ptr [dev] i32 [B+1]  (both may be NULL unless node_dist is given)
 *   mask     [dev] u8  [B,H,W] in/out GrabCut labels, may be NULL
 *   dist_fg, dist_bg [dev] i32 [B,H,W] out, each may be NULL
 *   node_dist [dev] i32 [N_total,2] out, may be NULL           (at least one of the four outputs must be given)
 * Guide: S_c(y,x) = sum of the nine bytes I_c(clamp(y+dy, 0, H-1), clamp(x+dx, 0, W-1)), dy, dx in {-1,0,1}: a 3x3 box sum with
 * replicated border, 0 .. 2295 per channel.  Arcs: the grid is 8-connected, arcs only between pixels inside the image, and
 *   c(p,q) = L(p,q) + gamma * (|S_0(p)-S_0(q)| + |S_1(p)-S_1(q)| + |S_2(p)-S_2(q)|),   L = 80 axial, 113 diagonal (80 * sqrt 2),
 * symmetric.  Sources: a click outside its image is ignored; a pixel clicked more than once takes the label of the image's LAST
 * click on it, so an image's foreground and background sources are disjoint.  Df(p), Db(p) = cost of the cheapest path from p
 * to the nearest foreground / background source.  dist_fg / dist_bg receive min(D, limit + 1); an image or label without a
 * source reports limit + 1 everywhere.  Label rule: mask = GGC_FGD where Df <= limit and Df < Db, GGC_BGD where Db <= limit and
 * Db < Df; every other pixel, ties included, is neither read nor written.  A source has distance 0 and takes its own label.
 * node_dist[n] = (min Df, min Db) of the capped values over the pixels of superpixel n of its image (labels outside
 * [0, n_nodes) are skipped), written for every node of every image, by integer atomicMin.
 * Ranges: the largest arc is 113 + 64 * 6885 = 440 753 and no stored value exceeds limit + 1 <= 1 310 721, so every sum the
 * relaxation forms stays below 2^21 + 2^19: everything fits int32.  radius or gamma out of range, a malformed hint_ptr /
 * node_ptr, or no output at all is GGC_E_INVALID_ARG, before any launch; B <= 65535, H, W >= 1 else GGC_E_SHAPE.  B == 0 or
 * K = hint_ptr[B] == 0 is a no-op: nothing is written.  The shortest-path value is unique, so the outputs do not depend on
 * the schedule, and every image's outputs equal those of its single-image call bit for bit.  Work beyond two streaming
 * launches is O(clicks * radius^2): tiles farther than `radius` pixels from every click are never visited.  The relaxation
 * runs in rounds, one launch each; past min(radius, 1024 * tiles per image - 1) + 2 rounds it returns GGC_E_DEVICE
 * "geodesic hints did not converge" (it cannot hang).  Scratch: 6 bytes per pixel for the guide, 4 more for each of dist_fg /
 * dist_bg that is NULL, and 16 bytes per 32x32 tile.  SYNCHRONISES the stream: hint_ptr, node_ptr (with node_dist) and the
 * work-list length every few rounds are read back. */
int ggc_geodesic_hints(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const int32_t* hints,
                       const int32_t* hint_ptr, int radius, int gamma, const int32_t* segments, const int32_t* node_ptr,
                       uint8_t* mask, int32_t* dist_fg, int32_t* dist_bg, int32_t* node_dist);

/* H2 — brush strokes as hard constraints (additive): the drag of a brush, where ggc_apply_hints has single clicks.  One exact
 * integer definition; no float is involved anywhere.
 *   strokes    [dev] i32 [S,5] = (r0, c0, r1, c1, label) straight segments, label 0 = background, nonzero = foreground;
 *              grouped by image, order kept within an image.  A polyline of n >= 2 vertices is its n-1 segments, a
 *              one-vertex stroke one segment with both ends equal.  |coordinate| <= 2^20; endpoints may lie outside the
 *              image and the part inside is painted (a CLICK outside the image is ignored; a stroke is clipped).
 *   stroke_ptr [dev] i32 [B+1]  image b owns strokes[stroke_ptr[b] .. stroke_ptr[b+1]); stroke_ptr[0] = 0, non-decreasing
 *   radius     0 .. 16384, the brush radius in pixels
 *   mask       [dev] u8 [B,H,W] in/out GrabCut labels
 * Rule: for pixel p and segment a -> b let w = p - a, d = b - a, L2 = d.d, t = w.d.  dist^2(p, segment) is |w|^2 if t <= 0,
 * |p - b|^2 if t >= L2, else (w x d)^2 / L2.  p is WITHIN RHO of the segment iff 4 dist^2 <= rho4 = max(4 radius^2, 1); the third
 * case is decided as 4 (w x d)^2 <= rho4 L2, without division, in 128-bit integers (t and w x d fit int64 under the limits
 * above; the squares do not).  radius >= 1: the closed capsule of that radius, boundary included, as dy*dy + dx*dx <=
 * radius*radius is for clicks, so a one-vertex stroke paints exactly ggc_apply_hints' disk.  radius == 0: the CENTRE LINE, the
 * pixels within half a pixel of the segment: 8-connected, holds both endpoints, exact half-pixel ties included.
 * ggc_apply_strokes: every in-image pixel within rho of a segment of its image becomes GGC_FGD or GGC_BGD; where segments
 * overlap the image's LAST segment wins, by index and not by timing; a pixel no stroke touches is neither read nor written.
 * Work is O(pixels + 32x8 tiles x segments), independent of the strokes' lengths; every image's result equals that of its
 * single-image call bit for bit.
 * B == 0 or stroke_ptr[B] == 0 is a no-op: nothing is written.  B, H or W outside 1..65535 is GGC_E_SHAPE; radius out of
 * range, a NULL stroke_ptr or mask, NULL strokes with segments, stroke_ptr[0] != 0, a decreasing stroke_ptr or an endpoint
 * beyond +-2^20 is GGC_E_INVALID_ARG, all before any launch.  SYNCHRONISES the stream: stroke_ptr and the segments are read
 * back and checked on the host. */
int ggc_apply_strokes(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* strokes, const int32_t* stroke_ptr,
                      int radius, uint8_t* mask);

/* H2 — the centre-line pixels of a batch's strokes (the radius == 0 rule above) inside the image, as a click list in
 * ggc_apply_hints' packing, so that a stroke can go wherever clicks go (superpixel regions, prior columns, geodesic sources).
 *   hint_ptr_out [dev] i32 [B+1] out, always written: image b owns rows hint_ptr_out[b] .. hint_ptr_out[b+1)
 *   hints_out    [dev] i32 [capacity,3] out = (row, col, label 1 | 0), or NULL: only the counts are produced (call once with
 *                NULL, allocate hint_ptr_out[B] rows, call again: the pattern of ggc_graph_count / ggc_graph_fill)
 * Rows are grouped by image, each image in raster order, each pixel once; a pixel's label is that of the image's last segment
 * whose centre line holds it.  Integer sums only, no atomics: the list does not depend on launch order.  A non-NULL
 * hints_out with capacity < hint_ptr_out[B] is GGC_E_INVALID_ARG with nothing written to hints_out.  B == 0 is a no-op; with
 * B >= 1 and no segments hint_ptr_out is all zeros and nothing else is written.  Arguments are checked as for
 * ggc_apply_strokes; also B*H*W must fit int32 (GGC_E_SHAPE).  Scratch: one byte per pixel and 4 bytes per row.
 * SYNCHRONISES the stream: stroke_ptr and the segments are read back and checked, and with hints_out the total is read. */
int ggc_stroke_pixels(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* strokes, const int32_t* stroke_ptr,
                      int32_t* hint_ptr_out, int32_t* hints_out, int64_t capacity);

/* H3 — lassos and filled polygons as hard constraints (additive): areas, where ggc_apply_strokes has lines.  One exact integer
 * definition; no float is involved anywhere.
 *   verts      [dev] i32 [V,2] = (row, col) vertices, grouped by polygon; |coordinate| <= 2^20; vertices may lie outside the image
 *   poly_ptr   [dev] i32 [P+1]  polygon q owns verts[poly_ptr[q] .. poly_ptr[q+1]), at least 3 of them; poly_ptr[0] = 0,
 *              V = poly_ptr[P].  A polygon is closed implicitly, last vertex to first; it may intersect itself.
 *   poly_label [dev] i32 [P]    0 = background fill, 1 = foreground fill, 2 = lasso
 *   image_ptr  [dev] i32 [B+1]  image b owns polygons image_ptr[b] .. image_ptr[b+1); image_ptr[0] = 0, image_ptr[B] = P
 *   mask       [dev] u8 [B,H,W] in/out GrabCut labels
 * Rule: pixel p = (r, c) is COVERED by a polygon iff (a) or (b) holds.
 *   (a) p lies on an edge a -> b: (b.r - a.r)(c - a.c) - (b.c - a.c)(r - a.r) == 0 and p is inside the edge's bounding box.
 *       The covered set is therefore closed, as the click disk and the stroke capsule are.
 *   (b) the crossing number is odd (even-odd rule): an edge counts iff (a.r <= r) != (b.r <= r), half-open in rows so that a
 *       horizontal edge never counts, and it crosses strictly to the right of p: with lo / hi the edge's ends ordered by row,
 *       (hi.c - lo.c)(r - lo.r) - (c - lo.c)(hi.r - lo.r) > 0.
 * Under the limits every product stays below 2^44: plain int64, no 128-bit compare.
 * Per image, in this order: (1) LASSOS: if the image has at least one lasso, every in-image pixel covered by none of its
 * lassos becomes GGC_BGD (lassos form a union; pixels inside a lasso are not touched); (2) FILLS, in polygon order: every
 * in-image pixel a fill covers becomes GGC_FGD (label 1) or GGC_BGD (label 0); where fills overlap the image's LAST fill
 * wins, by index and not by timing.  A pixel that neither step touches is neither read nor written.  No atomics; every
 * image's result equals that of its single-image call bit for bit.  Work is O(pixels + 32x8 tiles x edges): a tile sees the
 * edges of the polygons whose bounding box meets it, less those whose row span misses the tile's rows or that lie wholly
 * left of it.  Scratch: 16 bytes per polygon.
 * B == 0 is a no-op whatever the other arguments hold, as for ggc_apply_strokes; otherwise B, H or W outside 1..65535 is
 * GGC_E_SHAPE and a negative P GGC_E_INVALID_ARG, and then P == 0 is a no-op too (no pointer is looked at): nothing is
 * written.  With P >= 1, a NULL mask, image_ptr, poly_ptr, poly_label or verts, image_ptr or poly_ptr not starting at 0 or decreasing, image_ptr[B] != P, a
 * polygon of fewer than 3 vertices, a label outside {0, 1, 2} or a coordinate beyond +-2^20 is GGC_E_INVALID_ARG, all before
 * any launch.  SYNCHRONISES the stream: the four arrays are read back and checked on the host. */
int ggc_apply_polygons(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* verts, const int32_t* poly_ptr,
                       const int32_t* poly_label, const int32_t* image_ptr, int P, uint8_t* mask);

/* H4 — intelligent scissors (additive; live-wire, Mortensen & Barrett 1995): the user clicks a few anchors on an object's
 * outline and consecutive anchors are joined by the cheapest 8-connected path along image edges.  One exact integer
 * definition; no float is involved anywhere.
 *   bgr         [dev] u8  [B,H,W,3] the images (the guide)
 *   anchors     [dev] i32 [A,2] = (row, col), grouped by path, every anchor inside its image
 *   path_ptr    [dev] i32 [Q+1]  path q owns anchors[path_ptr[q] .. path_ptr[q+1]); path_ptr[0] = 0, A = path_ptr[Q]
 *   path_closed [dev] i32 [Q]    0 = open (at least 2 anchors), 1 = closed (at least 3)
 *   image_ptr   [dev] i32 [B+1]  image b owns paths image_ptr[b] .. image_ptr[b+1); image_ptr[0] = 0, image_ptr[B] = Q
 *   margin 0 .. 256      edge_cap 1 .. 13 770      smooth 1 .. 64
 *   vert_ptr_out [dev] i32 [Q+1] out, always written: path q owns rows vert_ptr_out[q] .. vert_ptr_out[q+1)
 *   verts_out    [dev] i32 [capacity,2] out = (row, col), or NULL: only the counts are produced (call once with NULL, allocate
 *                vert_ptr_out[Q] rows, call again: the pattern of ggc_stroke_pixels).  The pair is exactly ggc_apply_polygons'
 *                verts and poly_ptr: a traced batch goes into the painter without repacking.
 * Guide: S_c(y,x) is H1's 3x3 box sum with replicated border.  The gradient is
 *   G(p) = sum over c of |S_c(y, x+1) - S_c(y, x-1)| + |S_c(y+1, x) - S_c(y-1, x)|,
 * the coordinates clamped into the image, 0 .. 6 * 2295 = 13 770.  The flatness is F(p) = ((edge_cap - min(G(p), edge_cap)) * 255)
 * / edge_cap, floor division: 0 on a strong edge, 255 on flat ground.
 * Arcs: the grid is 8-connected and c(p,q) = L(p,q) * (smooth + F(p) + F(q)), L = 80 axial, 113 diagonal (H1's step lengths);
 * symmetric, at least 80.
 * Segments: an open path of n anchors has the n - 1 segments a_i -> a_(i+1); a closed one n segments, the last a_(n-1) -> a_0.
 * A segment's WINDOW is the bounding box of its two anchors grown by `margin` pixels on every side and clipped to the image;
 * the cheapest path is sought inside the window only.  Consecutive anchors are at most 1024 apart (Chebyshev).
 * Distance: for segment a -> b, D(p) = cost of the cheapest path inside the window from p to b; D(b) = 0.  D is unique
 * whatever the relaxation order.
 * Ranges: an arc is at most 113 * (64 + 510) = 64 862; a window side is at most 1024 + 1 + 512 = 1537 pixels and every window
 * pixel reaches b in at most 1536 arcs (king moves inside the box), so D <= 1536 * 64 862 < 2^27.  "Unreached" is 2^30 and an arc
 * that leaves the window costs 2^29, so every sum the relaxation forms stays at or below 2^30 + 2^29: everything fits int32.
 * Path: starting at p = a, while p != b: emit p, then move to the first neighbour q, in the order N, NE, E, SE, S, SW, W, NW
 * (N = row - 1, E = col + 1), that lies in the window and has D(q) + c(p,q) == D(p).  D falls by at least 80 per step, so the
 * walk ends, and it is unique because D is.  A segment contributes its pixels from a inclusive to b exclusive; an open path
 * appends its last anchor; a segment with a == b contributes nothing.  The vertices of path q are its segments' pixels in
 * order.  Every path's result equals that of its single-image, single-path call bit for bit.
 * B == 0 or Q == 0 is a no-op: nothing is written.  Otherwise, before any launch: H or W outside 1..65535 or B outside
 * 0..65535 is GGC_E_SHAPE; GGC_E_INVALID_ARG for a negative Q, a parameter out of range, a NULL pointer (verts_out excepted),
 * image_ptr or path_ptr not starting at 0 or decreasing, image_ptr[B] != Q, path_closed outside {0, 1}, an open path of fewer
 * than 2 or a closed one of fewer than 3 anchors, an anchor outside its image, consecutive anchors more than 1024 apart, windows
 * that hold more than 2^26 pixels or more than 2^21 tiles of 32x32 in all, and (after the counting pass) a non-NULL verts_out
 * with capacity < vert_ptr_out[Q], with nothing written to verts_out.
 * The relaxation runs in rounds, one launch each; past 1024 * (tiles of the largest window) + 2 rounds it returns
 * GGC_E_DEVICE "scissors did not converge" (it cannot hang).  Scratch: 5 bytes per window pixel, 16 per tile, 72 per segment;
 * ggc_debug_read_scratch "scissors_planes" reads the D planes of the last call, segment after segment in path order, each its
 * window row-major, i32.  SYNCHRONISES the stream: the four input arrays, the work-list length every few rounds and the vertex
 * total are read back. */
int ggc_trace_paths(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const int32_t* anchors,
                    const int32_t* path_ptr, const int32_t* path_closed, const int32_t* image_ptr, int Q, int margin, int edge_cap,
                    int smooth, int32_t* vert_ptr_out, int32_t* verts_out, int64_t capacity);

/* H5 — magic wand (additive): a seed selects the pixels that look like it, where every other tool defines a region by geometry
 * or by a path cost.  One exact integer definition; no float and no division is involved anywhere.
 *   bgr       [dev] u8  [B,H,W,3] the images
 *   seeds     [dev] i32 [K,3] = (row, col, label), label 0 = background / subtract, nonzero = foreground / add
 *   seed_ptr  [dev] i32 [B+1]  image b owns seeds[seed_ptr[b] .. seed_ptr[b+1]); seed_ptr[0] = 0, non-decreasing
 *             (ggc_apply_hints' packing).  A seed outside its image is ignored.
 *   tolerance 0 .. 255      connectivity 4, 8 or 0 = not contiguous ("select similar")      sample n in {1, 3, 5}
 *   mask      [dev] u8  [B,H,W] in/out GrabCut labels, may be NULL
 *   select    [dev] u8  [B,H,W] out, may be NULL
 *   counts    [dev] i32 [B,2]   out, may be NULL                          (at least one of the three must be given)
 * Reference colour of seed s at (r, c): ref_c(s) = sum of the n x n bytes I_c(clamp(r+dy, 0, H-1), clamp(c+dx, 0, W-1)), |dy|, |dx|
 * <= n / 2: a box sum with replicated border, as H1's guide.
 * Match: match(p, s) iff for all three channels |n^2 I_c(p) - ref_c(s)| <= n^2 tolerance: the max-channel metric against the
 * window's mean, without the division.  The largest value is 25 * 255 = 6375: everything fits int32.
 * Selection: Sel(s) = { p : match(p, s) } when connectivity == 0; otherwise the 4- or 8-connected component, within that set, of
 * the seed's own pixel.  If the seed's own pixel does not match its reference (possible with sample > 1), Sel(s) is empty.
 * Combination, per image: a pixel is DECIDED by the last seed of its image, in seed order, whose Sel holds it; by index and
 * not by timing.
 *   mask     a decided pixel becomes GGC_FGD or GGC_BGD; an undecided pixel is neither read nor written
 *   select   written for every pixel: 255 if a foreground seed decided it, 0 if a background seed did or nothing did (a later
 *            background seed subtracts)
 *   counts   [b] = (pixels decided by a foreground seed, by a background seed), written for every image, by integer atomics
 * The result is a set defined without reference to any schedule; every image's outputs equal those of its single-image call
 * bit for bit; the pass size (below) never changes an output.
 * B == 0 or K = seed_ptr[B] == 0 is a no-op: select and counts are not written.  Otherwise, before any launch: B, H or W outside
 * 1..65535 or H*W beyond int32 is GGC_E_SHAPE; a tolerance, connectivity or sample outside its set, a NULL bgr or seed_ptr, NULL
 * seeds with K > 0, seed_ptr[0] != 0, a decreasing seed_ptr or all three outputs NULL is GGC_E_INVALID_ARG.
 * Schedule: contiguous selections label one plane per live seed by union-find (csrc/ggc_ccl.h), S seeds per pass: as many as
 * keep the parent maps (4 bytes per pixel per seed) within 1 GiB, at least one, unless GGC_WAND_SEEDS_PER_PASS fixes S; passes
 * run in seed order.  Scratch: those maps, one byte per pixel of the batch, 24 bytes per seed.  connectivity == 0 is one
 * streaming launch without scratch planes.  SYNCHRONISES the stream: seed_ptr and the seeds are read back, the live seeds'
 * table is uploaded. */
int ggc_wand_select(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const int32_t* seeds,
                    const int32_t* seed_ptr, int tolerance, int connectivity, int sample, uint8_t* mask, uint8_t* select,
                    int32_t* counts);

/* C0 — next simulated click per image (additive; the standard NoC protocol of interactive segmentation).
 *   pred [dev] u8  [B,H,W]  current binary mask (nonzero = foreground)
 *   gt   [dev] u8  [B,H,W]  ground truth (nonzero = foreground; {0,1} and {0,255} both work)
 *   out  [dev] i32 [B,4]    row, col, label (1 = fg, 0 = bg), d2; row = col = label = -1, d2 = 0 when pred == gt
 * fn = gt & !pred, fp = !gt & pred.  d2(p) of a pixel of region R is the smallest squared Euclidean distance to a pixel
 * not in R, pixels outside the image counting as not in R (ndimage.distance_transform_edt(np.pad(R, 1))[1:-1, 1:-1]**2).
 * With Mfn, Mfp the maxima of d2 over fn and fp, the click is positive (in fn) iff Mfn > Mfp, else negative (in fp): a
 * tie goes to the background click.  It lies at the chosen region's pixel of largest d2, the smallest raster index
 * y*W + x among equals.  Integer arithmetic and integer atomics only: the result does not depend on launch order.
 * H <= 65535 and W <= 8192, else GGC_E_INVALID_ARG (as for B < 0 or B > 65535); B == 0 is a no-op.  Scratch: 4 bytes
 * per pixel from the context.  Does not synchronise. */
int ggc_next_click(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                   const uint8_t* pred, const uint8_t* gt, int32_t* out);

/* K0 — replaces clean_mask (pipeline.py:189-227); 8-connected components.
 *   mask_in/mask_out [dev] u8 [B,H,W] in {0,1} (may alias) */
int ggc_clean_mask(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                   const uint8_t* mask_in, float min_area_ratio, int keep_largest,
                   uint8_t* mask_out);

/* K1 — mask outlines: the exact vector contours of a mask, traced on the device.  Additive; integer only.
 *   mask [dev] u8 [B,H,W]: any nonzero byte is foreground, everything outside the image is background.
 * CORNER LATTICE.  The corners of an H x W image are the points (r, c), 0 <= r <= H, 0 <= c <= W; pixel (y, x) is the unit
 * square between corners (y, x) and (y+1, x+1).
 * CRACKS.  A crack is a directed unit step between two corners with a foreground pixel on its right and a background pixel
 * on its left.  Row grows downwards, so a step east has "below" on its right.  Directions: 0 = E (c+1), 1 = S (r+1), 2 = W,
 * 3 = N.  A crack leaves (r, c) in direction d iff
 *   E: pixel (r, c) fg and (r-1, c) bg        S: (r, c-1) fg and (r, c) bg
 *   W: (r-1, c-1) fg and (r, c-1) bg          N: (r-1, c) fg and (r-1, c-1) bg.
 * Its key is ((r (W+1) + c) 4 + d) of its tail.  An image has at most 2HW + H + W cracks, one per unit edge
 * (the checkerboard has all but the border edges of its clear pixels).
 * SUCCESSOR.  The successor of a crack that arrives at corner v in direction d is the first crack that exists among those
 * leaving v: connectivity 8 tries left (d+3)&3, straight d, right (d+1)&3, in that order; connectivity 4 tries right,
 * straight, left.  The orders differ only at saddle corners (two diagonal foreground pixels in the 2x2 block): 8 joins the
 * two pixels into one loop, 4 separates them.  Everywhere else exactly one candidate exists; a U-turn never does.
 * LOOPS.  Successor is a permutation of the cracks; its cycles are the loops.  A loop STARTS at its crack of smallest key;
 * that crack's tail is the loop's lexicographically smallest corner, the loop visits it once and turns there, no other loop
 * starts at it, and the start points E for an outer loop and S for a hole.  The VERTICES of a loop are the tails of those of
 * its cracks whose predecessor has another direction, in loop order from the start: an even number, at least 4.
 * ORDER AND RECORDS.  An image's loops are ordered by start key.  Per loop:
 *   area       half the shoelace sum  sum c_i r_(i+1) - c_(i+1) r_i  over its vertices, an exact integer: positive for an outer
 *              loop (clockwise on screen), negative for a hole.  The areas of an image sum to its foreground pixel count.
 *   perimeter  the loop's crack count.
 *   outer      the index, within the image, of the outer loop of the loop's component: the component, under `connectivity`,
 *              of the foreground pixel right of the start crack.  An outer loop names itself.
 * An image has as many outer loops as foreground components under `connectivity`, and as many holes as background
 * components under the dual connectivity that do not reach the border.  XOR-ing the even-odd fills of an image's loops gives
 * the mask back: double every coordinate, fill on a (2H+1) x (2W+1) grid by H3's rule, read the odd positions.
 *   image_ptr_out      [dev] i32 [B+1], always written: image b owns loops image_ptr_out[b] .. image_ptr_out[b+1)
 *   image_vert_ptr_out [dev] i32 [B+1], always written: ... and rows image_vert_ptr_out[b] .. [b+1) of verts_out
 *   loop_ptr_out       [dev] i32 [loop_capacity+1] or NULL: loop q owns rows loop_ptr_out[q] .. [q+1) of verts_out
 *   loop_info_out      [dev] i32 [loop_capacity,3] = area, outer, perimeter; or NULL
 *   verts_out          [dev] i32 [vert_capacity,2] = (row, col) corners; or NULL
 * The three fill arrays are NULL together (count only: read the totals at image_ptr_out[B] and image_vert_ptr_out[B], the
 * pattern of ggc_stroke_pixels) or all given; loop_ptr_out and verts_out are exactly ggc_apply_polygons' poly_ptr and verts.
 * Every image's result equals that of its single-image call, bit for bit.  B == 0 is a no-op.
 * Refused before any launch: H or W outside 1..65535 or B outside 0..65535 (GGC_E_SHAPE); (H+1)(W+1) > 2^28, so that keys
 * and areas fit int32, a connectivity other than 4 or 8, a NULL mask or image array, only some of the fill arrays, a
 * negative capacity (GGC_E_INVALID_ARG).  Refused after the counting pass: a capacity below the totals
 * (GGC_E_INVALID_ARG), with nothing written to the three fill arrays.
 * SYNCHRONISES the stream: the crack, loop and vertex totals are read back (three small reads per image group).  Scratch
 * from the context: 0.6 bytes per corner (a bitmap over the crack keys and a prefix per 64 corners), 4 bytes per pixel for
 * the component labelling, and 57 bytes per crack (key, successor, two ranking states, loop index).  A batch of more than
 * 2^26 corners is worked through in image groups of at most that many, with identical results; a filling call then counts
 * every group twice. */
int ggc_mask_outlines(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* mask, int connectivity,
                      int32_t* image_ptr_out, int32_t* image_vert_ptr_out, int32_t* loop_ptr_out, int32_t* loop_info_out,
                      int32_t* verts_out, int64_t loop_capacity, int64_t vert_capacity);

/* K2 — exact distance transform of a mask.  Additive; integer only.
 *   mask [dev] u8 [B,H,W]: any nonzero byte is foreground.   signed_d2_out [dev] i32 [B,H,W].
 * DISTANCE.  Between pixels (y, x) and (y', x') it is d2 = (y-y')^2 + (x-x')^2, the squared Euclidean distance of their centres.
 *   background pixel p:  out[p] = +min over foreground q of d2(p, q)   (>= 1)
 *   foreground pixel p:  out[p] = -min over background q of d2(p, q)   (<= -1)
 * so the output is never 0 and its sign gives the mask back.
 * BORDER.  With flags bit 0, GGC_DIST_BORDER_BG, every position outside the image counts as background (K1's convention): a
 * foreground pixel of row y is then at most min(y+1, H-y)^2 from background, and likewise in x.  Without the bit nothing
 * exists outside the image (scipy.ndimage.distance_transform_edt's convention).  Foreground never exists outside the image.
 * FAR.  Where no opposite pixel exists the magnitude is GGC_DIST_FAR = INT32_MAX (an all-foreground image without the bit is
 * -GGC_DIST_FAR everywhere).
 * CAP.  max_dist2 == 0: unbounded.  max_dist2 > 0: every magnitude greater than max_dist2 is reported as GGC_DIST_FAR, and
 * the row pass looks at most floor(sqrt(max_dist2)) columns to each side, which is what makes a small radius cheap.
 * METHOD.  A column pass leaves per pixel the 16-bit distance g, within its column, to the nearest pixel of the other class
 * (all ones in its 15 bits = none, the pixel's class in bit 15); a row pass takes min over x' of g(y,x')^2 + (x-x')^2 with the
 * row staged in LDS, walking outward from x until k^2 reaches the best so far (csrc/ggc_edt.h).  Exact in every case; an
 * unbounded call costs O(distance to the answer) per pixel, O(W) where the only opposite pixel is far away.
 * Every image's result equals that of its single-image call, bit for bit.  B == 0 is a no-op.
 * Refused before any launch: H or W outside 1..16384, or B*H*W >= 2^31 (GGC_E_SHAPE); a NULL pointer with B > 0, unknown
 * flag bits, a negative max_dist2 (GGC_E_INVALID_ARG).
 * No host synchronisation, nothing of data-dependent size.  Scratch from the context: 2 bytes per pixel (g). */
#define GGC_DIST_BORDER_BG 1
#define GGC_DIST_FAR 2147483647
int ggc_mask_distance(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* mask, int flags, int64_t max_dist2,
                      int32_t* signed_d2_out);

/* K3 — modify a mask by a distance: thresholds of K2, fused into its row pass (no int32 plane is written).
 *   mask_in [dev] u8 [B,H,W], any nonzero byte foreground.   out [dev] u8 [B,H,W]; may alias mask_in.
 * D_out(p) / D_in(p) are K2's magnitudes of a background / foreground pixel.  r2_a, r2_b are SQUARED radii: the disk is
 * dy^2 + dx^2 <= r2 (r2 = 1: the 4-neighbourhood, r2 = 2: the 8-neighbourhood).
 *   op 0 GROW    1 where fg or D_out <= r2_a (dilation by the exact disk)
 *   op 1 SHRINK  1 where fg and D_in > r2_a
 *   op 2 BORDER  1 where (fg and D_in <= r2_a) or (bg and D_out <= r2_b): GROW(r2_b) minus SHRINK(r2_a)
 *   op 3 OPEN    GROW(r2_a) of SHRINK(r2_a)
 *   op 4 CLOSE   SHRINK(r2_a) of GROW(r2_a)
 *   op 5 TRIMAP  255 where fg and D_in > r2_a, 0 where bg and D_out > r2_b, else 128 (what O3t reads as a trimap)
 * flags as K2; the bit bears on every shrink step (D_in).  r2 = 0 makes GROW and SHRINK the identity normalised to {0,1} and
 * BORDER empty.  r2_b must be 0 for ops 0, 1, 3, 4.  Each step runs K2 capped at its own radius; OPEN and CLOSE run two steps
 * on the device through a u8 plane of scratch, with no host round trip.
 * Refused before any launch: as K2, and an unknown op, a negative radius, a nonzero r2_b where it has no meaning
 * (GGC_E_INVALID_ARG).  Scratch: 2 bytes per pixel, 3 for OPEN and CLOSE. */
#define GGC_MODIFY_GROW 0
#define GGC_MODIFY_SHRINK 1
#define GGC_MODIFY_BORDER 2
#define GGC_MODIFY_OPEN 3
#define GGC_MODIFY_CLOSE 4
#define GGC_MODIFY_TRIMAP 5
int ggc_modify_mask(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* mask_in, int op, int64_t r2_a,
                    int64_t r2_b, int flags, uint8_t* out);

/* O0 — replaces GrabCut.overlay_mask / crop_foreground (grabcut.py:180-195).
 *   overlay [dev] u8 [B,H,W,3]   rgba [dev] u8 [B,H,W,4]   (either may be NULL) */
int ggc_compose_outputs(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                        const uint8_t* bgr, const uint8_t* binary,
                        float alpha, int tint_b, int tint_g, int tint_r,
                        uint8_t* overlay, uint8_t* rgba);

/* O1 — soft alpha matte of a binary mask: colour guided filter (guide = bgr / 255, input = binary), BORDER_REFLECT_101
 * (additive; He, Sun and Tang's guided filter used for feathering).
 *   bgr [dev] u8 [B,H,W,3]   binary [dev] u8 [B,H,W] (nonzero = 1: any nonzero byte counts as foreground)
 *   1 <= radius <= 64, 1e-12 <= eps < inf (else GGC_E_INVALID_ARG); windows larger than the image are legal
 *   alpha [dev] f32 [B,H,W] in [0,1] or NULL;  rgba [dev] u8 [B,H,W,4] (bgr, round(255 alpha)) or NULL (not both NULL)
 * The window sums are exact: integers for the covariances, int64 fixed point (rounding below 2^-28) for the averages of
 * the coefficients, so a pixel farther than 2*radius from any mask change gets exactly the mask value.  The 3x3 solve runs
 * in float64.  Every image's result is independent of the batch it is in (bit for bit).  Scratch: 32 bytes per pixel from the context.
 * Does not synchronise. */
int ggc_alpha_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const uint8_t* binary,
                    int radius, float eps, float* alpha, uint8_t* rgba);

/* O2 — the soft matte of O1 at a larger resolution (additive; He and Sun's fast guided filter): the mean coefficients
 * C = (mean a / 255, mean b) of ggc_alpha_matte's stage 2 at the working resolution, interpolated bilinearly to the
 * full resolution and applied to the full-resolution colours.
 *   bgr [dev] u8 [B,H,W,3], binary [dev] u8 [B,H,W] (nonzero = foreground), radius and eps: as ggc_alpha_matte
 *   bgr_full [dev] u8 [B,H1,W1,3] with H <= H1 <= 32768, W <= W1 <= 32768 (else GGC_E_SHAPE, as for B outside 1..65535)
 * For output pixel (y, x), in float64: sx = ((x + 0.5) * W) / W1 - 0.5, raised to 0 if negative; x0 = floor(sx), and
 * x0 = W - 1 with wx = 0 when x0 >= W - 1, else wx = sx - x0; x1 = min(x0 + 1, W - 1); the same for y with H, H1
 * (cv2.resize INTER_LINEAR's half-pixel centres).  c_k = lerp(lerp(C_k[y0,x0], C_k[y0,x1], wx), lerp(C_k[y1,x0],
 * C_k[y1,x1], wx), wy) with lerp(u, v, t) = u + t (v - u), and alpha = clamp(c_0 B + c_1 G + c_2 R + c_3, 0, 1) with the
 * full-resolution bytes, summed in ggc_alpha_matte's order.
 *   alpha_full [dev] f32 [B,H1,W1] = (float)alpha       binary_full [dev] u8 [B,H1,W1] = alpha >= 0.5 (on the double)
 *   rgba_full [dev] u8 [B,H1,W1,4] = bgr_full, floor(255 alpha + 0.5)      (each may be NULL, not all three)
 * With H1 = H, W1 = W and bgr_full = bgr every weight is 0: alpha_full and rgba_full are ggc_alpha_matte's outputs bit
 * for bit.  A pixel whose four source pixels lie farther than 2*radius from every change of the mask gets exactly that
 * mask value.  Every image's result is independent of the batch it is in (bit for bit); no atomics.  Scratch: 64 bytes
 * per working pixel from the context.  Does not synchronise. */
int ggc_upsample_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const uint8_t* binary,
                       int H1, int W1, const uint8_t* bgr_full, int radius, float eps,
                       float* alpha_full, uint8_t* binary_full, uint8_t* rgba_full);

/* O3 — closed-form alpha matte of a binary mask (additive; Levin, Lischinski and Weiss, TPAMI 2008, with He, Sun and
 * Tang's matrix-free L p, CVPR 2010).  Per image, with I_i = bgr_i / 255 and m = (binary != 0):
 *   windows   K = {k : r <= y_k < H-r, r <= x_k < W-r} (only windows wholly inside the image: L stays symmetric), w_k the
 *             (2r+1)^2 window at k, n = (2r+1)^2; mu_k the window mean of I, Sigma_k its population covariance,
 *             Delta_k = Sigma_k + (eps / n) U (Levin's convention)
 *   L         = sum_{k in K} L_k, (L_k)_ij = delta_ij - (1/n) (1 + (I_i - mu_k)^T Delta_k^-1 (I_j - mu_k)), i, j in w_k;
 *             L 1 = 0, and with eps > 0 its null space is the constants
 *   L p       a_k = Delta_k^-1 (mean_k(I p) - mu_k mean_k(p)), b_k = mean_k(p) - a_k^T mu_k,
 *             (L p)_i = c_i p_i - sum_{k in K, i in w_k} (a_k^T I_i + b_k), c_i = #{k in K : i in w_k}
 *   U         the pixels within Chebyshev distance `band` of a pixel whose 3x3 neighbourhood (clipped to the image) holds
 *             both mask values; every other pixel is known, alpha = m
 *   solve     L_UU alpha_U = -L_{U,known} m_known by Jacobi-preconditioned CG (preconditioner diag L on U) from alpha = m;
 *             an image stops when ||r_j||_2 <= tol ||r_0||_2 (unpreconditioned residual, r_0 = -(L m)_U) or after
 *             max_iter iterations.  An image whose U is empty or covers every pixel gets alpha = m and 0 iterations.
 *   bgr [dev] u8 [B,H,W,3]   binary [dev] u8 [B,H,W] (any nonzero byte is 1)
 *   1 <= radius <= 8, 1e-12 <= eps <= 1, 0 <= band <= 64, 1 <= max_iter <= 100000, 1e-12 <= tol < 1 (else
 *   GGC_E_INVALID_ARG); H, W >= 2 radius + 1, H, W <= 32768, B <= 65535 (else GGC_E_SHAPE); B == 0 does nothing
 *   alpha [dev] f32 [B,H,W] = clamp(alpha, 0, 1)     rgba [dev] u8 [B,H,W,4] = bgr, floor(255 clamp(alpha) + 0.5)
 *   raw [dev] f64 [B,H,W] = alpha unclamped         iters [dev] i32 [B]     rel_residual [dev] f64 [B] = ||r_j|| / ||r_0||
 *   (each may be NULL, not all of them; rel_residual is 0 for an image with 0 iterations)
 * mu_k and Sigma_k come from exact integer window sums, Delta_k^-1 from the adjugate in float64; the CG vectors and dot
 * products are float64.  Every per-image reduction runs in one fixed order over that image's tiles, so every image's
 * outputs equal its single-image call bit for bit; no float atomics.  Work is restricted to the 16 x 16 tiles that hold U
 * and their neighbours, listed once per call.  The entry SYNCHRONISES its stream: once to build that list on the host,
 * and every 8 iterations to read the count of converged images (an integer atomic) and stop when all are done.
 * Scratch: 147 bytes per pixel plus 28 bytes per 16 x 16 tile and 56 bytes per image, from the context. */
int ggc_closed_form_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const uint8_t* binary,
                          int radius, float eps, int band, int max_iter, float tol,
                          float* alpha, uint8_t* rgba, double* raw, int32_t* iters, double* rel_residual);

/* O3t — closed-form alpha matte on the unknown region of a caller's trimap (additive): the system of O3 with the unknown
 * set, the known values and the start taken from the caller instead of from a mask's edge.  Per image, with K, Delta_k, L
 * and the matrix-free L p exactly those of O3:
 *   regions   F = {trimap == 255}, G = {trimap == 0}, U = every other byte; alpha = 1 on F, 0 on G
 *   start     alpha_U = alpha0 read as float64 and clamped to [0, 1] (a NaN reads as 0), or 0.5 when alpha0 is NULL;
 *             alpha0 is read on U only
 *   solve     L_UU alpha_U = -L_{U,F} 1_F by the Jacobi-preconditioned CG of O3; an image stops when
 *             ||r_j||_2 <= tol ||r_0||_2 or after max_iter iterations, r_0 = -(L x0)_U the unpreconditioned residual of the
 *             start image x0 (the known values off U, the start on U), one application of L
 *   trivial   an image whose U is empty, or covers every pixel (nothing anchors the system: it is singular), or whose
 *             r_0 is 0, gets the start image, 0 iterations and rel_residual 0.  An image with G but no F is not special:
 *             its solution is alpha_U = 0 and CG goes there
 *   bgr [dev] u8 [B,H,W,3]   trimap [dev] u8 [B,H,W]   alpha0 [dev] f32 [B,H,W] or NULL
 *   radius, eps, max_iter, tol, the shape limits, the error codes, B == 0 and the five outputs with their NULL rule: as
 *   O3 (there is no band)
 * The two entries share one solver: after the flag plane, the start and the per-tile counts of U are written (O3: by the
 * band kernels; here: by one kernel over the trimap), the same tile list, set-up and iteration kernels run.  With
 * trimap = 128 on O3's U, else 255 m, and alpha0 = m, every output equals O3's bit for bit.  Reductions, batch
 * independence, atomics and the synchronisation of the stream are O3's.
 * Scratch: 145 bytes per pixel plus 28 bytes per 16 x 16 tile and 56 bytes per image, from the context. */
int ggc_trimap_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const uint8_t* trimap,
                     int radius, float eps, int max_iter, float tol, const float* alpha0,
                     float* alpha, uint8_t* rgba, double* raw, int32_t* iters, double* rel_residual);

/* O3w — O3t with a stop rule that does not move with the start (additive; for warm starts).  O3t stops an image on
 * ||r_j|| <= tol ||r_0|| with r_0 the residual of its own start: a good start has a small r_0 and earns nothing.  Here
 * the reference is the residual of the 0.5 start, whatever alpha0 holds:
 *   r_ref     = -(L x^1/2)_U, x^1/2 the known values off U and 0.5 on U: one more application of L in the set-up
 *   stop      an image stops when ||r_j||_2 <= tol ||r_ref||_2 or after max_iter iterations; the test is made on r_0 too,
 *             so a start that is already good enough comes back as it is, with 0 iterations
 *   trivial   the cases of O3t with r_ref = 0 in the place of r_0 = 0
 *   rel_residual = ||r_j|| / ||r_ref|| (||r_0|| / ||r_ref|| for an image that stopped on its start, 0 for a trivial one)
 * alpha0 is required (NULL is GGC_E_INVALID_ARG); every other argument, limit, error code and output is O3t's.  The
 * system, the CG and its kernels are O3t's; only the number an image's residual is divided by differs.  With alpha0 = 0.5
 * on U every output equals ggc_trimap_matte(alpha0 = NULL) bit for bit.  Reductions, batch independence, atomics and the
 * synchronisation of the stream are O3's.
 * Scratch: 145 bytes per pixel plus 28 bytes per 16 x 16 tile and 56 bytes per image, from the context (the reference
 * pass reuses the set-up's arrays). */
int ggc_trimap_matte_warm(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const uint8_t* trimap,
                          int radius, float eps, int max_iter, float tol, const float* alpha0,
                          float* alpha, uint8_t* rgba, double* raw, int32_t* iters, double* rel_residual);

/* O3l — a working-size trimap and alpha carried to a larger size (additive): the trimap and the start of a closed-form
 * solve on the full image (O3w) from a solve at the working size.
 *   trimap [dev] u8 [B,H,W] (255 foreground, 0 background, any other byte unknown)   alpha [dev] f32 [B,H,W]
 *   H <= H1 <= 32768, W <= W1 <= 32768, H, W >= 1, B <= 65535 (else GGC_E_SHAPE); 0 <= grow <= 64 (else
 *   GGC_E_INVALID_ARG); B == 0 does nothing
 * For output pixel (y, x) the source pixels (y0|y1, x0|x1) and the weights wy, wx are those of ggc_upsample_matte (O2),
 * its float64 half-pixel formula word for word.
 *   trimap_full [dev] u8 [B,H1,W1]  255 if every source pixel of nonzero weight is 255, 0 if every one is 0, else 128
 *               (x1 counts when wx > 0, y1 when wy > 0: a pixel that does not enter the interpolation does not make its
 *               neighbour unknown); the 128 set is then dilated by `grow` full-size pixels (Chebyshev, clipped to the image)
 *   alpha0_full [dev] f32 [B,H1,W1] = (float) lerp(lerp(a00, a01, wx), lerp(a10, a11, wx), wy), a = clamp((double)alpha,
 *               0, 1) with a NaN read as 0, lerp(u, v, t) = u + t (v - u) in float64, no contraction
 *   (either output may be NULL, not both; trimap is not read without trimap_full, alpha not without alpha0_full)
 * With H1 = H, W1 = W and grow = 0 every weight is 0: trimap_full is the trimap with every unknown byte written as 128,
 * alpha0_full the clamped alpha bit for bit.  A known pixel of trimap_full has a known nearest source pixel of the same
 * value.  No atomics; every image is independent of its batch.  Scratch: 2 bytes per full-size pixel from the context
 * when grow > 0 and trimap_full is given, else none.  Does not synchronise. */
int ggc_lift_trimap(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* trimap, const float* alpha,
                    int H1, int W1, int grow, uint8_t* trimap_full, float* alpha0_full);

/* O3b — the unknown band of O3 as a trimap (additive): what ggc_closed_form_matte(binary, band) solved on, written by the
 * kernels of its own front end, so that a later entry (O3l) starts from the solver's band and not from a restatement.
 *   binary [dev] u8 [B,H,W] (any nonzero byte is 1)   0 <= band <= 64 (else GGC_E_INVALID_ARG); H, W >= 1, H, W <= 32768,
 *   B <= 65535 (else GGC_E_SHAPE); B == 0 does nothing
 *   trimap [dev] u8 [B,H,W] = 128 on O3's U, else 255 (binary != 0) (NULL is GGC_E_INVALID_ARG)
 * ggc_trimap_matte with this trimap and alpha0 = (binary != 0) equals ggc_closed_form_matte bit for bit (O3t).  No atomics.
 * Scratch: 2 bytes per pixel from the context.  Does not synchronise. */
int ggc_closed_form_band(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* binary, int band,
                         uint8_t* trimap);

/* O3f — a working-size binary mask carried to a larger size as the start of a banded graph cut there (additive; Lombaert,
 * Sun, Grady and Xu, ICCV 2005): the lifted mask, and GrabCut labels that fix every pixel but a band around its edge.
 *   binary [dev] u8 [B,H,W] (any nonzero byte is 1)
 *   H <= H1 <= 32768, W <= W1 <= 32768, H, W >= 1, B <= 65535 (else GGC_E_SHAPE); 0 <= band <= 64 (else
 *   GGC_E_INVALID_ARG); B == 0 does nothing
 * For output pixel (y, x) the source pixels (y0|y1, x0|x1) and the weights wy, wx are those of ggc_upsample_matte (O2),
 * its float64 half-pixel formula word for word.  With m = (binary != 0) as 0.0 / 1.0:
 *   v         = lerp(lerp(m00, m01, wx), lerp(m10, m11, wx), wy), lerp(u, v, t) = u + t (v - u) in float64, no contraction
 *   M1        = (v >= 0.5), the lifted mask
 *   E         the pixels whose 3x3 neighbourhood of M1 (clipped to the image) holds both values
 *   U         the pixels within Chebyshev distance `band` of a pixel of E (clipped): O3's rule, so that
 *             ggc_closed_form_band(M1, band) writes 128 exactly on U
 *   labels_full [dev] u8 [B,H1,W1]  3 (PR_FGD) on U and M1, 2 (PR_BGD) on U and not M1, 1 (FGD) on M1 off U, else 0 (BGD)
 *   mask_full   [dev] u8 [B,H1,W1]  = M1                                  (either may be NULL, not both)
 * With H1 = H, W1 = W every weight is 0 and M1 = m.  An image whose M1 is empty or full has no E and no band: its labels
 * are all 0 or all 1.  No atomics; every image is independent of its batch.  Scratch: one bit per full-size pixel (rows
 * padded to 64 pixels) for M1 and, with labels_full, one more for the dilation, from the context: 1/4 byte per pixel.
 * Does not synchronise. */
int ggc_lift_labels(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* binary,
                    int H1, int W1, int band, uint8_t* labels_full, uint8_t* mask_full);

/* O4 — foreground colour estimation under a given alpha matte (additive; the multi-level foreground estimation energy of
 * Germer, Uelwer, Conrad and Harmeling, ICPR 2020, restricted to the pixels of fractional alpha with Dirichlet values).
 * A cut-out that keeps the image's bytes carries the old background along wherever alpha is fractional (I = alpha F +
 * (1 - alpha) B); this entry estimates F there.  Per image and independently per colour channel, I = byte / 255, alpha
 * read as float64:
 *   snap      alpha' = 0 where alpha < 1/510, 1 where alpha > 1 - 1/510, else alpha (the pixels whose alpha byte is 0 or
 *             255).  A NaN is not >= 1/510 and is snapped to 0; -inf and +inf snap to 0 and 1.  Z = {alpha' = 0},
 *             O = {alpha' = 1}, unknown set U = {0 < alpha' < 1}; no dilation
 *   known     F = I on O, B = I on Z; F on Z and B on O are not part of the system
 *   energy    E = sum_{i in U} (alpha'_i F_i + (1 - alpha'_i) B_i - I_i)^2
 *               + delta sum_{i in U} [(F_i - I_i)^2 + (B_i - I_i)^2],                          delta = 1e-6, fixed
 *               + sum_{(i,j)} w_ij [phiF_ij (F_i - F_j)^2 + phiB_ij (B_i - B_j)^2],  w_ij = eps_r + omega |alpha'_i - alpha'_j|
 *             over the horizontal and vertical neighbour pairs inside the image with at least one end in U; phiF_ij = 1
 *             when both ends are in U or O (an end in O contributes its known F = I), else 0; phiB_ij = 1 when both ends
 *             are in U or Z, else 0.  No links across the image border.
 *   solve     the normal equations A x = b (symmetric positive definite for eps_r >= 0) by preconditioned CG from
 *             F = B = I; preconditioner: the exact 2 x 2 diagonal block of each pixel, [[alpha'^2 + delta + sum w phiF,
 *             alpha' (1 - alpha')], [alpha' (1 - alpha'), (1 - alpha')^2 + delta + sum w phiB]]; one CG over the three
 *             channels of an image.  An image stops when ||r_j||_2 <= max(tol ||r_0||_2, 1e-12 sqrt(6 |U|))
 *             (unpreconditioned residual) or after max_iter iterations; the test is made on r_0 too, so an image whose U
 *             is empty, or whose start already solves the system (a flat-colour image), takes 0 iterations.
 *   bgr [dev] u8 [B,H,W,3]   alpha [dev] f32 [B,H,W]
 *   0 <= eps_r <= 1, 0 <= omega <= 1000, eps_r + omega > 0, 1 <= max_iter <= 100000, 1e-12 <= tol < 1 (else
 *   GGC_E_INVALID_ARG); H, W <= 32768, B <= 65535 (else GGC_E_SHAPE); B == 0 does nothing
 *   foreground [dev] u8 [B,H,W,3] = floor(255 clamp(F, 0, 1) + 0.5) on U, the image's bytes everywhere else
 *   rgba [dev] u8 [B,H,W,4] = that colour, floor(255 clamp(alpha, 0, 1) + 0.5) of the UNSNAPPED alpha (0 for a NaN)
 *   raw_f, raw_b [dev] f64 [B,H,W,3] = F, B unclamped (I outside U)
 *   iters [dev] i32 [B]     rel_residual [dev] f64 [B] = ||r_j|| / ||r_0|| (0 for an image with 0 iterations)
 *   (each may be NULL, not all of them)
 * The CG vectors and dot products are float64.  Every per-image reduction runs in one fixed order over that image's
 * tiles, so every image's outputs equal its single-image call bit for bit and two runs are identical; no float atomics.
 * Work is restricted to the 16 x 16 tiles that hold U, listed once per call.  The entry SYNCHRONISES its stream: once to
 * build that list on the host, and every 8 iterations to read the count of finished images (an integer atomic) and stop
 * when all are done.  Scratch from the context: 4 bytes per pixel, 32 bytes per 16 x 16 tile and 72 bytes per image over
 * the whole batch, plus 61440 bytes (256 pixels x 5 vectors x 48 bytes) per LISTED tile. */
int ggc_estimate_foreground(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const float* alpha,
                            float eps_r, float omega, int max_iter, float tol,
                            uint8_t* foreground, uint8_t* rgba, double* raw_f, double* raw_b, int32_t* iters,
                            double* rel_residual);

/* O5 — a cut-out placed on a new background (additive): alpha-over of a BGRA cut-out at an offset.  All arithmetic is
 * integer.
 *   rgba       [dev] u8  [B,Hs,Ws,4]  BGRA, as rgba / rgba_soft / rgba_clean
 *   background [dev] u8  [B,H,W,3]
 *   offsets    [dev] i32 [B,2]        row, col of the source's pixel (0,0) in the background; may be negative, and any
 *                                     value is taken (a source that lies wholly outside changes nothing)
 *   out        [dev] u8  [B,H,W,3]    for a pixel p whose source pixel p - offset exists, with a = that pixel's alpha byte
 *                                     and c its colour: (a c + (255 - a) bg + 127) / 255 per channel, integer division;
 *                                     bg everywhere else.  out may be background itself (in place)
 *   H, W, Hs, Ws in 1..32768, B <= 65535 (else GGC_E_SHAPE); B == 0 does nothing.
 * Does not synchronise; no scratch; every image is independent of its batch. */
int ggc_composite_over(ggc_ctx* ctx, ggc_stream stream, int B, int Hs, int Ws, const uint8_t* rgba, int H, int W,
                       const uint8_t* background, const int32_t* offsets, uint8_t* out);

/* O6 — gradient-domain ("seamless", Poisson) cloning of a selected source region into a target (additive; Perez, Gangnet
 * and Blake, SIGGRAPH 2003, with source or mixed gradients).  Per image and independently per colour channel, in byte
 * units, g the source and t the target:
 *   Omega     the target pixels p inside the target whose source pixel p - offset exists and is selected (mask != 0)
 *   N_p       the 4-neighbours of p that lie inside the target: no links across the target's border, so a pixel on it
 *             has degree |N_p| = 2 or 3
 *   system    for p in Omega:  |N_p| f_p - sum_{q in N_p and Omega} f_q = sum_{q in N_p \ Omega} t_q + sum_{q in N_p} v_pq
 *   guidance  d_s = g_p - g_q when q's source pixel exists, else 0;  d_t = t_p - t_q
 *             mixed = 0: v_pq = d_s;  mixed = 1: v_pq = d_t where |d_t| > |d_s|, else d_s (a tie goes to d_s), per
 *             channel.  The right-hand side is an exact integer.
 *   solve     preconditioned CG in float64, one CG over the three channels of an image; Jacobi preconditioner |N_p|;
 *             start f = g, the plain paste.  An image stops when ||r_j||_2 <= max(tol ||r_0||_2, 2.55e-10 sqrt(3 |Omega|))
 *             (unpreconditioned residual) or after max_iter iterations; the test is made on r_0 too, so an image cloned
 *             onto itself takes 0 iterations: its r_0 is exactly 0 and its composite is the target bit for bit.
 *   unsolved  an image whose Omega is empty is not solved: its composite is the target.  An image with |Omega| = H W is
 *             not solved either (nothing anchors it): its composite is the pasted source.  Both report 0 iterations and
 *             rel_residual 0.
 *   source [dev] u8 [B,Hs,Ws,3]   mask [dev] u8 [B,Hs,Ws]   target [dev] u8 [B,H,W,3]   offsets [dev] i32 [B,2] = row, col
 *   of the source's pixel (0,0) in the target, each within +-32768 (else GGC_E_INVALID_ARG, found after the front pass)
 *   mixed 0 | 1, 1 <= max_iter <= 100000, 1e-12 <= tol < 1 (else GGC_E_INVALID_ARG); H, W, Hs, Ws in 1..32768,
 *   B <= 65535 (else GGC_E_SHAPE); B == 0 does nothing
 *   composite [dev] u8 [B,H,W,3]  = floor(clamp(f, 0, 255) + 0.5) on Omega, the target's bytes elsewhere
 *   raw       [dev] f64 [B,H,W,3] = f unclamped on Omega, t elsewhere
 *   n_omega   [dev] i32 [B]       = |Omega|
 *   iters [dev] i32 [B]     rel_residual [dev] f64 [B] = ||r_j|| / ||r_0|| (0 for an image with 0 iterations)
 *   (each may be NULL, not all of them)
 * The CG vectors and dot products are float64.  Every per-image reduction runs in one fixed order over that image's
 * tiles, so every image's outputs equal its single-image call bit for bit and two runs are identical; no float atomics.
 * Work is restricted to the 16 x 16 tiles that hold Omega, listed once per call.  The entry SYNCHRONISES its stream: once
 * to build that list on the host, and every 8 iterations to read the count of finished images (an integer atomic) and
 * stop when all are done.  Scratch from the context: 1 byte per target pixel, 32 bytes per 16 x 16 tile and 64 bytes per
 * image over the whole batch, plus 30720 bytes (256 pixels x 5 vectors x 24 bytes) per LISTED tile. */
int ggc_poisson_clone(ggc_ctx* ctx, ggc_stream stream, int B, int Hs, int Ws, const uint8_t* source, const uint8_t* mask,
                      int H, int W, const uint8_t* target, const int32_t* offsets, int mixed, int max_iter, float tol,
                      uint8_t* composite, double* raw, int32_t* n_omega, int32_t* iters, double* rel_residual);

/* R0 — IoU = tp / (tp + fp + fn + 1e-8) per image (metrics.py:79-84).
 *   iou [dev] f64 [B] (may be NULL)   counts [dev] u64 [B,3] = tp, fp, fn (may be NULL) */
int ggc_mask_iou(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                 const uint8_t* pred, const uint8_t* gt, double* iou, uint64_t* counts);

/* C7 — 8-bit colour spaces for GrabCutConfig.color_space (reference grabcut.py:73-79: cv2.cvtColor(BGR2HSV / BGR2Lab)
 * on uint8 images).  mode 0 = HSV (H in [0,180), OpenCV's fixed-point scheme), mode 1 = Lab
 * (L*255/100, a+128, b+128 of the float64 CIELAB, rounded).  OpenCV is absent here: parity with it is unpinned.
 *   bgr, out [dev] u8 [n_pixels,3] */
int ggc_convert_color8(ggc_ctx* ctx, ggc_stream stream, int64_t n_pixels, const uint8_t* bgr, int mode, uint8_t* out);

/* R1 — integer tallies behind metrics.evaluate / boundary_f1 / evaluate_trimap (metrics.py:58-129, 152-201), per
 * image.  counts [dev] u64 [B,14]:
 *   0 tp 1 fp 2 fn (pred / gt != 0)
 *   3 |pred boundary| 4 |gt boundary| 5 |both|: boundary = m - erode(m, ones(2*width+1)^2) with cv2.erode's default
 *     border (pixels outside the image never erode); zeros when boundary_width <= 0
 *   6 fg_tp 7 fg_fp 8 fg_fn 9 bg_tp 10 bg_fp 11 bg_fn 12 probable pixels 13 pixels where (FG|PR_FG) == gt value;
 *     zeros when trimap == NULL (trimap values as ggc_grabcut's mask). */
int ggc_eval_counts(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                    const uint8_t* pred, const uint8_t* gt, const uint8_t* trimap, int boundary_width,
                    uint64_t* counts);

/* R2 — the four errors of an alpha matte against the true matte (additive; Rhemann, Rother, Wang, Gelautz, Kohli and
 * Rott, CVPR 2009, as the matting benchmarks report them), per image.  Both mattes are 8-bit levels, alpha = level / 255.
 *   pred, gt [dev] u8 [B,H,W]: a (the matte under test) and g (the true matte)
 *   region   [dev] u8 [B,H,W] or NULL: nonzero = counted (NULL: every pixel).  It restricts the SUMS only; the filter and
 *            the components always see the whole image.  With R the counted pixels:
 *   n     = |R|
 *   SAD   = sum_R |a - g|                                             (integer, unit 1/255)
 *   SSE   = sum_R (a - g)^2                                           (integer, unit 1/255^2)
 *   CONN  for k = 1..10, S_k = {10 a >= 255 k} & {10 g >= 255 k} (integer compares: level >= k/10) and Omega_k the largest
 *         4-CONNECTED component of S_k, among components of equal largest area the one that holds the smallest raster
 *         index y*W + x; Omega_k is empty when S_k is.  lev(p) = (the smallest k >= 1 with p not in Omega_k) - 1, and 10
 *         when there is none (the first failure: the Omega_k need not be nested).  d_a = 10 a - 255 lev,
 *         d_g = 10 g - 255 lev (both >= 0: p is in Omega_lev), D(d) = d if d >= 383 else 0 (d / 2550 >= 0.15).
 *         CONN = sum_R |D(d_a) - D(d_g)|                              (integer, unit 1/2550)
 *   GRAD  sigma = 1.4, taps x = -4..4, G(x) = exp(-x^2 / 2 sigma^2) / (sigma sqrt(2 pi)), G'(x) = -x G(x) / sigma^2,
 *         F_x[i][j] = G(i) G'(j) / N with N = sqrt(sum_ij (G(i) G'(j))^2), F_y its transpose; correlation of alpha in
 *         float64 with the border replicated, m(u) = sqrt((F_x * u)^2 + (F_y * u)^2), GRAD = sum_R (m(a) - m(g))^2.  The
 *         9 + 9 normalised taps are computed once on the host in float64 and passed to the kernel, which applies them
 *         separably (rows, then columns).
 *   sums   [dev] u64 [B,4] = n, SAD, SSE, CONN
 *   grad   [dev] f64 [B] = GRAD, or NULL: the filter is not run
 *   levels [dev] u8  [B,H,W] = lev, 0..10, or NULL
 * Conventional reporting (the host's business): sad = SAD / 255 / 1000, mse = SSE / 255^2 / n, grad = GRAD / 1000,
 * conn = CONN / 2550 / 1000.
 * B == 0 does nothing; B > 65535, H or W outside 1..32768 or H*W >= 2^31: GGC_E_SHAPE; pred, gt or sums NULL:
 * GGC_E_INVALID_ARG.  The integer sums use integer atomics, one set per block; GRAD uses none: fixed tiles, a fixed tree
 * per tile, the tiles of an image added in a fixed order.  Every image's five outputs and its levels equal its
 * single-image call bit for bit, and two runs are identical.  Scratch from the context: 8 L + 1 bytes per pixel (8 L when
 * `levels` is given), 80 bytes per image and, with `grad`, 8 bytes per 16 x 16 tile; L, the levels labelled per pass, is 10
 * (81 bytes per pixel) while 80 bytes x B x H x W is at most 4 GiB, else 1 (9 bytes per pixel), unless GGC_MATTE_EVAL_LEVELS
 * fixes it; the results do not depend on it.  Does not synchronise and reads nothing back on the host. */
int ggc_matte_errors(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                     const uint8_t* pred, const uint8_t* gt, const uint8_t* region,
                     uint64_t* sums, double* grad, uint8_t* levels);

/* D0 — per-region ground-truth coverage for the graph-cache writer: the integer sums behind
 * derive_trimap_labels and prepare_sample's fg_ratio (dataset.py:194-206, 245-248):
 *   counts[n] = pixels of region n,  fg[n] = pixels of region n with gt_mask > 0.
 *   segments [dev] i32 [B,H,W] (local labels)   gt_mask [dev] u8 [B,H,W]   node_ptr [dev] i32 [B+1]
 *   counts, fg [dev] i32 [node_ptr[B]]   (labels outside an image's node range are ignored) */
int ggc_region_label_stats(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W,
                           const int32_t* segments, const uint8_t* gt_mask, const int32_t* node_ptr,
                           int32_t* counts, int32_t* fg);

#ifdef __cplusplus
}
#endif
#endif /* GGC_H */
