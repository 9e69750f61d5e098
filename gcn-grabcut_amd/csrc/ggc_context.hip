// ggc_context.hip — context, error reporting, scratch arena.
#include "ggc_internal.h"
#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <mutex>

static thread_local std::string g_create_err;   // ggc_last_error(NULL) reports the calling thread's failed ggc_ctx_create

namespace ggc {

const Knobs& knobs() {
    static const Knobs k = [] {
        auto num = [](const char* name, int dflt, int lo) { const char* e = std::getenv(name); return e ? std::max(lo, std::atoi(e)) : dflt; };
        Knobs k;
        k.mf_trace = std::getenv("GGC_MF_TRACE") != nullptr;
        k.mf_warm = num("GGC_MF_WARM", 1, 0);
        k.mf_async_push_active = num("GGC_MF_ASYNC_PUSH_ACTIVE", 10000, 0);
        k.mf_async_tile = num("GGC_MF_ASYNC_TILE", 8, 8);
        k.mf_async_hops = num("GGC_MF_ASYNC_HOPS", 24, 1);
        k.mf_async_sweeps = num("GGC_MF_ASYNC_SWEEPS", 12, 1);
        k.mf_dense_launches = num("GGC_MF_DENSE_LAUNCHES", 12, 1);
        k.mf_dense_launches0 = num("GGC_MF_DENSE_LAUNCHES0", 8, 1);
        k.mf_dense_sweeps = num("GGC_MF_DENSE_SWEEPS", 12, 1);
        k.mf_relax_dense = num("GGC_MF_RELAX_DENSE", 3, 1);
        // a partial round never closes an image, so a value near the driver's round cap (4096) would fail every solve
        k.mf_partial_rounds = std::min(64, num("GGC_MF_PARTIAL_ROUNDS", 3, 0));
        k.mf_label_slack = std::min(1 << 20, num("GGC_MF_LABEL_SLACK", 0, -1));   // (the ceiling is formed as label + 1 + slack in int32)
        k.agg_direct = num("GGC_AGG_DIRECT", 0, 0);
        k.slic_seq_connectivity = num("GGC_SLIC_SEQ_CONNECTIVITY", 0, 0);
        k.slic_cn_tiles = num("GGC_SLIC_CN_TILES", 1, 0);
        k.matte_eval_levels = num("GGC_MATTE_EVAL_LEVELS", 0, 0);
        if (k.matte_eval_levels > 10 || (k.matte_eval_levels && 10 % k.matte_eval_levels != 0)) k.matte_eval_levels = 0;   // the passes must tile the ten levels
        k.graph_onchip = num("GGC_GRAPH_ONCHIP", 1, 0);
        k.graph_bands = num("GGC_GRAPH_BANDS", 0, 0);
        if (k.graph_bands > 8) k.graph_bands = 0;
        k.wand_seeds_per_pass = num("GGC_WAND_SEEDS_PER_PASS", 0, 0);
        if (k.wand_seeds_per_pass > 4096) k.wand_seeds_per_pass = 0;
        return k;
    }();
    return k;
}

int set_err(ggc_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_err = buf;
    return code;
}

void* scratch(ggc_ctx* ctx, int slot, size_t bytes) {
    Buf& b = ctx->slots[slot];
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return b.p;
    if (b.p) {
        // hipFree synchronises the device, so no kernel still reads the old buffer.
        if (hipFree(b.p) != hipSuccess) { set_err(ctx, GGC_E_DEVICE, "hipFree failed"); return nullptr; }
        b.p = nullptr; b.bytes = 0;
    }
    size_t want = bytes + bytes / 4;           // headroom so ragged batches rarely regrow
    want = (want + 255) & ~size_t(255);
    void* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
        set_err(ctx, GGC_E_OOM, "hipMalloc(%zu) failed for scratch slot %d", want, slot);
        return nullptr;
    }
    b.p = p; b.bytes = want;
    return p;
}

// small synchronous device -> host read through the context's page-locked staging buffer.  (Round 3 measured the
// alternative — a one-thread kernel publishing into host-coherent memory and the host spinning on a ticket instead of
// hipStreamSynchronize: 58.4-58.8 vs 59.1-60.3 ms per GrabCut stage, 86.9 vs 87.1 ms per step: not worth four spinning cores.)
int read_i32(ggc_ctx* ctx, hipStream_t st, const int32_t* dev, int n, std::vector<int32_t>& host) {
    host.resize(n);
    if (ctx->h_pinned && n <= ggc_ctx::H_PINNED_INTS) {
        GGC_HIP(ctx, hipMemcpyAsync(ctx->h_pinned, dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        GGC_HIP(ctx, hipStreamSynchronize(st));
        std::copy(ctx->h_pinned, ctx->h_pinned + n, host.begin());
        return GGC_OK;
    }
    GGC_HIP(ctx, hipMemcpyAsync(host.data(), dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    GGC_HIP(ctx, hipStreamSynchronize(st));
    return GGC_OK;
}

int check_offsets(ggc_ctx* ctx, const int32_t* off, int n, const char* name, const char* unit, int min_step) {
    GGC_REQUIRE(ctx, off[0] == 0, GGC_E_INVALID_ARG, "%s[0] = %d, expected 0", name, off[0]);
    for (int i = 0; i < n; ++i)
        GGC_REQUIRE(ctx, (int64_t)off[i + 1] - off[i] >= min_step, GGC_E_INVALID_ARG,
                    "%s decreases at %s %d, or steps by less than %d (%d -> %d)", name, unit, i, min_step, off[i], off[i + 1]);
    return GGC_OK;
}

int read_offsets(ggc_ctx* ctx, hipStream_t st, const int32_t* dev, int n, const char* name, const char* unit, int min_step,
                 std::vector<int32_t>& host) {
    const int rc = read_i32(ctx, st, dev, n + 1, host);
    return rc ? rc : check_offsets(ctx, host.data(), n, name, unit, min_step);
}

} // namespace ggc

extern "C" {

int ggc_version(void) { return GGC_VERSION; }

int ggc_ctx_create(int device_id, ggc_ctx** out) {
    if (!out) return ggc::set_err(nullptr, GGC_E_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return ggc::set_err(nullptr, GGC_E_DEVICE, "no HIP device available (%s)",
                            e == hipSuccess ? "count=0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return ggc::set_err(nullptr, GGC_E_INVALID_ARG, "device_id %d out of range [0,%d)", device_id, n);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return ggc::set_err(nullptr, GGC_E_DEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ggc::set_err(nullptr, GGC_E_UNSUPPORTED, "device %d is %s; this library is built for gfx950 (MI355X) only",
                            device_id, prop.gcnArchName);
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return ggc::set_err(nullptr, GGC_E_DEVICE, "hipSetDevice: %s", hipGetErrorString(e));
    ggc_ctx* c = new (std::nothrow) ggc_ctx();
    if (!c) return ggc::set_err(nullptr, GGC_E_OOM, "host allocation failed");
    c->device = device_id;
    c->n_cu = prop.multiProcessorCount;
    if (hipHostMalloc(reinterpret_cast<void**>(&c->h_pinned), sizeof(int32_t) * ggc_ctx::H_PINNED_INTS, hipHostMallocDefault) != hipSuccess)
        c->h_pinned = nullptr;              // reads fall back to pageable memory
    *out = c;
    return GGC_OK;
}

int ggc_ctx_destroy(ggc_ctx* ctx) {
    if (!ctx) return GGC_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto& r : ctx->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto& e : ctx->prof_pool) (void)hipEventDestroy(e);
    for (auto& b : ctx->slots) if (b.p) (void)hipFree(b.p);
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    for (ggc::WeightSet* m : {&ctx->resgcn, &ctx->gcnnet, &ctx->gat})
        for (auto& kv : m->dev) if (kv.second.p) (void)hipFree(kv.second.p);
    delete ctx;
    return GGC_OK;
}

int ggc_profile_enable(ggc_ctx* ctx, int on) {
    if (!ctx) return GGC_E_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto& r : ctx->prof) { ctx->prof_pool.push_back(r.a); ctx->prof_pool.push_back(r.b); }
    ctx->prof.clear();
    ctx->prof_on = on == 2 ? 2 : (on != 0 ? 1 : 0);
    if (on) {
        // An event pair around nothing does not report zero: the two markers are separate queue packets.  Calibrate
        // that offset (median of 15 empty pairs on the null stream) so that ggc_profile_query can report kernel time.
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) {
            std::vector<float> v;
            for (int i = 0; i < 15; ++i) {
                float ms = 0.0f;
                if (hipEventRecord(a, nullptr) == hipSuccess && hipEventRecord(b, nullptr) == hipSuccess &&
                    hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess)
                    v.push_back(ms);
            }
            if (!v.empty()) { std::sort(v.begin(), v.end()); ctx->prof_overhead_ms = v[v.size() / 2]; }
        }
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    return GGC_OK;
}

int ggc_profile_query(ggc_ctx* ctx, const char* kernel, int* launches, double* total_ms) {
    if (!ctx || !kernel || !launches || !total_ms) return GGC_E_INVALID_ARG;
    *launches = 0; *total_ms = 0.0;
    if (std::strcmp(kernel, "#event_pair_overhead") == 0) { *launches = 1; *total_ms = ctx->prof_overhead_ms; return GGC_OK; }
    for (auto& r : ctx->prof) {
        if (std::strcmp(r.name, kernel) != 0) continue;
        GGC_HIP(ctx, hipEventSynchronize(r.b));
        float ms = 0.0f;
        GGC_HIP(ctx, hipEventElapsedTime(&ms, r.a, r.b));
        *total_ms += std::max(0.0, (double)ms - ctx->prof_overhead_ms); *launches += 1;
    }
    return GGC_OK;
}

const char* ggc_last_error(const ggc_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_create_err.c_str();
}

} // extern "C"
