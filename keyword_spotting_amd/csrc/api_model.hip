// C ABI of libkws_amd.so (include/kws_amd.h): error state, live handles, the model handle's life (validate, pack, upload).
#include <cstdarg>
#include <mutex>
#include <new>
#include <unordered_map>

#include "api_internal.h"

namespace kws_host {

thread_local std::string g_last_error;

namespace {
std::mutex g_live_mutex;
std::unordered_map<const void*, unsigned long long> g_live;
unsigned long long g_live_serial = 0;
}  // namespace

unsigned long long live_register(const void* h) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    return g_live[h] = ++g_live_serial;
}
void live_unregister(const void* h) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.erase(h);
}
unsigned long long live_serial(const void* h) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    const auto it = g_live.find(h);
    return it == g_live.end() ? 0ull : it->second;
}

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? KWS_ERR_OUT_OF_MEMORY : KWS_ERR_HIP, "%s: %s", what,
                hipGetErrorString(e));
}

}  // namespace kws_host

using namespace kws_host;

static bool config_ok(const kws_config* c, int* code) {
    if (!c) { *code = fail(KWS_ERR_INVALID_ARGUMENT, "config is null"); return false; }
    if (c->n_mel < 1 || c->n_mel > 1024) { *code = fail(KWS_ERR_INVALID_ARGUMENT, "n_mel=%d out of range [1,1024]", c->n_mel); return false; }
    if (c->num_layers < 1 || c->num_layers > 8) { *code = fail(KWS_ERR_INVALID_ARGUMENT, "num_layers=%d out of range [1,8]", c->num_layers); return false; }
    if (c->num_classes < 3 || c->num_classes > kws::kMaxClasses) { *code = fail(KWS_ERR_UNSUPPORTED, "num_classes=%d unsupported (3..8)", c->num_classes); return false; }
    if (c->hidden != 64 && c->hidden != 128 && c->hidden != 256) { *code = fail(KWS_ERR_UNSUPPORTED, "hidden=%d unsupported (64, 128, 256)", c->hidden); return false; }
    if (c->precision == KWS_INT8 && c->hidden != 128) {
        *code = fail(KWS_ERR_UNSUPPORTED, "int8 path needs hidden=128 (OctbitMatMul K=2*hidden must be a multiple of 64 and the kernel is built for 128); got %d", c->hidden);
        return false;
    }
    if (c->precision != KWS_FP32 && c->precision != KWS_BF16 && c->precision != KWS_INT8 && c->precision != KWS_F16X3) { *code = fail(KWS_ERR_INVALID_ARGUMENT, "unknown precision %d", c->precision); return false; }
    if (c->precision == KWS_F16X3 && !kws::gru_f16x3_supported(c->hidden, c->n_mel) && !kws::gru_f16x3_generic_supported(c->hidden, c->n_mel)) {
        *code = fail(KWS_ERR_UNSUPPORTED, "f16x3 path needs hidden=128 (register-resident kernels) or 256 (weights streamed from L2) and n_mel%%4==0, 4..64; "
                     "got hidden=%d n_mel=%d", c->hidden, c->n_mel);
        return false;
    }
    if (c->precision == KWS_BF16 && !kws::gru_bf16_supported(c->hidden, c->n_mel, c->num_layers)) {
        *code = fail(KWS_ERR_UNSUPPORTED, "bf16 path needs hidden=128, num_layers<=2, n_mel%%4==0 and <=64; got hidden=%d layers=%d n_mel=%d",
                     c->hidden, c->num_layers, c->n_mel);
        return false;
    }
    return true;
}

// wrap == null reads as all-zero.  Checked after the config (config_ok).
static bool wrappers_ok(const kws_config* c, const kws_cell_wrappers* w, int* code) {
    if (!w) return true;
    const struct { const char* name; int32_t v; } opt[2] = {{"use_layer_norm", w->use_layer_norm}, {"use_residual", w->use_residual}};
    for (const auto& o : opt)
        if (o.v != 0 && o.v != 1) { *code = fail(KWS_ERR_INVALID_ARGUMENT, "cell wrapper %s=%d: must be 0 or 1", o.name, o.v); return false; }
    static const char* const prec_name[] = {"fp32", "bf16", "int8", "f16x3"};
    for (const auto& o : opt)
        if (o.v && c->precision != KWS_FP32) {
            *code = fail(KWS_ERR_UNSUPPORTED, "cell wrapper %s needs precision fp32 (the wrapped kernels are the fp32 generic ones); got %s",
                         o.name, prec_name[c->precision]);
            return false;
        }
    return true;
}
static kws_cell_wrappers wrappers_of(const kws_cell_wrappers* w) { return w ? *w : kws_cell_wrappers{0, 0}; }

// The second class head of kws_create_heads.  Checked after the config (config_ok), before any device work.
static bool heads_ok(const kws_config* c, int32_t num_classes2, int* code) {
    if (num_classes2 < 3 || num_classes2 > kws::kMaxClasses) {
        *code = fail(KWS_ERR_UNSUPPORTED, "num_classes2=%d unsupported (3..8)", num_classes2);
        return false;
    }
    const char* why = nullptr;
    switch (c->precision) {
        case KWS_BF16: why = "bf16: the fused bf16 stack has no seam between its layers for the heads to read"; break;
        case KWS_INT8: why = "int8: its class projection is the quantised OctbitMatMul behind the stack"; break;
        case KWS_F16X3: why = "f16x3: its seams hold fp16 pairs, not fp32 rows"; break;
        default: break;
    }
    if (why) { *code = fail(KWS_ERR_UNSUPPORTED, "a second class head needs precision fp32 (%s)", why); return false; }
    return true;
}
static size_t heads_floats(const kws_config* c, int32_t num_classes2) { return (size_t)c->hidden * num_classes2 + num_classes2; }

// kws_create_wrapped / kws_create_heads behind their argument checks: `need` bytes of blob, num_classes2 > 0: with the second head
static int create_model(const kws_config* cfg, const kws_cell_wrappers& wr, int num_classes2, const void* weights_blob, size_t nbytes,
                        size_t need, kws_handle* out);

extern "C" {

// Compiler provenance is part of the version string: the fp32 resident kernels rely on hand-placed hazard fences around
// inline-asm MFMAs and gru_bf16.hip on an internal LLVM option (csrc/Makefile), so "which hipcc built this" is the first
// thing to know when kws_selftest fails on a deployment.
const char* kws_version(void) {
    static const std::string v = [] {
        char buf[384];
        snprintf(buf, sizeof(buf), "kws_amd 0.6 (gfx950; HIP %d.%d.%d; %s; bf16 mfma-vgpr-form=%d; f16x3 mfma-vgpr-form=%d" KWS_VARIANT_TAG ")", HIP_VERSION_MAJOR,
                 HIP_VERSION_MINOR, HIP_VERSION_PATCH, __VERSION__, kws::gru_bf16_vgpr_form() ? 1 : 0, kws::gru_f16x3_vgpr_form() ? 1 : 0);
        return std::string(buf);
    }();
    return v.c_str();
}
const char* kws_last_error(void) { return g_last_error.c_str(); }
size_t kws_sizeof_config(void) { return sizeof(kws_config); }
size_t kws_sizeof_frontend_config(void) { return sizeof(kws_frontend_config); }

size_t kws_sizeof_cell_wrappers(void) { return sizeof(kws_cell_wrappers); }

size_t kws_weights_nbytes(const kws_config* cfg) { return kws_weights_nbytes_wrapped(cfg, nullptr); }

size_t kws_weights_nbytes_wrapped(const kws_config* cfg, const kws_cell_wrappers* wrap) {
    int code;
    if (!config_ok(cfg, &code) || !wrappers_ok(cfg, wrap, &code)) return 0;
    return wrap_layout(*cfg, wrappers_of(wrap)).total * sizeof(float);
}

int kws_create_wrapped(const kws_config* cfg, const kws_cell_wrappers* wrap, const void* weights_blob, size_t nbytes, kws_handle* out) {
    int code;
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!config_ok(cfg, &code) || !wrappers_ok(cfg, wrap, &code)) return code;
    const kws_cell_wrappers wr = wrappers_of(wrap);
    return create_model(cfg, wr, 0, weights_blob, nbytes, wrap_layout(*cfg, wr).total * sizeof(float), out);
}

size_t kws_sizeof_head_io(void) { return sizeof(kws_head_io); }

size_t kws_weights_nbytes_heads(const kws_config* cfg, int32_t num_classes2) {
    int code;
    if (!config_ok(cfg, &code) || !heads_ok(cfg, num_classes2, &code)) return 0;
    return (blob_layout(*cfg).total + heads_floats(cfg, num_classes2)) * sizeof(float);
}

int kws_create_heads(const kws_config* cfg, int32_t num_classes2, const void* weights_blob, size_t nbytes, kws_handle* out) {
    int code;
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!config_ok(cfg, &code) || !heads_ok(cfg, num_classes2, &code)) return code;
    return create_model(cfg, kws_cell_wrappers{0, 0}, num_classes2, weights_blob, nbytes,
                        (blob_layout(*cfg).total + heads_floats(cfg, num_classes2)) * sizeof(float), out);
}

}  // extern "C"

static int create_model(const kws_config* cfg, const kws_cell_wrappers& wr, int num_classes2, const void* weights_blob, size_t nbytes,
                        size_t need, kws_handle* out) {
    if (!weights_blob) return fail(KWS_ERR_INVALID_ARGUMENT, "weights_blob is null");
    if (nbytes != need)
        return fail(KWS_ERR_INVALID_ARGUMENT, "weights_blob has %zu bytes, config needs %zu", nbytes, need);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");

    kws_model* m = new (std::nothrow) kws_model();
    if (!m) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    m->cfg = *cfg;
    m->wrap = wr;
    m->wrapped = wr.use_layer_norm || wr.use_residual;
    m->num_classes2 = num_classes2;
    {
        const hipError_t e = hipGetDevice(&m->device);
        if (e != hipSuccess) { delete m; return hip_fail(e, "hipGetDevice"); }
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, m->device) == hipSuccess) m->num_cus = prop.multiProcessorCount;
    }
    std::vector<float> host;
    {
        const int rc = pack_weights(*cfg, wr, static_cast<const float*>(weights_blob), &m->pk, &host, num_classes2);
        if (rc != KWS_OK) { delete m; return rc; }
    }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->d_weights), host.size() * sizeof(float));
    if (e != hipSuccess) { delete m; return hip_fail(e, "hipMalloc(weights)"); }
    e = hipMemcpy(m->d_weights, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(m->d_weights); delete m; return hip_fail(e, "hipMemcpy(weights)"); }
    // A pageable-host hipMemcpy may return once the data is staged; make sure the DMA has landed before
    // any stream can launch a kernel that reads the fragments (observed: the tail of the upload missing
    // in the first launch after create).
    e = hipDeviceSynchronize();
    if (e != hipSuccess) { hipFree(m->d_weights); delete m; return hip_fail(e, "hipDeviceSynchronize(weights)"); }
    e = hipEventCreateWithFlags(&m->last_done, hipEventDisableTiming);
    if (e != hipSuccess) { hipFree(m->d_weights); delete m; return hip_fail(e, "hipEventCreate"); }
    m->ms_sum.assign(cfg->num_layers, 0.f);
    m->launches.assign(cfg->num_layers, 0);
    live_register(m);
    // KWS_SELFTEST=1: every kws_create first proves the kernels this handle will use against the library's own known
    // answers (kws_selftest, selftest.hip) -- a few milliseconds; meant for deployments on a ROCm other than the validated one
    static const bool selftest_env = [] { const char* e = getenv("KWS_SELFTEST"); return e && e[0] == '1'; }();
    if (selftest_env && !in_selftest()) {
        const int rc = kws_selftest(m);
        if (rc != KWS_OK) {
            const std::string keep = g_last_error;
            kws_destroy(m);
            g_last_error = keep;
            return rc;
        }
    }
    *out = m;
    return KWS_OK;
}

extern "C" {

int kws_create(const kws_config* cfg, const void* weights_blob, size_t nbytes, kws_handle* out) {
    return kws_create_wrapped(cfg, nullptr, weights_blob, nbytes, out);
}

int kws_destroy(kws_handle h) {
    if (!h) return KWS_OK;
    live_unregister(h);
    hipDeviceSynchronize();
    for (auto& pd : h->pending) { hipEventDestroy(pd.a); hipEventDestroy(pd.b); }
    for (auto ev : h->event_pool) hipEventDestroy(ev);
    for (void* p : {(void*)h->d_weights, (void*)h->arena.base, (void*)h->arena_fine.base, (void*)h->stage.base}) if (p) hipFree(p);
    if (h->last_done) hipEventDestroy(h->last_done);
    if (h->pipe_ready) hipFree(h->pipe_ready);
    // a layer-pipelined step that timed out and was never followed by another call is still reported, once
    const bool pipe_failed = h->pipe_error_host && *reinterpret_cast<volatile int*>(h->pipe_error_host) != 0;
    if (h->pipe_error_host) hipHostFree(h->pipe_error_host);
    for (auto ev : h->ovl_events) hipEventDestroy(ev);
    for (auto ev : h->ovl_tail) if (ev) hipEventDestroy(ev);
    for (auto sx : h->lane_stream) if (sx) hipStreamDestroy(sx);
    for (void* p : {(void*)h->oct_aq, (void*)h->oct_range, (void*)h->oct_prev, (void*)h->heads_prev}) if (p) hipFree(p);
    delete h;
    // The handle is gone whatever happened before: always KWS_OK (a caller that read a failure as "still alive" would free it
    // twice).  A pipelined step that timed out and was never followed by another call is left in kws_last_error().
    if (pipe_failed)
        fail(KWS_OK, "kws_destroy: the last layer-pipelined step of this handle had timed out waiting for the layer below; its results "
                     "were invalid (kws_poll_error before kws_destroy reports this as a status)");
    return KWS_OK;
}

int kws_set_kernel(kws_handle h, int kind) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (kind != KWS_KERNEL_AUTO && kind != KWS_KERNEL_GENERIC && kind != KWS_KERNEL_RESIDENT)
        return fail(KWS_ERR_INVALID_ARGUMENT, "unknown kernel kind %d", kind);
    if (kind == KWS_KERNEL_RESIDENT && h->wrapped)
        return fail(KWS_ERR_UNSUPPORTED, "resident kernels have no cell wrappers (use_layer_norm=%d use_residual=%d): a wrapped handle runs "
                    "the generic kernels", h->wrap.use_layer_norm, h->wrap.use_residual);
    if (kind == KWS_KERNEL_RESIDENT)
        for (const auto& L : h->pk.layers)
            if (!L.resident_ok)
                return fail(KWS_ERR_UNSUPPORTED, "resident kernels need hidden=128 and n_mel in {32, 40, 48, 60, 64}; got hidden=%d n_mel=%d",
                            h->cfg.hidden, h->cfg.n_mel);
    h->kernel_kind = kind;
    return KWS_OK;
}

int kws_last_launch(kws_handle h, int slot, char* buf, size_t n) {
    if (!h || !buf || n == 0) return fail(KWS_ERR_INVALID_ARGUMENT, "null handle / buffer");
    if (slot < 0 || slot >= h->cfg.num_layers) return fail(KWS_ERR_INVALID_ARGUMENT, "slot %d out of range [0,%d)", slot, h->cfg.num_layers);
    snprintf(buf, n, "%s", h->launch_name(slot).c_str());
    return KWS_OK;
}

}  // extern "C"
