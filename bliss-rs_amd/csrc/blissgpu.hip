// blissgpu.hip -- host side of the C ABI declared in include/blissgpu.h: context life cycle, constant tables,
// feature-vector distances, playlist ordering, device-memory helpers, profiling and debug taps.  The analysis
// batches (planning, chunk schedule, PCM feed, coalescing front) live in scheduler.hip, the multi-GPU node in node.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "launch_forms.hpp"
#include "metric_learn.hpp"
#include "covariance_metric.hpp"
#include "mst_merge.hpp"
#include "ward_merge.hpp"
#include "loudness_gate.hpp"
#include "forest.hpp"

using namespace bg;

namespace {
thread_local std::string g_last_error;

const char* const kKernelNames[K_COUNT] = {
#define X(id, name) name,
    BLISSGPU_KERNEL_TABLE(X)
#undef X
};
}  // namespace

namespace bg {
int fail(int code, const char* what, const char* detail) {
    g_last_error = std::string(what) + ": " + (detail ? detail : "");
    return code;
}
}  // namespace bg

namespace {

template <typename T>
int upload(T** dst, const std::vector<T>& h) {
    HIP_TRY(hipMalloc((void**)dst, h.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return BLISSGPU_OK;
}

int build_tables(blissgpu_ctx* c) {
    const float PI_F = 3.14159265358979323846f;
    std::vector<float2> tw8(8192), tw5(512);
    for (int k = 0; k < 8192; k++) {
        const double a = -2.0 * M_PI * (double)k / 8192.0;
        tw8[k] = make_float2((float)cos(a), (float)sin(a));
    }
    for (int k = 0; k < 512; k++) {
        const double a = -2.0 * M_PI * (double)k / 512.0;
        tw5[k] = make_float2((float)cos(a), (float)sin(a));
    }
    // periodic Hann, evaluated in f32 exactly as src/utils.rs:37-39
    std::vector<float> hann(8192), hannz(512), rwv(BT_LAGLEN), dfwv(BT_WINLEN);
    // Both device tables hold HALF the window: the real-input split needs X = (A + P) / 2, and a power-of-two scale
    // commutes with every rounding of the (linear) transform, so halving the window once removes a multiply per bin
    // and leaves every magnitude bit-identical.
    for (int n = 0; n < 8192; n++) hann[n] = 0.5f * (0.5f - 0.5f * cosf(2.0f * (float)n * PI_F / 8192.0f));
    // hanningz, src/aubio.rs:151-154
    for (int i = 0; i < 512; i++) hannz[i] = 0.5f * (0.5f * (1.0f - cosf(2.0f * PI_F * (float)i / 512.0f)));
    // BeatTracking::new, src/aubio.rs:911-936
    const float rayparam = 60.0f * (float)SAMPLE_RATE / 120.0f / (float)HOP_B;
    const float dfwvnorm = expf((logf(2.0f) / rayparam) * (float)(BT_WINLEN + 2));
    for (int i = 0; i < BT_LAGLEN; i++) {
        const float i_f = (float)(i + 1);
        rwv[i] = (i_f / (rayparam * rayparam)) * expf(-(i_f * i_f) / (2.0f * (rayparam * rayparam)));
    }
    for (int i = 0; i < BT_WINLEN; i++) dfwv[i] = expf((logf(2.0f) / rayparam) * (float)(i + 1)) / dfwvnorm;
    int rc;
    if ((rc = upload(&c->tw8192, tw8))) return rc;
    if ((rc = upload(&c->tw512, tw5))) return rc;
    if ((rc = upload(&c->hann8192, hann))) return rc;
    if ((rc = upload(&c->hannz512, hannz))) return rc;
    if ((rc = upload(&c->bt_rwv, rwv))) return rc;
    if ((rc = upload(&c->bt_dfwv, dfwv))) return rc;
    const size_t bank_elems = (size_t)(N_TUNING + 1) * BANK_ROWS * BANK_PITCH;
    HIP_TRY(hipMalloc((void**)&c->chroma_bank, bank_elems * sizeof(double)));
    launch_chroma_bank(c->chroma_bank, c->own_stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->own_stream));
    c->tables = DeviceTables{c->tw8192, c->tw512, c->hann8192, c->hannz512, c->chroma_bank, c->bt_rwv, c->bt_dfwv};
    return BLISSGPU_OK;
}

// Process-wide default contexts of the entry points that take no context: one per visible HIP device, created on first
// use.  BLISSGPU_DEFAULT_DEVICES="0,2,3" restricts / orders them (like HIP_VISIBLE_DEVICES, but for this library only);
// an ordinal may be named more than once (several contexts sharing a GPU -- how the multi-context front is tested on a
// one-GPU box).
std::mutex g_default_mu;
std::vector<int> g_default_devices;
// A default context is created under ITS OWN mutex (building the 40 MB filter bank takes a while: the seats of an 8-GPU node
// must not queue behind one another, and the counters below must stay readable meanwhile).  A creation that failed is
// remembered and not repeated on every call -- but only a failure that cannot change is remembered for good (no such
// device, another architecture: BLISSGPU_ERR_NO_DEVICE / _INVALID).  Anything else (no memory for the tables while another
// process holds the device, a HIP error) is tried again after a back-off that doubles from 100 ms to 5 s, so a long-running
// host recovers by itself; blissgpu_default_reset() forgets every remembered failure at once.
struct DefaultSeat {
    std::mutex mu;
    blissgpu_ctx* ctx = nullptr;
    int fails = 0;           // consecutive failed creations
    bool permanent = false;  // the last failure cannot change in this process
    std::chrono::steady_clock::time_point retry_at{};
    int rc = BLISSGPU_OK;
    std::string err;
};
std::deque<DefaultSeat> g_default_seats;  // (stable addresses)
std::vector<uint64_t> g_default_batches;
bool g_default_init = false;
std::atomic<int64_t> g_single_song_timeout_ms{600000};

void default_init_locked() {
    if (g_default_init) return;
    g_default_init = true;
    if (const char* e = getenv("BLISSGPU_DEFAULT_DEVICES")) {
        for (const char* p = e; *p;) {
            char* end = nullptr;
            const long v = strtol(p, &end, 10);
            if (end == p) break;
            if (v >= 0 && v < 4096 && g_default_devices.size() < 64) g_default_devices.push_back((int)v);
            p = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') break;
        }
    }
    if (g_default_devices.empty()) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) count = 1;  // no device: ctx_create reports it
        for (int k = 0; k < count && k < 64; k++) g_default_devices.push_back(k);
    }
    g_default_seats.resize(g_default_devices.size());
    g_default_batches.assign(g_default_devices.size(), 0);
}

}  // namespace

namespace bg {
int default_ctx_count() {
    std::lock_guard<std::mutex> lk(g_default_mu);
    default_init_locked();
    return (int)g_default_devices.size();
}
int default_ctx_at(int k, blissgpu_ctx** out) {
    DefaultSeat* seat = nullptr;
    int device = 0;
    {
        std::lock_guard<std::mutex> lk(g_default_mu);
        default_init_locked();
        if (k < 0 || k >= (int)g_default_devices.size()) return fail(BLISSGPU_ERR_INVALID, "default context", "no such default device");
        seat = &g_default_seats[(size_t)k];
        device = g_default_devices[(size_t)k];
    }
    std::lock_guard<std::mutex> lk(seat->mu);
    if (!seat->ctx) {
        const auto now = std::chrono::steady_clock::now();
        if (seat->fails == 0 || (!seat->permanent && now >= seat->retry_at)) {
            seat->rc = blissgpu_ctx_create(device, &seat->ctx);
            if (seat->rc) {
                seat->ctx = nullptr;
                seat->fails++;
                seat->permanent = seat->rc == BLISSGPU_ERR_NO_DEVICE || seat->rc == BLISSGPU_ERR_INVALID;
                seat->retry_at = now + std::chrono::milliseconds(std::min(5000, 100 << std::min(seat->fails - 1, 6)));
                seat->err = std::string("default context ") + std::to_string(k) + " (HIP device " + std::to_string(device) + "): " + blissgpu_last_error();
            } else {
                seat->fails = 0;
                seat->permanent = false;
            }
        }
    }
    if (!seat->ctx) return fail(seat->rc, "default context", seat->err.c_str());
    *out = seat->ctx;
    return BLISSGPU_OK;
}
void default_ctx_forget_failures() {
    std::lock_guard<std::mutex> lk(g_default_mu);
    default_init_locked();
    for (DefaultSeat& seat : g_default_seats) {
        std::lock_guard<std::mutex> sl(seat.mu);
        if (!seat.ctx) { seat.fails = 0; seat.permanent = false; seat.rc = BLISSGPU_OK; }
    }
}
// Live contexts per HIP device in this process.  The single-launch sort and the song_to_song chain spin on grid barriers: their
// workgroups must all be resident at once.  One such kernel asks for at most one 256-thread workgroup per CU, so two contexts'
// worth of them always fit beside each other; with more contexts alive on the device the sort falls back to one launch per
// step, and the chain -- which has no multi-launch form -- runs one at a time per device (persistent_kernel_mutex: launch, wait
// for it, release), so that two spinning grids can never hold each other's missing workgroups out of the CUs.
namespace {
std::mutex g_live_mu;
std::vector<int> g_live_contexts;
std::mutex g_persistent_mu[64];
}
std::mutex& persistent_kernel_mutex(int device) { return g_persistent_mu[(unsigned)device % 64u]; }
void live_context_add(int device, int delta) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    if (device < 0) return;
    if ((size_t)device >= g_live_contexts.size()) g_live_contexts.resize((size_t)device + 1, 0);
    g_live_contexts[(size_t)device] += delta;
}
int live_contexts(int device) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    return device >= 0 && (size_t)device < g_live_contexts.size() ? g_live_contexts[(size_t)device] : 0;
}
int64_t single_song_timeout_ms() { return g_single_song_timeout_ms.load(); }
int default_ctx(blissgpu_ctx** out) { return default_ctx_at(0, out); }
void default_ctx_count_batch(int k) {
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (k >= 0 && k < (int)g_default_batches.size()) g_default_batches[k]++;
}
}  // namespace bg

extern "C" {
int blissgpu_default_device_count(void) { return default_ctx_count(); }
int blissgpu_default_ctx(int k, blissgpu_ctx** ctx) {
    if (!ctx) return fail(BLISSGPU_ERR_INVALID, "blissgpu_default_ctx", "NULL argument");
    *ctx = nullptr;
    return default_ctx_at(k, ctx);
}
int blissgpu_set_single_song_timeout_ms(int64_t ms) {
    // "never" (INT64_MAX) must not overflow the nanosecond clock the deadline is computed on: ten years is never
    constexpr int64_t TEN_YEARS_MS = 10LL * 365 * 24 * 3600 * 1000;
    g_single_song_timeout_ms.store(ms > 0 ? std::min(ms, TEN_YEARS_MS) : 600000);
    return BLISSGPU_OK;
}
int blissgpu_default_reset(void) {
    default_ctx_forget_failures();
    front_revive_all();
    return BLISSGPU_OK;
}
int blissgpu_default_device(int k) {
    std::lock_guard<std::mutex> lk(g_default_mu);
    default_init_locked();
    return (k >= 0 && k < (int)g_default_devices.size()) ? g_default_devices[k] : -1;
}
uint64_t blissgpu_default_device_batches(int k) {
    std::lock_guard<std::mutex> lk(g_default_mu);
    return (k >= 0 && k < (int)g_default_batches.size()) ? g_default_batches[k] : 0;
}
}  // extern "C"

namespace {

int is_diag(const float* M, uint32_t d) {
    for (uint32_t i = 0; i < d; i++)
        for (uint32_t j = 0; j < d; j++)
            if (i != j && M[i * d + j] != 0.0f) return 0;
    return 1;
}

// *diag = whether the Mahalanobis matrix d_M [d][d] on the device is diagonal (0 for another metric).  Staged by a host form
// (d_M == c->st_m.p): the host copy is at hand; otherwise it is copied back, which synchronises the stream
int metric_is_diag(blissgpu_ctx* c, const float* d_M, uint32_t d, int metric, int* diag) {
    *diag = 0;
    if (metric != BLISSGPU_METRIC_MAHALANOBIS) return BLISSGPU_OK;
    if (d_M == c->st_m.p && c->m_cache.size() == (size_t)d * d) {
        *diag = is_diag(c->m_cache.data(), d);
    } else {
        std::vector<float> hM((size_t)d * d);
        HIP_TRY(hipMemcpyAsync(hM.data(), d_M, hM.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *diag = is_diag(hM.data(), d);
    }
    return BLISSGPU_OK;
}

}  // namespace

// Locks the context for the duration of one entry point and selects its device.
#define CTX_ENTER(c, who)                                                     \
    if (!(c)) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");          \
    std::lock_guard<std::recursive_mutex> ctx_lock_((c)->mu);                 \
    HIP_TRY(hipSetDevice((c)->device))

extern "C" {

const char* blissgpu_version(void) { return "blissgpu 0.3.0 (gfx950)"; }
const char* blissgpu_last_error(void) { return g_last_error.c_str(); }

const char* blissgpu_strerror(int code) {
    switch (code) {
        case BLISSGPU_OK: return "ok";
        case BLISSGPU_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
        case BLISSGPU_ERR_INVALID: return "invalid argument";
        case BLISSGPU_ERR_HIP: return "HIP runtime error";
        case BLISSGPU_ERR_NAN: return "a distance is NaN";
        case BLISSGPU_ERR_OOM: return "out of device memory";
        case BLISSGPU_ERR_RCCL: return "RCCL error";
        case BLISSGPU_ERR_TIMEOUT: return "no default context picked the call up within its deadline";
        case BLISSGPU_ERR_INTERNAL: return "a bounded loop did not end";
        default: return "unknown error";
    }
}

uint32_t blissgpu_feature_count(uint32_t v) { return v == BLISSGPU_FEATURES_V1 ? 20u : (v == BLISSGPU_FEATURES_V2 ? 23u : 0u); }

int blissgpu_ctx_create(int device, blissgpu_ctx** out) {
    if (!out) return fail(BLISSGPU_ERR_INVALID, "blissgpu_ctx_create", "ctx is NULL");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0 || device < 0 || device >= count)
        return fail(BLISSGPU_ERR_NO_DEVICE, "hipGetDeviceCount", e != hipSuccess ? hipGetErrorString(e) : "no such device");
    HIP_TRY(hipSetDevice(device));
    blissgpu_ctx* c = new blissgpu_ctx();
    c->device = device;
    (void)hipDeviceGetAttribute(&c->n_cus, hipDeviceAttributeMultiprocessorCount, device);
    hipError_t se = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (se != hipSuccess) { delete c; return fail(BLISSGPU_ERR_HIP, "hipStreamCreate", hipGetErrorString(se)); }
    c->stream = c->own_stream;
    // the side streams carry small latency-bound kernels: at high priority they get a CU slot as soon as one frees up
    // instead of queueing behind the thousands of workgroups of an FFT kernel
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    const int prio_aux = prio_greatest;
    se = hipStreamCreateWithPriority(&c->aux_stream, hipStreamNonBlocking, prio_aux);
    if (se == hipSuccess) se = hipStreamCreateWithPriority(&c->chr_stream, hipStreamNonBlocking, prio_greatest);
    if (se == hipSuccess) se = hipEventCreateWithFlags(&c->ev_interop, hipEventDisableTiming);
    if (se == hipSuccess) se = hipHostMalloc((void**)&c->h_scalar, 64, hipHostMallocDefault);
    if (se != hipSuccess) { blissgpu_ctx_destroy(c); return fail(BLISSGPU_ERR_HIP, "aux stream/events", hipGetErrorString(se)); }
    // Scratch limit per chunk slot: a third of what is free now, at most 64 GiB (1024 three-minute songs need ~37 GB).  A
    // batch that needs more runs as several chunks; a chunk that still does not fit (the caller allocated in the meantime)
    // is halved until it does.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
        c->ws_limit = std::max<uint64_t>(256ull << 20, std::min<uint64_t>(64ull << 30, free_b / 3));
    else
        c->ws_limit = 16ull << 30;
    int rc = build_tables(c);
    if (rc) { blissgpu_ctx_destroy(c); return rc; }
    live_context_add(device, 1);
    c->counted_live = true;
    *out = c;
    return BLISSGPU_OK;
}

int blissgpu_ctx_destroy(blissgpu_ctx* c) {
    if (!c) return BLISSGPU_OK;
    if (c->counted_live) live_context_add(c->device, -1);
    {
        std::lock_guard<std::recursive_mutex> lk(c->mu);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
        if (c->chr_stream) (void)hipStreamSynchronize(c->chr_stream);
        if (c->mask_stream) { (void)hipStreamSynchronize(c->mask_stream); (void)hipStreamDestroy(c->mask_stream); }
        for (auto& v : c->events)
            for (auto& ev : v) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
        (void)hipFree(c->tw8192); (void)hipFree(c->tw512); (void)hipFree(c->hann8192); (void)hipFree(c->hannz512);
        (void)hipFree(c->bt_rwv); (void)hipFree(c->bt_dfwv); (void)hipFree(c->chroma_bank);
        scheduler_release(c);
        c->dbg_tuning.release(); c->dbg_nbpms.release(); c->dbg_chroma.release(); c->dbg_interval.release();
        c->pl_sync.release(); c->pl_keys.release(); c->pl_tmp.release(); c->pl_slots.release(); c->pl_chain.release(); c->km_ws.release(); c->sil_ws.release(); c->mo_ws.release(); c->ch_ws.release(); c->ms_ws.release(); c->wd_ws.release(); c->wd_host.release(); c->pam_ws.release(); c->fp_ws.release(); c->ld_ws.release(); c->map_ws.release(); c->mt_ws.release(); c->pl_next.release(); c->st_idx.release();
        c->st_a.release(); c->st_b.release(); c->st_m.release(); c->st_dist.release(); c->st_out.release();
        c->fl_bytes.release(); c->fl_tab.release(); c->fl_pcm.release(); c->fl_status.release(); c->fl_end.release();
        c->fl_bad.release(); c->fl_mono.release(); c->fl_rows.release(); c->fl_htab.release();
        c->fl_vsong.release(); c->fl_md5_jobs.release(); c->fl_md5.release();
        if (c->fl_ev) (void)hipEventDestroy(c->fl_ev);
        for (int s = 0; s < 2; s++) {
            c->gf_img[s].release();
            c->gf_host[s].release();
            if (c->gf_ev[s]) (void)hipEventDestroy(c->gf_ev[s]);
        }
        if (c->h_scalar) (void)hipHostFree(c->h_scalar);
        if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
        if (c->chr_stream) (void)hipStreamDestroy(c->chr_stream);
        if (c->ev_interop) (void)hipEventDestroy(c->ev_interop);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    }
    delete c;
    return BLISSGPU_OK;
}

int blissgpu_ctx_set_stream(blissgpu_ctx* c, void* s) {
    CTX_ENTER(c, "blissgpu_ctx_set_stream");
    (void)hipStreamSynchronize(c->stream);
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return BLISSGPU_OK;
}
void* blissgpu_ctx_get_stream(blissgpu_ctx* c) { return c ? (void*)c->stream : nullptr; }

// Stream interop for hosts that keep their own streams (e.g. torch's current stream, NULL = the legacy default
// stream): order the context's stream after / before work queued on another stream without a host synchronisation.
int blissgpu_ctx_wait_stream(blissgpu_ctx* c, void* producer_stream) {
    CTX_ENTER(c, "blissgpu_ctx_wait_stream");
    if ((hipStream_t)producer_stream == c->stream) return BLISSGPU_OK;
    HIP_TRY(hipEventRecord(c->ev_interop, (hipStream_t)producer_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_interop, 0));
    return BLISSGPU_OK;
}
int blissgpu_ctx_signal_stream(blissgpu_ctx* c, void* consumer_stream) {
    CTX_ENTER(c, "blissgpu_ctx_signal_stream");
    if ((hipStream_t)consumer_stream == c->stream) return BLISSGPU_OK;
    HIP_TRY(hipEventRecord(c->ev_interop, c->stream));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)consumer_stream, c->ev_interop, 0));
    return BLISSGPU_OK;
}

int blissgpu_ctx_set_option(blissgpu_ctx* c, int option, int64_t value) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_ctx_set_option", "ctx is NULL");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // nothing of the previous schedule is in flight when it changes
    switch (option) {
        case BLISSGPU_OPT_SERIAL: c->serial = value != 0; break;
        case BLISSGPU_OPT_TAIL_MODE: c->tail_mode = (int)value; break;
        case BLISSGPU_OPT_PIPELINE_CHUNKS: c->pipeline_chunks = (uint32_t)std::min<int64_t>(64, std::max<int64_t>(1, value)); break;
        case BLISSGPU_OPT_ROLLOFF_EXACT_ALL: c->rolloff_exact_all = value != 0; break;
        case BLISSGPU_OPT_DEBUG_CHROMA: c->debug_chroma = value != 0; break;
        case BLISSGPU_OPT_TAIL_SPLIT: c->tail_split = (int)value; break;
        case BLISSGPU_OPT_FLUX_ORDER: c->flux_order = value != 0; break;
        case BLISSGPU_OPT_STFT_SHAPE: c->stft_shape = (value >= 0 && value <= 3) ? (int)value : 0; break;
        case BLISSGPU_OPT_STAGE_LANES: c->feed.stage_cfg.lanes = (int)std::max<int64_t>(0, std::min<int64_t>(value, bg::MAX_STAGE_LANES)); break;
        case BLISSGPU_OPT_STAGE_SLAB_KIB: c->feed.stage_cfg.slab_bytes = (size_t)std::max<int64_t>(64, std::min<int64_t>(value, 65536)) << 10; break;
        case BLISSGPU_OPT_STAGE_NUMA: c->feed.stage_numa = value != 0; break;
        case BLISSGPU_OPT_STAGE_SLABS: c->feed.stage_cfg.slabs_per_lane = (int)std::max<int64_t>(1, std::min<int64_t>(value, 8)); break;
        case BLISSGPU_OPT_FOREST_SPLIT: c->forest_split = std::max<int64_t>(0, std::min<int64_t>(value, 65535)); break;
        case BLISSGPU_OPT_FOREST_WALK: c->forest_global = value == 1; break;
        case BLISSGPU_OPT_FOREST_GROUP_NODES: c->forest_group_nodes = std::max<int64_t>(0, value); break;
        case BLISSGPU_OPT_CAND_BUDGET: c->cand_budget = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 714)); break;
        default: return fail(BLISSGPU_ERR_INVALID, "blissgpu_ctx_set_option", "unknown option");
    }
    return BLISSGPU_OK;
}

uint64_t blissgpu_ctx_staged_bytes(blissgpu_ctx* c) {
    if (!c) return 0;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    return c->feed.staged_bytes + (c->feed.ring ? c->feed.ring->bytes_staged() : 0);
}

int blissgpu_ctx_set_workspace_limit(blissgpu_ctx* c, uint64_t bytes) {
    if (!c || bytes < (1ull << 20)) return fail(BLISSGPU_ERR_INVALID, "blissgpu_ctx_set_workspace_limit", "limit < 1 MiB");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->ws_limit = bytes;
    return BLISSGPU_OK;
}
uint64_t blissgpu_ctx_get_workspace_limit(blissgpu_ctx* c) { return c ? c->ws_limit : 0; }

int blissgpu_ctx_synchronize(blissgpu_ctx* c) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_ctx_synchronize", "ctx is NULL");
    hipStream_t st;
    { std::lock_guard<std::recursive_mutex> lk(c->mu); st = c->stream; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(st));  // not under the lock: other threads may keep enqueueing
    return BLISSGPU_OK;
}

int blissgpu_host_alloc(void** p, uint64_t bytes) {
    if (!p) return fail(BLISSGPU_ERR_INVALID, "blissgpu_host_alloc", "NULL");
    hipError_t e = hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? BLISSGPU_ERR_OOM : BLISSGPU_ERR_NO_DEVICE, "hipHostMalloc", hipGetErrorString(e));
    return BLISSGPU_OK;
}
int blissgpu_host_free(void* p) { HIP_TRY(hipHostFree(p)); return BLISSGPU_OK; }

int blissgpu_feature_weights(uint32_t features_version, float* M) {
    const uint32_t d = blissgpu_feature_count(features_version);
    if (!d || !M) return fail(BLISSGPU_ERR_INVALID, "blissgpu_feature_weights", "bad version or NULL");
    memset(M, 0, sizeof(float) * d * d);
    for (uint32_t i = 0; i < d; i++) {
        float w = 1.0f;
        if (features_version == BLISSGPU_FEATURES_V2) {  // VERSION2_WEIGHTS, src/lib.rs:209-234
            if (i == 0) w = 0.25f;
            else if (i >= 10) w = 3.0f / 13.0f;
        }
        M[i * d + i] = w;
    }
    return BLISSGPU_OK;
}

int blissgpu_pairwise_device(blissgpu_ctx* c, const float* d_A, uint64_t n, const float* d_B, uint64_t m, uint32_t d,
                             int metric, const float* d_M, float* d_out, uint64_t ld_out) {
    if (!c || !d_A || !d_B || !d_out) return fail(BLISSGPU_ERR_INVALID, "blissgpu_pairwise_device", "NULL argument");
    if (d == 0 || d > 64 || metric < 0 || metric > 2 || ld_out < m)
        return fail(BLISSGPU_ERR_INVALID, "blissgpu_pairwise_device", "bad d / metric / ld_out");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !d_M)
        return fail(BLISSGPU_ERR_INVALID, "blissgpu_pairwise_device", "mahalanobis needs M");
    CTX_ENTER(c, "blissgpu_pairwise_device");
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    {
        Prof p(c, K_PAIRWISE);
        launch_pairwise(d_A, n, d_B, m, d, metric, d_M, diag, d_out, ld_out, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return BLISSGPU_OK;
}

}  // extern "C"

namespace {

// Stage the d x d matrix of a host-pointer call in the context (uploaded only when it differs from the one staged last:
// a library is ordered with the same weights over and over).  Returns the device pointer through *d_M (NULL if none).
int stage_matrix(blissgpu_ctx* c, const float* M, uint32_t d, int metric, const float** d_M) {
    *d_M = nullptr;
    if (metric != BLISSGPU_METRIC_MAHALANOBIS) return BLISSGPU_OK;
    const size_t n = (size_t)d * d;
    int rc = c->st_m.ensure(4096);  // 64 x 64: never regrown, so the pointer identifies "staged by us"
    if (rc) return rc;
    if (c->m_cache.size() != n || memcmp(c->m_cache.data(), M, n * sizeof(float)) != 0) {
        c->m_cache.assign(M, M + n);
        // the source is the context's own copy: the caller's buffer may go away as soon as the call returns
        HIP_TRY(hipMemcpyAsync(c->st_m.p, c->m_cache.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *d_M = c->st_m.p;
    return BLISSGPU_OK;
}

// The copies of one host-pointer form around its device form: inputs up, results down, the first HIP error
// kept and reported under the family's tag.  An absent array (NULL) and an empty one (0 bytes) are not copied.
struct HostStage {
    blissgpu_ctx* c;
    const char* tag;  // "chains": the family in "hipMemcpyAsync(chains)" / "copy back(chains)"
    hipError_t e = hipSuccess;
    bool queued = false;  // a copy back is on the stream
    void up(void* dst, const void* src, size_t bytes) {
        if (src && bytes && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    }
    int uploaded() const { return e == hipSuccess ? BLISSGPU_OK : report("hipMemcpyAsync("); }
    void down(void* dst, const void* src, size_t bytes) {
        if (!dst || !bytes || e != hipSuccess) return;
        e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
        queued = true;
    }
    // waits for the copies back; a form calls it itself where further copies depend on what came back
    int landed() {
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        queued = false;
        return e == hipSuccess ? BLISSGPU_OK : report("copy back(");
    }
    // the end of every host form: rc = what the uploads and the device form returned
    int finish(int rc) {
        if (!rc && queued) rc = landed();
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    int report(const char* what) const { return fail(BLISSGPU_ERR_HIP, (std::string(what) + tag + ")").c_str(), hipGetErrorString(e)); }
};

// The host form of the families that answer one list per seed group (group_knn, group_knn_weighted, chains, album_knn,
// group_forest_knn), the way knn_host serves both searches, in two steps.  group_lists_stage grows the buffers and says where
// everything goes: candidates in st_b, seeds in st_a (stage_seeds; the forests keep theirs on the host), idx | skip in st_idx,
// dist_floats floats (0: none) in st_dist, M staged; nothing is queued yet, so a caller returns at once when it fails.
// group_lists_host copies the inputs up, runs `run`, the family's device form on these pointers, and queues idx and dist back.
// What a family stages beside that it queues on s itself: uploads in `run` before its device call, copies back after
// group_lists_host; then s.finish.
struct GroupLists {
    float *seeds, *cand;  // seeds == NULL: not staged
    const float* M;
    uint32_t *skip, *idx;
    float* dist;
};
int group_lists_stage(blissgpu_ctx* c, uint64_t n_seeds, bool stage_seeds, uint64_t n, uint32_t d, int metric, const float* M,
                      bool skip, size_t out_n, size_t dist_floats, GroupLists* g) {
    const float* dM = nullptr;
    int rc = c->st_b.ensure(std::max<size_t>(1, n * d));
    if (!rc && stage_seeds) rc = c->st_a.ensure(std::max<size_t>(1, n_seeds * d));
    if (!rc) rc = c->st_idx.ensure(out_n + (skip ? n_seeds : 0));
    if (!rc && dist_floats) rc = c->st_dist.ensure(dist_floats);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    *g = GroupLists{stage_seeds ? c->st_a.p : nullptr, c->st_b.p, dM, skip ? c->st_idx.p + out_n : nullptr, c->st_idx.p,
                    dist_floats ? c->st_dist.p : nullptr};
    return BLISSGPU_OK;
}
template <typename Run>
int group_lists_host(HostStage& s, const GroupLists& g, const float* seeds, uint64_t n_seeds, const float* cand, uint64_t n, uint32_t d,
                     const uint32_t* skip, size_t out_n, uint32_t* idx, float* dist, Run run) {
    s.up(g.cand, cand, n * d * sizeof(float));
    if (g.seeds) s.up(g.seeds, seeds, n_seeds * d * sizeof(float));
    s.up(g.skip, skip, n_seeds * sizeof(uint32_t));
    int rc = s.uploaded();
    if (!rc) rc = run();
    if (!rc) {
        s.down(idx, g.idx, out_n * sizeof(uint32_t));
        s.down(dist, g.dist, out_n * sizeof(float));
    }
    return rc;
}

// a host form's skip array, checked before the device is touched
int skip_entries_ok(const char* who, const uint32_t* skip, uint64_t count, uint64_t n) {
    if (skip)
        for (uint64_t i = 0; i < count; i++)
            if (skip[i] != 0xFFFFFFFFu && skip[i] >= n) return fail(BLISSGPU_ERR_INVALID, who, "skip entries must be < n or 0xFFFFFFFF");
    return BLISSGPU_OK;
}

// the device flag words of a call, read back: the synchronisation every device form ends in
int read_flags(blissgpu_ctx* c, const uint32_t* d_flags, uint32_t count, uint32_t* h_flags) {
    HIP_TRY(hipMemcpyAsync(h_flags, d_flags, count * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BLISSGPU_OK;
}

// The k-means sort of a labelling of n songs into k groups, at the head of a call's workspace (the words: launch_forms.hpp):
// labels -> arow_off (the groups' offsets) and arow (their rows).  The call's flags are the workspace's first four words, so that
// one memset of zero_words() clears them with the histograms, which the sort needs zero on entry
struct LabelSort : LabelSortWords {
    KmeansPlan plan;
    uint32_t k, n;
    uint32_t *flags = nullptr, *hist = nullptr, *bsum = nullptr, *arow_off = nullptr, *arow = nullptr;
    LabelSort(const KmeansPlan& plan, uint32_t k, uint64_t n)
        : LabelSortWords(label_sort_words(plan.hist_words, plan.scan_tiles, k, n)), plan(plan), k(k), n((uint32_t)n) {}
    void bind(uint32_t* w) { flags = w; hist = w + o_hist; bsum = w + o_bsum; arow_off = w + o_off; arow = w + o_arow; }
    size_t zero_words() const { return o_bsum; }
    // (without the rows: the offsets alone; hist is then left at the positions the scatter would start from)
    void launch(blissgpu_ctx* c, const uint32_t* d_labels, bool with_rows = true) const {
        { Prof p(c, KX_KMEANS_HIST); launch_kmeans_hist(d_labels, n, k, plan, hist, c->stream); }
        { Prof p(c, KX_KMEANS_SCAN_TILES); launch_kmeans_scan_tiles(hist, plan, bsum, c->stream); }
        { Prof p(c, KX_KMEANS_SCAN_ADD); launch_kmeans_scan_add(hist, n, k, plan, bsum, arow_off, c->stream); }
        if (with_rows) { Prof p(c, KX_KMEANS_SCATTER); launch_kmeans_scatter(d_labels, n, k, plan, hist, arow, c->stream); }
    }
};

}  // namespace

extern "C" {

int blissgpu_pairwise(const float* A, uint64_t n, const float* B, uint64_t m, uint32_t d, int metric, const float* M,
                      float* out) {
    if (!A || !B || !out) return fail(BLISSGPU_ERR_INVALID, "blissgpu_pairwise", "NULL argument");
    if (d == 0 || d > 64 || metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, "blissgpu_pairwise", "bad d / metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, "blissgpu_pairwise", "mahalanobis needs M");
    if (n == 0 || m == 0) return BLISSGPU_OK;
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, "blissgpu_pairwise");
    // rows of the output are produced in slabs of <= 4 GiB so host-sized problems never need n*m device memory
    const uint64_t slab_rows = std::max<uint64_t>(1, std::min<uint64_t>(n, (1ull << 30) / std::max<uint64_t>(m, 1)));
    const bool self = (A == B && n == m);  // self-distance matrix: one device copy, symmetric kernel
    const float* dM = nullptr;
    if ((rc = c->st_a.ensure(n * d))) return rc;
    if (!self && (rc = c->st_b.ensure(m * d))) return rc;
    if ((rc = c->st_out.ensure(slab_rows * m * sizeof(float)))) return rc;
    if ((rc = stage_matrix(c, M, d, metric, &dM))) return rc;
    float *dA = c->st_a.p, *dB = self ? c->st_a.p : c->st_b.p, *dO = reinterpret_cast<float*>(c->st_out.p);
    hipError_t e = hipMemcpyAsync(dA, A, n * d * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && !self) e = hipMemcpyAsync(dB, B, m * d * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) rc = fail(BLISSGPU_ERR_HIP, "hipMemcpyAsync", hipGetErrorString(e));
    for (uint64_t r0 = 0; !rc && r0 < n; r0 += slab_rows) {
        const uint64_t rows = std::min(slab_rows, n - r0);
        // a row slab of a self-distance matrix is not square: only the full matrix takes the symmetric kernel
        rc = blissgpu_pairwise_device(c, dA + r0 * d, rows, dB, m, d, metric, dM, dO, m);
        if (!rc) {
            e = hipMemcpyAsync(out + r0 * m, dO, rows * m * sizeof(float), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = fail(BLISSGPU_ERR_HIP, "copy back", hipGetErrorString(e));
        }
    }
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

// One pair: both vectors travel in the kernel arguments and the result lands in a page-locked word, so the call is
// one launch + one stream synchronisation -- no allocation, no staging copy (Song::distance, src/song/mod.rs:519-521).
int blissgpu_distance(const float* a, const float* b, uint32_t d, int metric, const float* M, float* out) {
    if (!a || !b || !out) return fail(BLISSGPU_ERR_INVALID, "blissgpu_distance", "NULL argument");
    if (d == 0 || d > 64 || metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, "blissgpu_distance", "bad d / metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, "blissgpu_distance", "mahalanobis needs M");
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, "blissgpu_distance");
    const float* dM = nullptr;
    if ((rc = stage_matrix(c, M, d, metric, &dM))) return rc;
    launch_pair_distance(a, b, d, metric, dM, c->h_scalar, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = *c->h_scalar;
    return BLISSGPU_OK;
}

// ---- playlist ordering (src/playlist.rs:24-59, 256-326) ----
static int playlist_args_ok(const char* who, const void* a, const void* b, const void* o, uint32_t n_seeds, uint64_t n,
                            uint32_t d, int metric, const float* M) {
    // An EMPTY seed set is legal: FunctionDistanceMetric::distance sums over no vectors, i.e. 0.0 for every candidate
    // (src/playlist.rs:52-58) -- closest_to_songs then keeps the candidates' order (stable sort) and song_to_song
    // starts from the first candidate.
    if ((n_seeds && !a) || (n && !b) || !o) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (d == 0 || d > 64 || metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, who, "bad d / metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n > 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "more than 2^32 - 1 candidates");
    return BLISSGPU_OK;
}

// reads the device NaN flag (synchronises the stream)
static int nan_check(blissgpu_ctx* c, const uint32_t* d_flag, const char* who) {
    uint32_t flag = 0;
    if (int rc = read_flags(c, d_flag, 1, &flag)) return rc;
    if (flag) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

int blissgpu_set_distance_device(blissgpu_ctx* c, const float* d_seeds, uint32_t n_seeds, const float* d_cand, uint64_t n,
                                 uint32_t d, int metric, const float* d_M, float* d_out) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_set_distance_device", "ctx is NULL");
    int rc = playlist_args_ok("blissgpu_set_distance_device", d_seeds, d_cand, d_out, n_seeds, n, d, metric, d_M);
    if (rc) return rc;
    if (n == 0) return BLISSGPU_OK;
    CTX_ENTER(c, "blissgpu_set_distance_device");
    rc = c->pl_sync.ensure(4);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    {
        Prof p(c, K_SET_DISTANCE);
        launch_set_distance(d_seeds, n_seeds, d_cand, n, d, metric, d_M, d_out, nullptr, nullptr, c->pl_sync.p + 1, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return BLISSGPU_OK;  // NaN distances are returned as data here, like DistanceMetric::distance
}

int blissgpu_closest_to_songs_device(blissgpu_ctx* c, const float* d_seeds, uint32_t n_seeds, const float* d_cand,
                                     uint64_t n, uint32_t d, int metric, const float* d_M, uint32_t* d_order, float* d_dist) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_closest_to_songs_device", "ctx is NULL");
    int rc = playlist_args_ok("blissgpu_closest_to_songs_device", d_seeds, d_cand, d_order, n_seeds, n, d, metric, d_M);
    if (rc) return rc;
    if (n == 0) return BLISSGPU_OK;
    CTX_ENTER(c, "blissgpu_closest_to_songs_device");
    const uint32_t n32 = (uint32_t)n;
    size_t tmp_bytes = 0;
    HIP_TRY(sort_pairs_u32(nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, n32, c->stream));
    rc = c->pl_sync.ensure(4);
    if (!rc) rc = c->pl_keys.ensure((size_t)3 * n32);  // keys in | keys out | indices in
    if (!rc) rc = c->pl_tmp.ensure(tmp_bytes);
    if (rc) return rc;
    uint32_t *keys_in = c->pl_keys.p, *keys_out = keys_in + n32, *idx_in = keys_out + n32;
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    {
        Prof p(c, K_SET_DISTANCE);
        launch_set_distance(d_seeds, n_seeds, d_cand, n, d, metric, d_M, d_dist, keys_in, idx_in, c->pl_sync.p + 1, c->stream);
    }
    HIP_TRY(hipGetLastError());
    // the single-launch sort spins on grid barriers: only while its workgroups are certainly co-resident (one per CU, and at
    // most two contexts' worth of persistent kernels on the device); otherwise one launch per step
    HIP_TRY(sort_pairs_u32(c->pl_tmp.p, &tmp_bytes, keys_in, keys_out, idx_in, d_order, n32, c->stream, c->pl_sync.p + 2,
                           live_contexts(c->device) <= 2 ? (uint32_t)std::max(1, c->n_cus) : 0u));
    return nan_check(c, c->pl_sync.p + 1, "blissgpu_closest_to_songs_device");
}

int blissgpu_song_to_song_device(blissgpu_ctx* c, const float* d_seeds, uint32_t n_seeds, const float* d_cand, uint64_t n,
                                 uint32_t d, int metric, const float* d_M, uint32_t* d_order) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_song_to_song_device", "ctx is NULL");
    int rc = playlist_args_ok("blissgpu_song_to_song_device", d_seeds, d_cand, d_order, n_seeds, n, d, metric, d_M);
    if (rc) return rc;
    if (n == 0) return BLISSGPU_OK;
    CTX_ENTER(c, "blissgpu_song_to_song_device");
    // one workgroup per 256 candidates up to one per CU (all workgroups must be co-resident: the kernel spins on
    // a grid barrier); each thread then owns ceil(n / (256 G)) <= 64 candidates
    // four candidates per thread (register-resident) is the sweet spot: fewer workgroups make the grid barrier and the
    // slot reduction cheaper (100 k songs: 98 workgroups, 7.3 us per step; 256 workgroups with two each: 11.7 us)
    uint32_t grid = (uint32_t)std::min<uint64_t>((n + 1023) / 1024, (uint64_t)std::min(256, std::max(1, c->n_cus)));
    if ((n + (uint64_t)grid * 256 - 1) / ((uint64_t)grid * 256) > 64)
        return fail(BLISSGPU_ERR_INVALID, "blissgpu_song_to_song_device", "pool too large for one launch (> 64 candidates per thread)");
    rc = c->pl_sync.ensure(4);
    if (!rc) rc = c->pl_slots.ensure((size_t)2 * grid);
    if (rc) return rc;
    // more than two contexts alive on this device: spinning grids of different contexts must not overlap (see live_contexts)
    std::unique_lock<std::mutex> one_at_a_time;
    if (live_contexts(c->device) > 2) one_at_a_time = std::unique_lock<std::mutex>(persistent_kernel_mutex(c->device));
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    {
        Prof p(c, K_SONG_TO_SONG);
        launch_song_to_song(d_seeds, n_seeds, d_cand, (uint32_t)n, d, metric, d_M, d_order, c->pl_slots.p, c->pl_sync.p, grid,
                            c->stream);
    }
    HIP_TRY(hipGetLastError());
    if (one_at_a_time.owns_lock()) HIP_TRY(hipStreamSynchronize(c->stream));  // the chain has left the CUs before the next one starts
    return nan_check(c, c->pl_sync.p + 1, "blissgpu_song_to_song_device");
}

// ---- dedup_playlist_custom_distance (src/playlist.rs:343-402) over a playlist of rows ----
static int dedup_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, const void* seq, uint64_t len, int metric,
                         const float* M, const void* kept, const void* n_kept) {
    int rc = playlist_args_ok(who, x, x, kept, n ? 1u : 0u, n, d, metric, M);
    if (rc) return rc;
    if (!n_kept) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (!seq && len && len != n) return fail(BLISSGPU_ERR_INVALID, who, "seq == NULL needs len == n");
    if (len > 0x7FFFFFFEull) return fail(BLISSGPU_ERR_INVALID, who, "more than 2^31 - 2 playlist entries");
    if (len && !n) return fail(BLISSGPU_ERR_INVALID, who, "seq entries must be < n");
    return BLISSGPU_OK;
}

int blissgpu_dedup_playlist_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const uint32_t* d_seq,
                                   uint64_t len, const uint32_t* d_meta, int metric, const float* d_M, float threshold,
                                   uint32_t* d_kept, uint64_t* d_n_kept) {
    const char* who = "blissgpu_dedup_playlist_device";
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    int rc = dedup_args_ok(who, d_x, n, d, d_seq, len, metric, d_M, d_kept, d_n_kept);
    if (rc) return rc;
    CTX_ENTER(c, who);
    if (len == 0) {
        HIP_TRY(hipMemsetAsync(d_n_kept, 0, sizeof(uint64_t), c->stream));
        return BLISSGPU_OK;
    }
    const uint32_t len32 = (uint32_t)len;
    rc = c->pl_sync.ensure(4);
    if (!rc) rc = c->pl_next.ensure(len32);
    if (rc) return rc;
    // pl_sync: [1] NaN on the chain, [3] a seq entry >= n
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    {
        Prof p(c, K_DEDUP_NEXT);
        launch_dedup_next(d_x, n, d, d_seq, len32, d_meta, metric, d_M, threshold, c->pl_next.p, c->pl_sync.p + 3, c->stream);
    }
    HIP_TRY(hipGetLastError());
    {
        Prof p(c, K_DEDUP_WALK);
        launch_dedup_walk(d_x, n, d, d_seq, len32, d_meta, metric, d_M, threshold, c->pl_next.p, d_kept, d_n_kept,
                          c->pl_sync.p + 1, c->pl_sync.p + 3, c->stream);
    }
    HIP_TRY(hipGetLastError());
    uint32_t flags[4];
    if ((rc = read_flags(c, c->pl_sync.p, 4, flags))) return rc;
    if (flags[3]) return fail(BLISSGPU_ERR_INVALID, who, "seq entries must be < n");
    if (flags[1]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

}  // extern "C"

// host-pointer wrappers: stage seeds / candidates / M in the context's buffers, run the device form, copy the result back
namespace {
struct PlStage {
    HostStage s;
    float *seeds = nullptr, *cand = nullptr, *dist = nullptr;
    const float* M = nullptr;
    void* out = nullptr;
    explicit PlStage(blissgpu_ctx* c) : s{c, "playlist"} {}
    int up(const float* h_seeds, uint32_t n_seeds, const float* h_cand, uint64_t n, uint32_t d, int metric, const float* h_M,
           size_t out_bytes, bool want_dist) {
        blissgpu_ctx* c = s.c;
        int rc = c->st_a.ensure(std::max<size_t>(1, (size_t)n_seeds * d));
        if (!rc) rc = c->st_b.ensure(std::max<size_t>(1, n * d));
        if (!rc) rc = c->st_out.ensure(std::max<size_t>(4, out_bytes));
        if (!rc && want_dist) rc = c->st_dist.ensure(std::max<size_t>(1, n));
        if (!rc) rc = stage_matrix(c, h_M, d, metric, &M);
        if (rc) return rc;
        seeds = c->st_a.p; cand = c->st_b.p; out = c->st_out.p; dist = want_dist ? c->st_dist.p : nullptr;
        s.up(seeds, h_seeds, (size_t)n_seeds * d * sizeof(float));
        s.up(cand, h_cand, n * d * sizeof(float));
        return s.uploaded();
    }
    // the end of the three forms: rc = what up and the device form returned
    int down(int rc, void* h_out, size_t out_bytes, float* h_dist, uint64_t n) {
        if (!rc) {
            s.down(h_out, out, out_bytes);
            s.down(h_dist, dist, n * sizeof(float));
        }
        return s.finish(rc);
    }
};
}  // namespace

extern "C" {

int blissgpu_set_distance(const float* seeds, uint32_t n_seeds, const float* cand, uint64_t n, uint32_t d, int metric,
                          const float* M, float* out) {
    int rc = playlist_args_ok("blissgpu_set_distance", seeds, cand, out, n_seeds, n, d, metric, M);
    if (rc || n == 0) return rc;
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, "blissgpu_set_distance");
    PlStage s(c);
    rc = s.up(seeds, n_seeds, cand, n, d, metric, M, n * sizeof(float), false);
    if (!rc) rc = blissgpu_set_distance_device(c, s.seeds, n_seeds, s.cand, n, d, metric, s.M, (float*)s.out);
    return s.down(rc, out, n * sizeof(float), nullptr, 0);
}

int blissgpu_closest_to_songs(const float* seeds, uint32_t n_seeds, const float* cand, uint64_t n, uint32_t d, int metric,
                              const float* M, uint32_t* order, float* dist) {
    int rc = playlist_args_ok("blissgpu_closest_to_songs", seeds, cand, order, n_seeds, n, d, metric, M);
    if (rc || n == 0) return rc;
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, "blissgpu_closest_to_songs");
    PlStage s(c);
    rc = s.up(seeds, n_seeds, cand, n, d, metric, M, n * sizeof(uint32_t), dist != nullptr);
    if (!rc) rc = blissgpu_closest_to_songs_device(c, s.seeds, n_seeds, s.cand, n, d, metric, s.M, (uint32_t*)s.out, s.dist);
    return s.down(rc, order, n * sizeof(uint32_t), dist, n);
}

int blissgpu_song_to_song(const float* seeds, uint32_t n_seeds, const float* cand, uint64_t n, uint32_t d, int metric,
                          const float* M, uint32_t* order) {
    int rc = playlist_args_ok("blissgpu_song_to_song", seeds, cand, order, n_seeds, n, d, metric, M);
    if (rc || n == 0) return rc;
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, "blissgpu_song_to_song");
    PlStage s(c);
    rc = s.up(seeds, n_seeds, cand, n, d, metric, M, n * sizeof(uint32_t), false);
    if (!rc) rc = blissgpu_song_to_song_device(c, s.seeds, n_seeds, s.cand, n, d, metric, s.M, (uint32_t*)s.out);
    return s.down(rc, order, n * sizeof(uint32_t), nullptr, 0);
}

int blissgpu_dedup_playlist(const float* x, uint64_t n, uint32_t d, const uint32_t* seq, uint64_t len, const uint32_t* meta,
                            int metric, const float* M, float threshold, uint32_t* kept, uint64_t* n_kept) {
    const char* who = "blissgpu_dedup_playlist";
    int rc = dedup_args_ok(who, x, n, d, seq, len, metric, M, kept, n_kept);
    if (rc) return rc;
    if (seq)
        for (uint64_t i = 0; i < len; i++)
            if (seq[i] >= n) return fail(BLISSGPU_ERR_INVALID, who, "seq entries must be < n");
    *n_kept = 0;
    if (len == 0) return BLISSGPU_OK;
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    // st_idx: n_kept (two words) | kept[len] | seq[len] | meta[n]
    const size_t o_kept = 2, o_seq = o_kept + len, o_meta = o_seq + (seq ? len : 0);
    const float* dM = nullptr;
    rc = c->st_b.ensure(std::max<size_t>(1, n * d));
    if (!rc) rc = c->st_idx.ensure(o_meta + (meta ? n : 0));
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    uint32_t* idx = c->st_idx.p;
    HostStage s{c, "dedup"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(idx + o_seq, seq, len * sizeof(uint32_t));
    s.up(idx + o_meta, meta, n * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc)
        rc = blissgpu_dedup_playlist_device(c, c->st_b.p, n, d, seq ? idx + o_seq : nullptr, len, meta ? idx + o_meta : nullptr,
                                            metric, dM, threshold, idx + o_kept, reinterpret_cast<uint64_t*>(idx));
    uint64_t nk = 0;
    if (!rc) {  // the device form has synchronised: the count is there
        s.down(&nk, idx, sizeof(nk));
        rc = s.landed();
        if (!rc) {
            s.down(kept, idx + o_kept, nk * sizeof(uint32_t));
            rc = s.landed();
        }
    }
    rc = s.finish(rc);
    if (!rc) *n_kept = nk;
    return rc;
}

// ---- k nearest candidates per query: closest_to_songs(&[query], candidates, metric) cut after k (src/playlist.rs:256-270), the
// primitive behind Library::playlist_from(&[song]).take(k) (src/library.rs:762-850), for q queries in one call ----
// everything that can be said about the arguments without a device (both forms check it BEFORE the device is touched)
static int knn_args_ok(const char* who, const void* queries, uint64_t q, const void* cand, uint64_t n, uint32_t d, int metric,
                       const float* M, uint32_t k, const void* idx) {
    if (k == 0 || k > BLISSGPU_KNN_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KNN_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 candidates");
    if (q > (1ull << 40)) return fail(BLISSGPU_ERR_INVALID, who, "q must be at most 2^40 queries");
    if (q && !queries) return fail(BLISSGPU_ERR_INVALID, who, "queries is NULL");
    if (q && n && !cand) return fail(BLISSGPU_ERR_INVALID, who, "cand is NULL");
    if (q && !idx) return fail(BLISSGPU_ERR_INVALID, who, "idx is NULL");
    return BLISSGPU_OK;
}

// locally scaled: blissgpu_knn's selection under dist / sqrtf(qscale[i] * cscale[j]), the cure for hubs (kernels_scaled_knn.hip,
// DESIGN.md 3.27); the same scan, split and merge
static int scaled_knn_args_ok(const char* who, const void* queries, uint64_t q, const void* qscale, const void* cand, uint64_t n,
                              const void* cscale, uint32_t d, int metric, const float* M, uint32_t k, const void* idx) {
    int rc = knn_args_ok(who, queries, q, cand, n, d, metric, M, k, idx);
    if (rc) return rc;
    if (q && !qscale) return fail(BLISSGPU_ERR_INVALID, who, "qscale is NULL");
    if (q && n && !cscale) return fail(BLISSGPU_ERR_INVALID, who, "cscale is NULL");
    return BLISSGPU_OK;
}

// the device form of both searches, their arguments checked; d_qscale == NULL: the plain one (d_cscale is then not looked at)
static int knn_run(blissgpu_ctx* c, const char* who, const float* d_queries, uint64_t q, const float* d_qscale, const float* d_cand,
                   uint64_t n, const float* d_cscale, uint32_t d, int metric, const float* d_M, const uint32_t* d_skip, uint32_t k,
                   uint32_t* d_idx, float* d_dist) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (q == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // workspace: the sorted k best keys of every (query, split) -- O(q k), see knn_plan; no q x n tile exists anywhere
    const KnnPlan plan = knn_plan(q, n, k, c->n_cus);
    int rc = c->pl_sync.ensure(4);
    if (!rc) rc = c->pl_tmp.ensure((size_t)plan.part_keys * sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long* part = reinterpret_cast<unsigned long long*>(c->pl_tmp.p);
    // pl_sync: [1] NaN among the evaluated distances, [2] a scale outside [2^-60, 2^60], [3] a skip entry >= n
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    {
        Prof p(c, d_qscale ? KX_SCALED_KNN_SCAN : K_KNN_SCAN);
        if (d_qscale)
            launch_scaled_knn_scan(d_queries, q, d_qscale, d_cand, (uint32_t)n, d_cscale, d, metric, d_M, diag, d_skip, k, plan, part,
                                   c->pl_sync.p + 1, c->pl_sync.p + 3, c->pl_sync.p + 2, c->stream);
        else
            launch_knn_scan(d_queries, q, d_cand, (uint32_t)n, d, metric, d_M, diag, d_skip, k, plan, part, c->pl_sync.p + 1,
                            c->pl_sync.p + 3, c->stream);
    }
    HIP_TRY(hipGetLastError());
    {
        Prof p(c, K_KNN_MERGE);
        launch_knn_merge(part, q, k, plan, d_idx, d_dist, c->stream);
    }
    HIP_TRY(hipGetLastError());
    uint32_t flags[4];
    if ((rc = read_flags(c, c->pl_sync.p, 4, flags))) return rc;
    if (flags[3]) return fail(BLISSGPU_ERR_INVALID, who, "skip entries must be < n or 0xFFFFFFFF");
    if (flags[2]) return fail(BLISSGPU_ERR_INVALID, who, "scales must lie in [2^-60, 2^60]");
    if (flags[1]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

// the host form of both, their arguments checked; qscale == NULL: the plain one.  run_who: the device form's name
static int knn_host(const char* who, const char* run_who, const float* queries, uint64_t q, const float* qscale, const float* cand,
                    uint64_t n, const float* cscale, uint32_t d, int metric, const float* M, const uint32_t* skip, uint32_t k,
                    uint32_t* idx, float* dist) {
    int rc = skip_entries_ok(who, skip, q, n);
    if (rc || q == 0) return rc;
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    // queries that ARE the candidate matrix (the similar-songs table of a library), with the same scales, travel once:
    // st_b = cand | cscale, st_a = queries | qscale
    const bool scaled = qscale != nullptr, shared = queries == cand && qscale == cscale && q <= n;
    const size_t out_n = (size_t)q * k;
    const float* dM = nullptr;
    rc = c->st_b.ensure(std::max<size_t>(1, n * d + (scaled ? n : 0)));
    if (!rc && !shared) rc = c->st_a.ensure(q * d + (scaled ? q : 0));
    if (!rc) rc = c->st_idx.ensure(out_n + (skip ? q : 0));
    if (!rc && dist) rc = c->st_dist.ensure(out_n);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    const float* dQ = shared ? c->st_b.p : c->st_a.p;
    float* d_cs = scaled ? c->st_b.p + n * d : nullptr;
    const float* d_qs = !scaled ? nullptr : shared ? d_cs : c->st_a.p + q * d;
    uint32_t *d_idx = c->st_idx.p, *d_skip = skip ? c->st_idx.p + out_n : nullptr;
    HostStage s{c, scaled ? "scaled_knn" : "knn"};
    s.up(c->st_b.p, cand, n * d * sizeof(float));
    s.up(d_cs, cscale, n * sizeof(float));
    if (!shared) {
        s.up(c->st_a.p, queries, q * d * sizeof(float));
        s.up(c->st_a.p + q * d, qscale, q * sizeof(float));
    }
    s.up(d_skip, skip, q * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc) rc = knn_run(c, run_who, dQ, q, d_qs, c->st_b.p, n, d_cs, d, metric, dM, d_skip, k, d_idx, dist ? c->st_dist.p : nullptr);
    if (!rc) {
        s.down(idx, d_idx, out_n * sizeof(uint32_t));
        s.down(dist, c->st_dist.p, out_n * sizeof(float));
    }
    return s.finish(rc);
}

int blissgpu_knn_device(blissgpu_ctx* c, const float* d_queries, uint64_t q, const float* d_cand, uint64_t n, uint32_t d,
                        int metric, const float* d_M, const uint32_t* d_skip, uint32_t k, uint32_t* d_idx, float* d_dist) {
    const char* who = "blissgpu_knn_device";
    const int rc = knn_args_ok(who, d_queries, q, d_cand, n, d, metric, d_M, k, d_idx);
    return rc ? rc : knn_run(c, who, d_queries, q, nullptr, d_cand, n, nullptr, d, metric, d_M, d_skip, k, d_idx, d_dist);
}

int blissgpu_knn(const float* queries, uint64_t q, const float* cand, uint64_t n, uint32_t d, int metric, const float* M,
                 const uint32_t* skip, uint32_t k, uint32_t* idx, float* dist) {
    const char* who = "blissgpu_knn";
    const int rc = knn_args_ok(who, queries, q, cand, n, d, metric, M, k, idx);
    return rc ? rc : knn_host(who, "blissgpu_knn_device", queries, q, nullptr, cand, n, nullptr, d, metric, M, skip, k, idx, dist);
}

int blissgpu_scaled_knn_device(blissgpu_ctx* c, const float* d_queries, uint64_t q, const float* d_qscale, const float* d_cand,
                               uint64_t n, const float* d_cscale, uint32_t d, int metric, const float* d_M, const uint32_t* d_skip,
                               uint32_t k, uint32_t* d_idx, float* d_dist) {
    const char* who = "blissgpu_scaled_knn_device";
    const int rc = scaled_knn_args_ok(who, d_queries, q, d_qscale, d_cand, n, d_cscale, d, metric, d_M, k, d_idx);
    return rc ? rc : knn_run(c, who, d_queries, q, d_qscale, d_cand, n, d_cscale, d, metric, d_M, d_skip, k, d_idx, d_dist);
}

int blissgpu_scaled_knn(const float* queries, uint64_t q, const float* qscale, const float* cand, uint64_t n, const float* cscale,
                        uint32_t d, int metric, const float* M, const uint32_t* skip, uint32_t k, uint32_t* idx, float* dist) {
    const char* who = "blissgpu_scaled_knn";
    const int rc = scaled_knn_args_ok(who, queries, q, qscale, cand, n, cscale, d, metric, M, k, idx);
    return rc ? rc
              : knn_host(who, "blissgpu_scaled_knn_device", queries, q, qscale, cand, n, cscale, d, metric, M, skip, k, idx, dist);
}

// ---- k-occurrence: how many lists of an index matrix every song is in (the counts hubness is measured on) ----
static int occurrence_args_ok(const char* who, const void* idx, uint64_t q, uint32_t k, uint64_t n, const void* count) {
    if (k == 0) return fail(BLISSGPU_ERR_INVALID, who, "k must be at least 1");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 songs");
    if (q > (1ull << 40) / k) return fail(BLISSGPU_ERR_INVALID, who, "q * k must be at most 2^40 entries");
    if (q && !idx) return fail(BLISSGPU_ERR_INVALID, who, "idx is NULL");
    if (n && !count) return fail(BLISSGPU_ERR_INVALID, who, "count is NULL");
    return BLISSGPU_OK;
}

int blissgpu_knn_occurrence_device(blissgpu_ctx* c, const uint32_t* d_idx, uint64_t q, uint32_t k, uint64_t n, uint32_t* d_count) {
    const char* who = "blissgpu_knn_occurrence_device";
    int rc = occurrence_args_ok(who, d_idx, q, k, n, d_count);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (q == 0 && n == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    if (n) HIP_TRY(hipMemsetAsync(d_count, 0, n * sizeof(uint32_t), c->stream));
    uint32_t flag = 0;
    if (q) {
        rc = c->pl_sync.ensure(4);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
        // (for the bench tool's A/B: the windowed LDS histogram counts the same)
        const char* e = getenv("BLISSGPU_OCCURRENCE_LDS");
        {
            Prof p(c, KX_KNN_OCCURRENCE);
            launch_knn_occurrence(d_idx, q * k, (uint32_t)n, d_count, c->pl_sync.p + 3, e && e[0] == '1', c->n_cus, c->stream);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&flag, c->pl_sync.p + 3, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flag) return fail(BLISSGPU_ERR_INVALID, who, "idx entries must be < n or 0xFFFFFFFF");
    return BLISSGPU_OK;
}

int blissgpu_knn_occurrence(const uint32_t* idx, uint64_t q, uint32_t k, uint64_t n, uint32_t* count) {
    const char* who = "blissgpu_knn_occurrence";
    int rc = occurrence_args_ok(who, idx, q, k, n, count);
    if (rc) return rc;
    const uint64_t entries = q * k;
    for (uint64_t e = 0; e < entries; e++)
        if (idx[e] != 0xFFFFFFFFu && idx[e] >= n) return fail(BLISSGPU_ERR_INVALID, who, "idx entries must be < n or 0xFFFFFFFF");
    if (n == 0) return BLISSGPU_OK;
    if (q == 0) {  // nothing to count: no device is touched
        memset(count, 0, n * sizeof(uint32_t));
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    rc = c->st_idx.ensure(entries + n);
    if (rc) return rc;
    HostStage s{c, "knn_occurrence"};
    s.up(c->st_idx.p, idx, entries * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc) rc = blissgpu_knn_occurrence_device(c, c->st_idx.p, q, k, n, c->st_idx.p + entries);
    if (!rc) s.down(count, c->st_idx.p + entries, n * sizeof(uint32_t));
    return s.finish(rc);
}

// ---- k-means of a library: Lloyd's algorithm with the all-pairs kernel's distances, ties to the lower centre, sequential f32
// means and empty clusters that keep their centre (kernels_kmeans.hip); labels, row lists and centres stay on the device ----
// everything that can be said about the arguments without a device (both forms check it BEFORE the device is touched)
static int kmeans_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, const void* init, uint32_t k, int metric,
                          const float* M, const void* labels, const void* centroids, const void* n_iter, const void* converged) {
    if (k == 0 || k > BLISSGPU_KMEANS_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KMEANS_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric == BLISSGPU_METRIC_COSINE) return fail(BLISSGPU_ERR_INVALID, who, "cosine: a mean does not minimise it");
    if (metric != BLISSGPU_METRIC_EUCLIDEAN && metric != BLISSGPU_METRIC_MAHALANOBIS) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 songs");
    if (n && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (!init) return fail(BLISSGPU_ERR_INVALID, who, "init is NULL");
    if (n && !labels) return fail(BLISSGPU_ERR_INVALID, who, "labels is NULL");
    if (!centroids) return fail(BLISSGPU_ERR_INVALID, who, "centroids is NULL");
    if (!n_iter || !converged) return fail(BLISSGPU_ERR_INVALID, who, "n_iter / converged is NULL");
    return BLISSGPU_OK;
}

int blissgpu_kmeans_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const float* d_init, uint32_t k, int metric,
                           const float* d_M, uint32_t max_iter, uint32_t* d_labels, float* d_dist, float* d_centroids,
                           uint32_t* d_sizes, uint32_t* n_iter, int32_t* converged) {
    const char* who = "blissgpu_kmeans_device";
    int rc = kmeans_args_ok(who, d_x, n, d, d_init, k, metric, d_M, d_labels, d_centroids, n_iter, converged);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    CTX_ENTER(c, who);
    const size_t cent_bytes = (size_t)k * d * sizeof(float);
    if (n == 0) {  // no song: no assignment, no update
        if (d_centroids != d_init) HIP_TRY(hipMemcpyAsync(d_centroids, d_init, cent_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (d_sizes) HIP_TRY(hipMemsetAsync(d_sizes, 0, (size_t)k * sizeof(uint32_t), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *n_iter = 0;
        *converged = 1;
        return BLISSGPU_OK;
    }
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // workspace, O(n + K d + chunks x K): flags u32[4] ([0] labels that moved, [1] NaN) | hist u32[K][W] | scan totals | arow_off
    // u32[K + 1] | arow u32[n] | centres f32[2][K][d]
    const KmeansPlan plan = kmeans_plan(n, k, c->n_cus);
    LabelSort sort(plan, k, n);
    const size_t o_cent = sort.end, words = o_cent + 2 * (size_t)k * d;
    rc = c->km_ws.ensure(words * sizeof(uint32_t));
    if (rc) return rc;
    uint32_t* w = reinterpret_cast<uint32_t*>(c->km_ws.p);
    sort.bind(w);
    uint32_t *flags = sort.flags, *arow_off = sort.arow_off;
    float* cent[2] = {reinterpret_cast<float*>(w + o_cent), reinterpret_cast<float*>(w + o_cent) + (size_t)k * d};
    const AlbumTables tables{nullptr, arow_off, sort.arow, nullptr, nullptr, nullptr, nullptr, nullptr, k, 0u, 0u};
    const size_t zero_bytes = sort.zero_words() * sizeof(uint32_t);  // the flags and the histograms: one memset
    HIP_TRY(hipMemcpyAsync(cent[0], d_init, cent_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_labels, 0xFF, (size_t)n * sizeof(uint32_t), c->stream));  // L_-1: no label
    uint32_t t = 0;
    int cur = 0, conv = 0;
    c->km_loop_copies = c->km_loop_bytes = 0;
    for (;; t++) {
        HIP_TRY(hipMemsetAsync(w, 0, zero_bytes, c->stream));
        {
            Prof p(c, KX_KMEANS_ASSIGN);
            launch_kmeans_assign(d_x, (uint32_t)n, cent[cur], k, d, metric, d_M, diag, plan, d_labels, d_dist, flags, flags + 1, c->stream);
        }
        HIP_TRY(hipGetLastError());
        // the one word pair the host reads per iteration
        uint32_t h_flags[2];
        if ((rc = read_flags(c, flags, 2, h_flags))) return rc;
        c->km_loop_copies++;
        c->km_loop_bytes += sizeof(h_flags);
        if (h_flags[1]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
        if (h_flags[0] == 0) { conv = 1; break; }
        if (t == max_iter) break;
        sort.launch(c, d_labels);
        { Prof p(c, KX_SEGMENT_MEAN); launch_segment_mean(d_x, nullptr, d, tables, cent[cur ^ 1], nullptr, nullptr, c->stream); }
        { Prof p(c, KX_KMEANS_SELECT); launch_kmeans_select(cent[cur], cent[cur ^ 1], arow_off, k, d, nullptr, c->stream); }
        HIP_TRY(hipGetLastError());
        cur ^= 1;
    }
    if (d_sizes) {
        // converged after an update: the labels are those the last sort saw; otherwise they moved since (or were never sorted)
        if (!conv || t == 0) {
            HIP_TRY(hipMemsetAsync(w, 0, zero_bytes, c->stream));
            sort.launch(c, d_labels, false);  // (the sizes need the offsets only)
        }
        { Prof p(c, KX_KMEANS_SELECT); launch_kmeans_select(nullptr, nullptr, arow_off, k, d, d_sizes, c->stream); }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(d_centroids, cent[cur], cent_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_iter = t;
    *converged = conv;
    return BLISSGPU_OK;
}

int blissgpu_kmeans(const float* x, uint64_t n, uint32_t d, const float* init, uint32_t k, int metric, const float* M,
                    uint32_t max_iter, uint32_t* labels, float* dist, float* centroids, uint32_t* sizes, uint32_t* n_iter,
                    int32_t* converged) {
    const char* who = "blissgpu_kmeans";
    int rc = kmeans_args_ok(who, x, n, d, init, k, metric, M, labels, centroids, n_iter, converged);
    if (rc) return rc;
    if (n == 0) {  // no song: nothing for a device to do
        memmove(centroids, init, (size_t)k * d * sizeof(float));
        if (sizes) memset(sizes, 0, (size_t)k * sizeof(uint32_t));
        *n_iter = 0;
        *converged = 1;
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const size_t cent_floats = (size_t)k * d;
    const float* dM = nullptr;
    rc = c->st_b.ensure(n * d);
    if (!rc) rc = c->st_a.ensure(2 * cent_floats);  // the initial centres | the result
    if (!rc) rc = c->st_idx.ensure(n + k);          // labels | sizes
    if (!rc && dist) rc = c->st_dist.ensure(n);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    float* d_cent = c->st_a.p + cent_floats;
    uint32_t *d_labels = c->st_idx.p, *d_sizes = sizes ? c->st_idx.p + n : nullptr;
    HostStage s{c, "kmeans"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(c->st_a.p, init, cent_floats * sizeof(float));
    rc = s.uploaded();
    if (!rc)
        rc = blissgpu_kmeans_device(c, c->st_b.p, n, d, c->st_a.p, k, metric, dM, max_iter, d_labels, dist ? c->st_dist.p : nullptr,
                                    d_cent, d_sizes, n_iter, converged);
    if (!rc) {
        s.down(labels, d_labels, n * sizeof(uint32_t));
        s.down(dist, c->st_dist.p, n * sizeof(float));
        s.down(centroids, d_cent, cent_floats * sizeof(float));
        s.down(sizes, d_sizes, (size_t)k * sizeof(uint32_t));
    }
    return s.finish(rc);
}

// ---- the silhouette of a labelling: the k-means sort of the labels, then the all-pairs sums per (song, cluster) and the scores
// (kernels_silhouette.hip); no distance matrix, the host reads one pair of words ----
// everything that can be said about the scalar arguments and the pointers without a device; *q_eff = the scored songs
static int silhouette_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, const void* labels, uint32_t k, int metric,
                              const float* M, const void* rows, uint64_t q, const void* s, uint64_t* q_eff) {
    if (k == 0 || k > BLISSGPU_KMEANS_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KMEANS_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric == BLISSGPU_METRIC_COSINE) return fail(BLISSGPU_ERR_INVALID, who, "cosine: not a metric the clusters were formed with");
    if (metric != BLISSGPU_METRIC_EUCLIDEAN && metric != BLISSGPU_METRIC_MAHALANOBIS) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 songs");
    *q_eff = rows ? q : n;
    if (*q_eff >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "q must be below 2^32 - 1 songs");
    if (n && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (n && !labels) return fail(BLISSGPU_ERR_INVALID, who, "labels is NULL");
    if (n && *q_eff && !s) return fail(BLISSGPU_ERR_INVALID, who, "s is NULL");
    return BLISSGPU_OK;
}

int blissgpu_silhouette_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const uint32_t* d_labels, uint32_t k,
                               int metric, const float* d_M, const uint32_t* d_rows, uint64_t q, uint32_t col_groups, float* d_s,
                               double* d_a, double* d_b, uint32_t* d_neighbour, uint32_t* d_sizes) {
    const char* who = "blissgpu_silhouette_device";
    int rc = silhouette_args_ok(who, d_x, n, d, d_labels, k, metric, d_M, d_rows, q, d_s, &q);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    CTX_ENTER(c, who);
    if (n == 0) {  // no song: every cluster is empty, nothing is scored
        if (d_sizes) HIP_TRY(hipMemsetAsync(d_sizes, 0, (size_t)k * sizeof(uint32_t), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return BLISSGPU_OK;
    }
    if (q == 0) return BLISSGPU_OK;
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // workspace, O(n + chunks x K + q Y): flags u32[4] ([0] NaN, [1] SIL_ERR_*) | hist u32[K][W] | scan totals | arow_off u32[K + 1]
    // | arow u32[n] | (8-byte aligned) own sums f64[Y][q] | best quotients f64[Y][q] | their clusters u32[Y][q]: 20 q Y bytes
    LabelSort sort(kmeans_plan(n, k, c->n_cus), k, n);
    const SilhouettePlan plan = silhouette_plan(q, k, c->n_cus, col_groups);
    const size_t qy = (size_t)q * plan.Y;
    const size_t o_part = (sort.end + 1) & ~(size_t)1, words = o_part + 5 * qy;
    rc = c->sil_ws.ensure(words * sizeof(uint32_t));
    if (rc) return rc;
    uint32_t* w = reinterpret_cast<uint32_t*>(c->sil_ws.p);
    sort.bind(w);
    uint32_t* flags = sort.flags;
    double* part = reinterpret_cast<double*>(w + o_part);
    SilhouetteArgs a{};
    a.X = d_x; a.labels = d_labels; a.arow_off = sort.arow_off; a.arow = sort.arow; a.rows = d_rows; a.M = d_M;
    a.n = (uint32_t)n; a.K = k; a.q = (uint32_t)q; a.Y = plan.Y; a.d = d; a.metric = metric;
    a.ws_own = part; a.ws_best_q = part + qy; a.ws_best_i = reinterpret_cast<uint32_t*>(part + 2 * qy);
    a.flags = flags; a.s = d_s; a.a = d_a; a.b = d_b; a.neighbour = d_neighbour; a.sizes = d_sizes;
    HIP_TRY(hipMemsetAsync(w, 0, sort.zero_words() * sizeof(uint32_t), c->stream));  // the flags and the histograms
    sort.launch(c, d_labels);
    { Prof p(c, KX_SILHOUETTE_SCAN); launch_silhouette_scan(a, diag, plan, c->stream); }
    { Prof p(c, KX_SILHOUETTE_FINISH); launch_silhouette_finish(a, c->stream); }
    HIP_TRY(hipGetLastError());
    // the one synchronisation: the NaN word and the data-dependent errors
    uint32_t h_flags[2];
    if ((rc = read_flags(c, flags, 2, h_flags))) return rc;
    if (h_flags[1] & SIL_ERR_LABEL) return fail(BLISSGPU_ERR_INVALID, who, "a label is >= k");
    if (h_flags[1] & SIL_ERR_ROW) return fail(BLISSGPU_ERR_INVALID, who, "a rows entry is >= n");
    if (h_flags[1] & SIL_ERR_CLUSTERS) return fail(BLISSGPU_ERR_INVALID, who, "fewer than two non-empty clusters");
    if (h_flags[0]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

int blissgpu_silhouette(const float* x, uint64_t n, uint32_t d, const uint32_t* labels, uint32_t k, int metric, const float* M,
                        const uint32_t* rows, uint64_t q, uint32_t col_groups, float* s, double* a, double* b, uint32_t* neighbour,
                        uint32_t* sizes) {
    const char* who = "blissgpu_silhouette";
    int rc = silhouette_args_ok(who, x, n, d, labels, k, metric, M, rows, q, s, &q);
    if (rc) return rc;
    if (n == 0) {  // no song: nothing for a device to do
        if (sizes) memset(sizes, 0, (size_t)k * sizeof(uint32_t));
        return BLISSGPU_OK;
    }
    if (q == 0) return BLISSGPU_OK;
    // labels and rows are host memory: what the device form finds after its sort is found here, before the device is touched
    {
        std::vector<uint8_t> seen(k, 0);
        uint32_t distinct = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (labels[i] >= k) return fail(BLISSGPU_ERR_INVALID, who, "a label is >= k");
            if (!seen[labels[i]]) { seen[labels[i]] = 1; distinct++; }
        }
        if (distinct < 2) return fail(BLISSGPU_ERR_INVALID, who, "fewer than two non-empty clusters");
        if (rows)
            for (uint64_t p = 0; p < q; p++)
                if (rows[p] >= n) return fail(BLISSGPU_ERR_INVALID, who, "a rows entry is >= n");
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const float* dM = nullptr;
    rc = c->st_b.ensure(n * d);
    if (!rc) rc = c->st_idx.ensure(n + 2 * q + k);  // labels | rows | neighbour | sizes
    if (!rc) rc = c->st_dist.ensure(q);
    if (!rc) rc = c->st_out.ensure(2 * q * sizeof(double));  // a | b
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    uint32_t *d_labels = c->st_idx.p, *d_rows = rows ? c->st_idx.p + n : nullptr, *d_nb = c->st_idx.p + n + q,
             *d_sizes = c->st_idx.p + n + 2 * q;
    double *d_a = reinterpret_cast<double*>(c->st_out.p), *d_b = d_a + q;
    HostStage st{c, "silhouette"};
    st.up(c->st_b.p, x, n * d * sizeof(float));
    st.up(d_labels, labels, n * sizeof(uint32_t));
    st.up(d_rows, rows, q * sizeof(uint32_t));
    rc = st.uploaded();
    if (!rc)
        rc = blissgpu_silhouette_device(c, c->st_b.p, n, d, d_labels, k, metric, dM, d_rows, q, col_groups, c->st_dist.p, d_a, d_b,
                                        d_nb, d_sizes);
    if (!rc) {
        st.down(s, c->st_dist.p, q * sizeof(float));
        st.down(a, d_a, q * sizeof(double));
        st.down(b, d_b, q * sizeof(double));
        st.down(neighbour, d_nb, q * sizeof(uint32_t));
        st.down(sizes, d_sizes, (size_t)k * sizeof(uint32_t));
    }
    return st.finish(rc);
}

// ---- group neighbours: the k-means sort of the labels, then per slab of target groups the minima per (song, group) and their
// blocked sums, then the selection per query row (kernels_chamfer.hip); no distance matrix, the host reads one pair of words ----
// everything that can be said about the scalar arguments and the pointers without a device; *q_eff = the rows to answer
static int neighbours_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, const void* labels, uint32_t k, int metric,
                              const float* M, const void* queries, uint64_t q, uint32_t t, int mode, const void* idx, const void* dist,
                              uint64_t* q_eff) {
    if (k == 0 || k > BLISSGPU_KMEANS_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KMEANS_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (t == 0 || t > BLISSGPU_KNN_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "t must be 1 .. BLISSGPU_KNN_MAX_K");
    if (mode != BLISSGPU_GROUPS_SYMMETRIC && mode != BLISSGPU_GROUPS_DIRECTED) return fail(BLISSGPU_ERR_INVALID, who, "unknown mode");
    if (metric == BLISSGPU_METRIC_COSINE) return fail(BLISSGPU_ERR_INVALID, who, "cosine: not a distance a nearest member is defined with");
    if (metric != BLISSGPU_METRIC_EUCLIDEAN && metric != BLISSGPU_METRIC_MAHALANOBIS) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 songs");
    *q_eff = queries ? q : k;
    if (*q_eff >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "q must be below 2^32 - 1 rows");
    if (n && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (n && !labels) return fail(BLISSGPU_ERR_INVALID, who, "labels is NULL");
    if (*q_eff && !idx) return fail(BLISSGPU_ERR_INVALID, who, "idx is NULL");
    if (*q_eff && !dist) return fail(BLISSGPU_ERR_INVALID, who, "dist is NULL");
    return BLISSGPU_OK;
}

int blissgpu_group_neighbours_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const uint32_t* d_labels, uint32_t k,
                                     int metric, const float* d_M, const uint32_t* d_queries, uint64_t q, uint32_t t, int mode,
                                     uint32_t slab_groups, uint32_t* d_idx, double* d_dist, uint32_t* d_sizes, double* d_matrix) {
    const char* who = "blissgpu_group_neighbours_device";
    int rc = neighbours_args_ok(who, d_x, n, d, d_labels, k, metric, d_M, d_queries, q, t, mode, d_idx, d_dist, &q);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    CTX_ENTER(c, who);
    if (q == 0 && !d_sizes && !d_matrix) return BLISSGPU_OK;  // no row to answer and nothing else asked for
    const bool pairs = n && (q || d_matrix);                  // whether any distance is evaluated
    int diag = 0;
    if (int e = pairs ? metric_is_diag(c, d_M, d, metric, &diag) : 0) return e;
    // workspace: flags u32[4] ([0] NaN, [1] CH_ERR_*) | hist u32[K][W] | scan totals | arow_off u32[K + 1] | arow u32[n] | (8-byte
    // aligned) D f64[K][K] | row buffers f64[select grid][K] | minima f32[slab][n]
    LabelSort sort(n ? kmeans_plan(n, k, c->n_cus) : KmeansPlan{}, k, n);
    const size_t o_d = (sort.end + 1) & ~(size_t)1;
    const ChamferPlan plan = chamfer_plan(n, k, q, d_matrix != nullptr, c->n_cus, slab_groups, c->ws_limit, o_d * sizeof(uint32_t));
    if (!plan.fits) return fail(BLISSGPU_ERR_OOM, who, "D [k][k], the row buffers and one slab of minima do not fit the workspace limit");
    rc = c->ch_ws.ensure(plan.bytes);
    if (rc) return rc;
    uint32_t* w = reinterpret_cast<uint32_t*>(c->ch_ws.p);
    sort.bind(w);
    uint32_t* flags = sort.flags;
    ChamferArgs a{};
    a.X = d_x; a.labels = d_labels; a.arow_off = sort.arow_off; a.arow = sort.arow; a.queries = d_queries; a.M = d_M;
    a.n = (uint32_t)n; a.K = k; a.d = d; a.q = (uint32_t)q; a.t = t; a.metric = metric; a.mode = mode;
    a.D = reinterpret_cast<double*>(w + o_d); a.rowbuf = a.D + (size_t)k * k;
    a.minima = reinterpret_cast<float*>(a.rowbuf + (size_t)plan.select_grid * k);
    a.flags = flags; a.idx = d_idx; a.dist = d_dist; a.sizes = d_sizes; a.matrix = d_matrix;
    // the flags and the histograms; without a song the offsets too (every group is empty)
    HIP_TRY(hipMemsetAsync(w, 0, (n ? sort.zero_words() : sort.o_arow) * sizeof(uint32_t), c->stream));
    if (n) sort.launch(c, d_labels);
    if (pairs)
        for (uint32_t s0 = 0; s0 < k; s0 += plan.slab) {
            a.s0 = s0;
            a.s1 = (uint32_t)std::min<uint64_t>(k, (uint64_t)s0 + plan.slab);
            { Prof p(c, KX_CHAMFER_SCAN); launch_chamfer_scan(a, diag, plan, c->n_cus, c->stream); }
            { Prof p(c, KX_CHAMFER_REDUCE); launch_chamfer_reduce(a, c->stream); }
        }
    { Prof p(c, KX_CHAMFER_SELECT); launch_chamfer_select(a, plan, c->stream); }
    HIP_TRY(hipGetLastError());
    // the one synchronisation: the NaN word and the data-dependent errors
    uint32_t h_flags[2];
    if ((rc = read_flags(c, flags, 2, h_flags))) return rc;
    if (h_flags[1] & CH_ERR_LABEL) return fail(BLISSGPU_ERR_INVALID, who, "a label is >= k");
    if (h_flags[1] & CH_ERR_QUERY) return fail(BLISSGPU_ERR_INVALID, who, "a query is >= k");
    if (h_flags[0]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

int blissgpu_group_neighbours(const float* x, uint64_t n, uint32_t d, const uint32_t* labels, uint32_t k, int metric, const float* M,
                              const uint32_t* queries, uint64_t q, uint32_t t, int mode, uint32_t slab_groups, uint32_t* idx,
                              double* dist, uint32_t* sizes, double* matrix) {
    const char* who = "blissgpu_group_neighbours";
    int rc = neighbours_args_ok(who, x, n, d, labels, k, metric, M, queries, q, t, mode, idx, dist, &q);
    if (rc) return rc;
    // labels and queries are host memory: what the device form finds after its sort is found here, before the device is touched
    for (uint64_t i = 0; i < n; i++)
        if (labels[i] >= k) return fail(BLISSGPU_ERR_INVALID, who, "a label is >= k");
    if (queries)
        for (uint64_t g = 0; g < q; g++)
            if (queries[g] >= k) return fail(BLISSGPU_ERR_INVALID, who, "a query is >= k");
    if (n == 0 || (q == 0 && !matrix)) {  // no song, or no row to answer: nothing for a device to do
        if (sizes) {
            memset(sizes, 0, (size_t)k * sizeof(uint32_t));
            for (uint64_t i = 0; i < n; i++) sizes[labels[i]]++;
        }
        if (n == 0) {
            for (uint64_t e = 0; e < q * t; e++) { idx[e] = 0xFFFFFFFFu; dist[e] = INFINITY; }
            if (matrix)
                for (uint64_t e = 0; e < (uint64_t)k * k; e++) matrix[e] = (e / k == e % k) ? 0.0 : (double)INFINITY;
        }
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const float* dM = nullptr;
    const size_t kk = matrix ? (size_t)k * k : 0;
    rc = c->st_b.ensure(n * d);
    if (!rc) rc = c->st_idx.ensure(n + q + q * t + k);  // labels | queries | idx | sizes
    if (!rc) rc = c->st_out.ensure((q * t + kk) * sizeof(double));  // dist | matrix
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    uint32_t *d_labels = c->st_idx.p, *d_queries = queries ? c->st_idx.p + n : nullptr, *d_idx = c->st_idx.p + n + q,
             *d_sizes = c->st_idx.p + n + q + q * t;
    double *d_dist = reinterpret_cast<double*>(c->st_out.p), *d_matrix = matrix ? d_dist + q * t : nullptr;
    HostStage s{c, "group_neighbours"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(d_labels, labels, n * sizeof(uint32_t));
    s.up(d_queries, queries, q * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc)
        rc = blissgpu_group_neighbours_device(c, c->st_b.p, n, d, d_labels, k, metric, dM, d_queries, q, t, mode, slab_groups, d_idx,
                                              d_dist, sizes ? d_sizes : nullptr, d_matrix);
    if (!rc) {
        s.down(idx, d_idx, q * t * sizeof(uint32_t));
        s.down(dist, d_dist, q * t * sizeof(double));
        s.down(sizes, d_sizes, (size_t)k * sizeof(uint32_t));
        s.down(matrix, d_matrix, kk * sizeof(double));
    }
    return s.finish(rc);
}

// ---- the minimum spanning tree: Boruvka's rounds, each one scan and one pick on the device (kernels_mst.hip) and the merge on
// the host (mst_merge.hpp); no distance matrix, the host reads one pair of words and one pick per component per round ----
// everything that can be said about the scalar arguments and the pointers without a device
static int mst_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, int metric, const float* M, const void* eu, const void* ev,
                       const void* ew) {
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric == BLISSGPU_METRIC_COSINE) return fail(BLISSGPU_ERR_INVALID, who, "cosine: not a distance a spanning tree is defined with");
    if (metric != BLISSGPU_METRIC_EUCLIDEAN && metric != BLISSGPU_METRIC_MAHALANOBIS) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 songs");
    if (n >= 2 && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (n >= 2 && !eu) return fail(BLISSGPU_ERR_INVALID, who, "edge_u is NULL");
    if (n >= 2 && !ev) return fail(BLISSGPU_ERR_INVALID, who, "edge_v is NULL");
    if (n >= 2 && !ew) return fail(BLISSGPU_ERR_INVALID, who, "edge_w is NULL");
    return BLISSGPU_OK;
}

// the rounds on device pointers; the sorted edges arrive in `out` (host memory)
static int mst_run(blissgpu_ctx* c, const char* who, const float* d_x, uint64_t n, uint32_t d, int metric, const float* d_M,
                   const float* d_core, MstState& st) {
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // (for the tests and the bench tool: no bit of the result depends on either)
    uint32_t col_groups = 0, skip = 1;
    if (const char* e = getenv("BLISSGPU_MST_COL_GROUPS")) col_groups = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 65535ul);
    if (const char* e = getenv("BLISSGPU_MST_SKIP")) skip = e[0] != '0';
    const bool trace = getenv("BLISSGPU_MST_TRACE") != nullptr;
    const MstPlan plan = mst_plan(n, c->n_cus, col_groups, c->ws_limit);
    if (!plan.fits) return fail(BLISSGPU_ERR_OOM, who, "the order, the picks and the column groups' winners do not fit the workspace limit");
    int rc = c->ms_ws.ensure(plan.bytes);
    if (rc) return rc;
    uint32_t* w = reinterpret_cast<uint32_t*>(c->ms_ws.p);
    const size_t o_order = 4, o_cpos = o_order + n, o_cw = o_cpos + n, o_pw = o_cw + n, o_pj = o_pw + (size_t)plan.Y * n,
                 o_uv = (o_pj + (size_t)plan.Y * n + 1) & ~(size_t)1;
    MstArgs a{};
    a.X = d_x; a.M = d_M; a.core = d_core; a.order = w + o_order; a.cpos = w + o_cpos;
    a.n = (uint32_t)n; a.d = d; a.metric = metric; a.Y = plan.Y; a.skip = skip;
    a.part_w = w + o_pw; a.part_j = w + o_pj; a.comp_w = w + o_cw; a.comp_uv = reinterpret_cast<unsigned long long*>(w + o_uv);
    a.flags = w;
    int err = BLISSGPU_OK;  // what the pick below failed with
    auto pick = [&](MstState& s, uint32_t* pw, uint64_t* puv) -> int {
        auto hip = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && !err) err = fail(BLISSGPU_ERR_HIP, what, hipGetErrorString(e));
            return e == hipSuccess;
        };
        const auto t_begin = std::chrono::steady_clock::now();
        a.comps = s.comps;
        if (!hip(hipMemsetAsync(w, 0, 4 * sizeof(uint32_t), c->stream), "hipMemsetAsync(mst flags)")) return -1;
        if (!hip(hipMemcpyAsync(w + o_order, s.order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(mst order)")) return -1;
        if (!hip(hipMemcpyAsync(w + o_cpos, s.cpos.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(mst components)")) return -1;
        if (!hip(hipMemsetAsync(a.comp_w, 0xFF, (size_t)s.comps * sizeof(uint32_t), c->stream), "hipMemsetAsync(mst picks)")) return -1;
        if (!hip(hipMemsetAsync(a.comp_uv, 0xFF, (size_t)s.comps * sizeof(uint64_t), c->stream), "hipMemsetAsync(mst picks)")) return -1;
        double scan_ms = 0.0;
        if (trace) (void)hipStreamSynchronize(c->stream);  // (tracing only: the scan between two synchronisations of its own)
        const auto t_scan = std::chrono::steady_clock::now();
        { Prof p(c, KX_MST_SCAN); launch_mst_scan(a, diag, plan, c->stream); }
        if (trace) {
            (void)hipStreamSynchronize(c->stream);
            scan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_scan).count();
        }
        { Prof p(c, KX_MST_PICK); launch_mst_pick(a, 0u, plan, c->stream); }
        { Prof p(c, KX_MST_PICK); launch_mst_pick(a, 1u, plan, c->stream); }
        if (!hip(hipGetLastError(), "mst launch")) return -1;
        uint32_t h_flags[2] = {0, 0};
        if (!hip(hipMemcpyAsync(h_flags, w, sizeof(h_flags), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(mst flags)")) return -1;
        if (!hip(hipMemcpyAsync(pw, a.comp_w, (size_t)s.comps * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(mst picks)")) return -1;
        if (!hip(hipMemcpyAsync(puv, a.comp_uv, (size_t)s.comps * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(mst picks)")) return -1;
        if (!hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(mst)")) return -1;
        if (trace) {
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
            fprintf(stderr, "blissgpu_mst round %u: %u components, scan %.3f ms, round %.3f ms (copies and picks included)\n", s.rounds + 1u,
                    s.comps, scan_ms, ms);
        }
        if (h_flags[1]) { err = fail(BLISSGPU_ERR_INVALID, who, "core holds a NaN or a negative value"); return -1; }
        if (h_flags[0]) { err = fail(BLISSGPU_ERR_INVALID, who, "NaN distance (a NaN feature, or an M that is not positive semi-definite)"); return -1; }
        return 0;
    };
    const auto t0 = std::chrono::steady_clock::now();
    const int m = mst_boruvka(st, (uint32_t)n, pick);
    if (trace)
        fprintf(stderr, "blissgpu_mst: %u rounds, %.3f ms in all (the rounds and the host's merges between them)\n", st.rounds,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (m == -1) return err;
    if (m == MST_TOO_MANY_ROUNDS) return fail(BLISSGPU_ERR_INTERNAL, who, "more than 64 rounds: the components stopped merging");
    if (m != MST_OK || st.edges.size() != (size_t)n - 1) return fail(BLISSGPU_ERR_INTERNAL, who, "a component picked an edge that does not leave it");
    return BLISSGPU_OK;
}

int blissgpu_mst_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, int metric, const float* d_M, const float* d_core,
                        uint32_t* d_edge_u, uint32_t* d_edge_v, float* d_edge_w, uint32_t* rounds) {
    const char* who = "blissgpu_mst_device";
    int rc = mst_args_ok(who, d_x, n, d, metric, d_M, d_edge_u, d_edge_v, d_edge_w);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (rounds) *rounds = 0;
    if (n <= 1) return BLISSGPU_OK;  // no edge: no device is touched
    CTX_ENTER(c, who);
    MstState st;
    rc = mst_run(c, who, d_x, n, d, metric, d_M, d_core, st);
    if (rc) return rc;
    const size_t m = st.edges.size();
    std::vector<uint32_t> out(3 * m);
    for (size_t e = 0; e < m; e++) { out[e] = st.edges[e].u; out[m + e] = st.edges[e].v; out[2 * m + e] = st.edges[e].w; }
    HIP_TRY(hipMemcpyAsync(d_edge_u, out.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_edge_v, out.data() + m, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_edge_w, out.data() + 2 * m, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (rounds) *rounds = st.rounds;
    return BLISSGPU_OK;
}

int blissgpu_mst(const float* x, uint64_t n, uint32_t d, int metric, const float* M, const float* core, uint32_t* edge_u,
                 uint32_t* edge_v, float* edge_w, uint32_t* rounds) {
    const char* who = "blissgpu_mst";
    int rc = mst_args_ok(who, x, n, d, metric, M, edge_u, edge_v, edge_w);
    if (rc) return rc;
    if (rounds) *rounds = 0;
    if (n <= 1) return BLISSGPU_OK;  // no edge: nothing for a device to do
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const float* dM = nullptr;
    rc = c->st_b.ensure(n * d + (core ? n : 0));
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    float* d_core = core ? c->st_b.p + n * d : nullptr;
    HostStage s{c, "mst"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(d_core, core, n * sizeof(float));
    rc = s.uploaded();
    MstState st;
    if (!rc) rc = mst_run(c, who, c->st_b.p, n, d, metric, dM, d_core, st);
    if ((rc = s.finish(rc))) return rc;  // (the edges are host memory: nothing to copy back)
    for (size_t k = 0; k < st.edges.size(); k++) {
        edge_u[k] = st.edges[k].u;
        edge_v[k] = st.edges[k].v;
        memcpy(edge_w + k, &st.edges[k].w, sizeof(float));
    }
    if (rounds) *rounds = st.rounds;
    return BLISSGPU_OK;
}

// ---- Ward clustering: per round one all-pairs scan of the current centroids and one join on the device (kernels_ward.hip), the
// mutual pairs and the plan on the host (ward_merge.hpp); no distance matrix, the host reads one key per position per round and
// sends the plan.  Host-pointer forms only: the cores below take the context and device pointers ----
constexpr uint64_t WARD_MAX_SONGS = 1ull << 24;  // every size and every sum of two sizes is exact in f32 below this

// everything that can be said about the scalar arguments without a device
static int ward_scalars_ok(const char* who, uint64_t n, uint32_t d, int metric, const float* M) {
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric == BLISSGPU_METRIC_COSINE) return fail(BLISSGPU_ERR_INVALID, who, "cosine: Ward's cost is the growth of a sum of squares, which cosine does not give");
    if (metric != BLISSGPU_METRIC_EUCLIDEAN && metric != BLISSGPU_METRIC_MAHALANOBIS) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= WARD_MAX_SONGS) return fail(BLISSGPU_ERR_INVALID, who, "n (m) and the sum of the sizes must be below 2^24");
    return BLISSGPU_OK;
}

// (for the tests and the bench tool: no bit of the result depends on any of them)
// The filter in front of the root pays from about 10^4 positions on (per round 0.425 against 0.425 ms at
// m = 10 186, 0.83 against 0.89 ms at m = 15 497, and slightly slower below), so every scan chooses by its own m
constexpr uint32_t WARD_FILTER_MIN_M = 12288;
struct WardSwitches {
    uint32_t col_groups = 0;
    int filter = -1;  // -1: by m; 0 / 1: BLISSGPU_WARD_FILTER says
    bool trace = false;
    WardSwitches() {
        if (const char* e = getenv("BLISSGPU_WARD_COL_GROUPS")) col_groups = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 65535ul);
        if (const char* e = getenv("BLISSGPU_WARD_FILTER")) filter = e[0] != '0';
        trace = getenv("BLISSGPU_WARD_TRACE") != nullptr;
    }
    bool filter_at(uint32_t m) const { return filter < 0 ? m >= WARD_FILTER_MIN_M : filter != 0; }
};

// the workspace: flags u32[4] | best u64[n] | and for the tree rows f32[n][d] | size u32[2][n] | low u32[2][n] | plan u32[n][2]
struct WardWs {
    uint32_t* flags;
    unsigned long long* best;
    float* rows;
    uint32_t *size[2], *low[2], *plan;
    uint64_t* host;  // page-locked, u64 [2 + n]: what a round brings back -- the flags, then the best keys
};
static int ward_workspace(blissgpu_ctx* c, const char* who, uint64_t n, uint32_t d, bool tree, WardWs* ws) {
    const uint64_t bytes = 16 + 8 * n + (tree ? 4 * n * d + 24 * n : 0);
    if (bytes > c->ws_limit) return fail(BLISSGPU_ERR_OOM, who, "the rows, the sizes, the plan and the best keys do not fit the workspace limit");
    int rc = c->wd_ws.ensure(bytes);
    if (!rc) rc = c->wd_host.ensure(2 + n);
    if (rc) return rc;
    ws->host = c->wd_host.p;
    uint8_t* b = c->wd_ws.p;
    ws->flags = reinterpret_cast<uint32_t*>(b);
    ws->best = reinterpret_cast<unsigned long long*>(b + 16);
    ws->rows = reinterpret_cast<float*>(b + 16 + 8 * n);
    uint32_t* w = reinterpret_cast<uint32_t*>(b + 16 + 8 * n + 4 * n * d);
    ws->size[0] = w; ws->size[1] = w + n; ws->low[0] = w + 2 * n; ws->low[1] = w + 3 * n; ws->plan = w + 4 * n;
    return BLISSGPU_OK;
}

// one scan: every position's nearest other position.  d_low / d_size may be NULL (X[p], 1).  The smallest (cost bits << 32 |
// p XOR j) per position arrives in ws.host[2 .. 2 + m); the stream is synchronised when this returns.  fresh: the flags and the
// best keys are reset here (a call's first scan; after that the join has reset the keys, and a raised flag ends the call)
static int ward_nearest_core(blissgpu_ctx* c, const char* who, const float* d_rows, const uint32_t* d_low, const uint32_t* d_size, uint32_t m,
                             uint32_t slots, uint32_t d, int metric, const float* d_M, int diag, const WardSwitches& sw, const WardWs& ws,
                             bool fresh, double* scan_ms) {
    const WardPlan plan = ward_plan(m, c->n_cus, sw.col_groups);
    WardArgs a{};
    a.X = d_rows; a.M = d_M; a.low = d_low; a.size = d_size; a.m = m; a.d = d; a.slots = slots; a.metric = metric; a.Y = plan.Y;
    a.best = ws.best; a.flags = ws.flags;
    if (fresh) {
        HIP_TRY(hipMemsetAsync(ws.flags, 0, 4 * sizeof(uint32_t), c->stream));
        HIP_TRY(hipMemsetAsync(ws.best, 0xFF, (size_t)m * sizeof(uint64_t), c->stream));
    }
    if (sw.trace) (void)hipStreamSynchronize(c->stream);  // (tracing only: the scan between two synchronisations of its own)
    const auto t_scan = std::chrono::steady_clock::now();
    { Prof p(c, KX_WARD_SCAN); launch_ward_scan(a, diag, sw.filter_at(m), plan, c->stream); }
    HIP_TRY(hipGetLastError());
    if (sw.trace) {
        (void)hipStreamSynchronize(c->stream);
        if (scan_ms) *scan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_scan).count();
    }
    // (the flags lie in front of the best keys: one copy brings both)
    HIP_TRY(hipMemcpyAsync(ws.host, ws.flags, 16 + (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((uint32_t)ws.host[0]) return fail(BLISSGPU_ERR_INVALID, who, "NaN cost (a NaN feature, inf - inf, or an M that is not positive semi-definite)");
    return BLISSGPU_OK;
}

// the rounds.  The rows are in ws.rows already (d_x == NULL) or are copied there from d_x; the sorted edges arrive in st
static int ward_core(blissgpu_ctx* c, const char* who, const float* d_x, uint64_t n, uint32_t d, int metric, const float* d_M, const WardWs& ws,
                     WardState& st) {
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    const WardSwitches sw;
    if (d_x) HIP_TRY(hipMemcpyAsync(ws.rows, d_x, n * d * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    {
        std::vector<uint32_t> init(2 * n, 1u);
        for (uint64_t i = 0; i < n; i++) init[n + i] = (uint32_t)i;
        HIP_TRY(hipMemcpyAsync(ws.size[0], init.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(ws.low[0], init.data() + n, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (init goes away)
    }
    int err = BLISSGPU_OK;  // what a step below failed with
    int cur = 0;            // which of the two (size, low) pairs holds the current round
    const uint64_t* keys = ws.host + 2;
    auto t_round = std::chrono::steady_clock::now();
    double scan_ms = 0.0;
    bool round_open = false;  // (tracing only) a round has scanned and its line is not printed yet
    auto trace_round = [&](const WardState& s) {  // s is the state after the round's merge
        if (sw.trace && round_open)
            fprintf(stderr, "%s round %u: %u clusters, %u pairs, scan %.3f ms, round %.3f ms (copies and the join included)\n", who, s.rounds - 1u,
                    s.prev_m, s.prev_m - s.m, scan_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_round).count());
        round_open = false;
    };
    auto nearest = [&](WardState& s, uint32_t* nn, uint32_t* cost) -> int {
        t_round = std::chrono::steady_clock::now();
        round_open = true;
        err = ward_nearest_core(c, who, ws.rows, ws.low[cur], ws.size[cur], s.m, (uint32_t)n, d, metric, d_M, diag, sw, ws, s.rounds == 0, &scan_ms);
        if (err) return -1;
        for (uint32_t p = 0; p < s.m; p++) {
            cost[p] = (uint32_t)(keys[p] >> 32);
            nn[p] = keys[p] == ~0ull ? WARD_NONE : (p ^ (uint32_t)keys[p]);
        }
        return 0;
    };
    auto join = [&](WardState& s) -> int {
        auto hip = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && !err) err = fail(BLISSGPU_ERR_HIP, what, hipGetErrorString(e));
            return e == hipSuccess;
        };
        WardJoinArgs j{};
        j.X = ws.rows; j.plan = ws.plan; j.size = ws.size[cur]; j.low = ws.low[cur]; j.size_out = ws.size[cur ^ 1]; j.low_out = ws.low[cur ^ 1];
        j.m_old = s.prev_m; j.m_new = s.m; j.d = d; j.slots = (uint32_t)n; j.best = ws.best;
        // (the plan is two words per position in the order of WardJoin: p, q)
        static_assert(sizeof(WardJoin) == 2 * sizeof(uint32_t), "the plan is uploaded as it stands");
        if (!hip(hipMemcpyAsync(ws.plan, s.plan.data(), (size_t)s.m * sizeof(WardJoin), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(ward plan)")) return -1;
        { Prof p(c, KX_WARD_JOIN); launch_ward_join(j, c->stream); }
        if (!hip(hipGetLastError(), "ward join launch")) return -1;
        // (no synchronisation here: the plan is host memory that only the next merge rewrites, and the next scan's
        // synchronisation comes before that merge; the caller synchronises before the state goes away)
        cur ^= 1;
        trace_round(s);
        return 0;
    };
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = ward_rounds(st, (uint32_t)n, nearest, join);
    if (rc == WARD_OK) trace_round(st);  // (the last round has no join)
    if (sw.trace)
        fprintf(stderr, "%s: %u rounds, %.3f pairs / n^2, %.3f ms in all (the rounds and the host's merges between them)\n", who, st.rounds,
                (double)st.pairs_scanned / ((double)n * (double)n), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (rc == -1) return err;
    if (rc == WARD_STALLED) return fail(BLISSGPU_ERR_INTERNAL, who, "a round merged nothing: no two positions are each other's nearest");
    if (rc != WARD_OK || st.edges.size() != (size_t)n - 1) return fail(BLISSGPU_ERR_INTERNAL, who, "a position's nearest is no other position");
    return BLISSGPU_OK;
}

int blissgpu_ward_nearest(const float* cc, const uint32_t* size, uint64_t m, uint32_t d, int metric, const float* M, uint32_t* nn, float* cost) {
    const char* who = "blissgpu_ward_nearest";
    int rc = ward_scalars_ok(who, m, d, metric, M);
    if (rc) return rc;
    if (m == 0) return BLISSGPU_OK;  // nothing is touched
    if (m >= 2 && !cc) return fail(BLISSGPU_ERR_INVALID, who, "c is NULL");
    if (!nn) return fail(BLISSGPU_ERR_INVALID, who, "nn is NULL");
    if (!cost) return fail(BLISSGPU_ERR_INVALID, who, "cost is NULL");
    if (size) {
        uint64_t total = 0;
        for (uint64_t p = 0; p < m; p++) {
            if (size[p] == 0) return fail(BLISSGPU_ERR_INVALID, who, "size holds a 0: every cluster has at least one song");
            total += size[p];
        }
        if (total >= WARD_MAX_SONGS) return fail(BLISSGPU_ERR_INVALID, who, "n (m) and the sum of the sizes must be below 2^24");
    }
    if (m == 1) {  // no other position: no device is touched
        nn[0] = WARD_NONE;
        cost[0] = INFINITY;
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const float* dM = nullptr;
    WardWs ws{};
    rc = ward_workspace(c, who, m, d, false, &ws);
    if (!rc) rc = c->st_b.ensure(m * d);
    if (!rc && size) rc = c->st_idx.ensure(m);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    int diag = 0;
    if (int e = metric_is_diag(c, dM, d, metric, &diag)) return e;
    HostStage s{c, "ward_nearest"};
    s.up(c->st_b.p, cc, m * d * sizeof(float));
    if (size) s.up(c->st_idx.p, size, m * sizeof(uint32_t));
    rc = s.uploaded();
    const uint64_t* keys = ws.host + 2;
    const WardSwitches sw;
    if (!rc) rc = ward_nearest_core(c, who, c->st_b.p, nullptr, size ? c->st_idx.p : nullptr, (uint32_t)m, (uint32_t)m, d, metric, dM, diag, sw, ws, true, nullptr);
    if ((rc = s.finish(rc))) return rc;  // (the keys are host memory: nothing to copy back)
    for (uint64_t p = 0; p < m; p++)
        if (keys[p] == ~0ull) return fail(BLISSGPU_ERR_INTERNAL, who, "a position found no other position");
    for (uint64_t p = 0; p < m; p++) {
        const uint32_t cb = (uint32_t)(keys[p] >> 32);
        nn[p] = (uint32_t)p ^ (uint32_t)keys[p];
        memcpy(cost + p, &cb, sizeof(float));
    }
    return BLISSGPU_OK;
}

int blissgpu_ward(const float* x, uint64_t n, uint32_t d, int metric, const float* M, uint32_t* edge_u, uint32_t* edge_v, float* edge_cost,
                  uint32_t* edge_size, uint32_t* edge_round, uint32_t* rounds) {
    const char* who = "blissgpu_ward";
    int rc = ward_scalars_ok(who, n, d, metric, M);
    if (rc) return rc;
    if (n >= 2 && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (n >= 2 && !edge_u) return fail(BLISSGPU_ERR_INVALID, who, "edge_u is NULL");
    if (n >= 2 && !edge_v) return fail(BLISSGPU_ERR_INVALID, who, "edge_v is NULL");
    if (n >= 2 && !edge_cost) return fail(BLISSGPU_ERR_INVALID, who, "edge_cost is NULL");
    if (rounds) *rounds = 0;
    if (n <= 1) return BLISSGPU_OK;  // no edge: nothing for a device to do
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const float* dM = nullptr;
    WardWs ws{};
    rc = ward_workspace(c, who, n, d, true, &ws);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    HostStage s{c, "ward"};
    s.up(ws.rows, x, n * d * sizeof(float));  // (the rows go straight into the copy the joins rewrite)
    rc = s.uploaded();
    WardState st;
    if (!rc) rc = ward_core(c, who, nullptr, n, d, metric, dM, ws, st);
    if ((rc = s.finish(rc))) return rc;  // (the edges are host memory: nothing to copy back)
    for (size_t k = 0; k < st.edges.size(); k++) {
        const WardEdge& e = st.edges[k];
        edge_u[k] = e.u;
        edge_v[k] = e.v;
        memcpy(edge_cost + k, &e.cost, sizeof(float));
        if (edge_size) edge_size[k] = e.size;
        if (edge_round) edge_round[k] = e.round;
    }
    if (rounds) *rounds = st.rounds;
    return BLISSGPU_OK;
}

// ---- k-medoids (PAM): the state by the k-nearest core over the medoids' rows, then per round one all-pairs scan of every
// candidate against every song (kernels_pam.hip); no distance matrix, the host reads one record per round ----
// (for the tests and the bench tool: no bit of the result depends on either)
struct PamSwitches {
    uint32_t col_groups = 0;
    bool trace = false;
    PamSwitches() {
        if (const char* e = getenv("BLISSGPU_PAM_COL_GROUPS")) col_groups = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 65535ul);
        trace = getenv("BLISSGPU_PAM_TRACE") != nullptr;
    }
};

// the workspace, O(n + slab k): the record (32 bytes, then 32 unused) | hist u32[hist_cap] | scan totals u32[tiles_cap + 1] |
// arow_off u32[k + 1] | arow u32[n] | near u32[n] | ismed u32[n] | med u32[k] | d1 f32[n] | d2 f32[n] | the medoids' rows
// f32[k][d] | the state's search: idx u32[n][2], dist f32[n][2] | (8-byte aligned) A f64[slab][k] | B f64[slab][k].  The slab is
// every candidate when that fits the workspace limit, else as many rows as fit (whole wavefronts of 256 where there is room for
// them).  hist_cap / tiles_cap: the largest histogram table and scan-total count among the sorts the call makes -- K = k_lo .. k
// slots (BUILD sorts every K from 1; a scan alone sorts k).  kmeans_plan caps its chunks at 2^21 / K and rounds them to 64
// songs, so K * W is NOT monotone in K: the largest is found by asking the plan of every K, not by asking that of k
struct PamLayout {
    size_t o_hist, o_bsum, o_off, o_arow, o_near, o_ismed, o_med, o_d1, o_d2, o_rows, o_kidx, o_kdist, o_ab;
    uint64_t hist_cap, tiles_cap, fixed, per_row, slab;  // fixed: the bytes in front of A; slab == 0: one candidate's share does not fit
};
static PamLayout pam_layout(uint64_t n, uint32_t d, uint32_t k_lo, uint32_t k, uint64_t q, uint64_t ws_limit) {
    PamLayout L{};
    for (uint32_t K = k_lo; K <= k; K++) {
        const KmeansPlan sort = kmeans_plan(n, K, 0);
        L.hist_cap = std::max<uint64_t>(L.hist_cap, sort.hist_words);
        L.tiles_cap = std::max<uint64_t>(L.tiles_cap, sort.scan_tiles);
    }
    size_t o = 16;
    L.o_hist = o; o += (size_t)L.hist_cap;
    L.o_bsum = o; o += (size_t)L.tiles_cap + 1;
    L.o_off = o; o += (size_t)k + 1;
    L.o_arow = o; o += n;
    L.o_near = o; o += n;
    L.o_ismed = o; o += n;
    L.o_med = o; o += k;
    L.o_d1 = o; o += n;
    L.o_d2 = o; o += n;
    L.o_rows = o; o += (size_t)k * d;
    L.o_kidx = o; o += 2 * n;
    L.o_kdist = o; o += 2 * n;
    L.o_ab = (o + 1) & ~(size_t)1;
    L.fixed = (uint64_t)L.o_ab * sizeof(uint32_t);
    L.per_row = 16ull * k;
    if (L.fixed + L.per_row > ws_limit) return L;
    L.slab = std::min<uint64_t>(std::max<uint64_t>(q, 1), (ws_limit - L.fixed) / L.per_row);
    if (L.slab < q) L.slab = L.slab >= 1024 ? L.slab & ~1023ull : L.slab >= 256 ? L.slab & ~255ull : L.slab;
    return L;
}
struct PamWs {
    PamRecord* rec;
    uint32_t *hist, *bsum, *arow_off, *arow, *near, *ismed, *med, *kidx;
    float *d1, *d2, *medrows, *kdist;
    double *a, *b;
    uint64_t slab, hist_cap, tiles_cap;
    size_t zero_words;  // the record's 16 words: zeroed before a round's first launch
};
static int pam_workspace(blissgpu_ctx* c, const char* who, uint64_t n, uint32_t d, uint32_t k_lo, uint32_t k, uint64_t q, PamWs* ws) {
    const PamLayout L = pam_layout(n, d, k_lo, k, q, c->ws_limit);
    if (L.slab == 0) return fail(BLISSGPU_ERR_OOM, who, "the state and one candidate's sums do not fit the workspace limit");
    int rc = c->pam_ws.ensure(L.fixed + L.slab * L.per_row);
    if (rc) return rc;
    uint32_t* w = reinterpret_cast<uint32_t*>(c->pam_ws.p);
    ws->rec = reinterpret_cast<PamRecord*>(w);
    ws->hist = w + L.o_hist; ws->bsum = w + L.o_bsum; ws->arow_off = w + L.o_off; ws->arow = w + L.o_arow; ws->near = w + L.o_near;
    ws->ismed = w + L.o_ismed; ws->med = w + L.o_med; ws->kidx = w + L.o_kidx;
    ws->d1 = reinterpret_cast<float*>(w + L.o_d1); ws->d2 = reinterpret_cast<float*>(w + L.o_d2);
    ws->medrows = reinterpret_cast<float*>(w + L.o_rows); ws->kdist = reinterpret_cast<float*>(w + L.o_kdist);
    ws->a = reinterpret_cast<double*>(w + L.o_ab); ws->b = ws->a + L.slab * k;
    ws->slab = L.slab; ws->hist_cap = L.hist_cap; ws->tiles_cap = L.tiles_cap;
    ws->zero_words = L.o_hist;
    static_assert(sizeof(PamRecord) == 32, "the record is the workspace's first 32 bytes");
    return BLISSGPU_OK;
}

struct PamPick {  // what the round's winner is taken over
    enum Kind { NONE, BEST, BTOT, A0 } kind = NONE;
    bool skip_medoids = false;
};
struct PamOut {  // where a scan's results go: btot, best, arg on the device, [q]
    double *btot, *best;
    uint32_t* arg;
    double *host_a, *host_b;  // HOST memory [q][K] (either may be NULL): copied back slab by slab through the call's HostStage
};

// one scan over the candidates d_rows[0 .. q) (NULL: every song, q = n) under the state in ws (near, d1, d2) with K slots: the
// sort of near, then per slab of candidates the scan, the fold and -- when asked -- the pick into ws.rec.  The caller has zeroed
// the record.  Nothing is synchronised unless host_a / host_b want a slab's sums before the next overwrites them
static int pam_scan_core(blissgpu_ctx* c, HostStage& s, const char* who, const float* d_x, uint64_t n, uint32_t d, uint32_t K, int metric,
                         const float* d_M, int diag, const uint32_t* d_rows, uint64_t q, const PamSwitches& sw, const PamWs& ws,
                         const PamOut& out, PamPick pick) {
    const KmeansPlan sort = kmeans_plan(n, K, c->n_cus);
    if (sort.hist_words > ws.hist_cap || sort.scan_tiles > ws.tiles_cap)
        return fail(BLISSGPU_ERR_INTERNAL, who, "the sort of the slots needs more than the workspace holds for it");
    HIP_TRY(hipMemsetAsync(ws.hist, 0, (size_t)sort.hist_words * sizeof(uint32_t), c->stream));
    LabelSort slots(sort, K, n);  // (on the tables pam_layout sized for the call's largest K, not on its own words)
    slots.hist = ws.hist; slots.bsum = ws.bsum; slots.arow_off = ws.arow_off; slots.arow = ws.arow;
    slots.launch(c, ws.near);
    HIP_TRY(hipGetLastError());
    for (uint64_t row0 = 0; row0 < q; row0 += ws.slab) {
        const uint64_t qs = std::min<uint64_t>(ws.slab, q - row0);
        const SilhouettePlan plan = silhouette_plan(qs, K, c->n_cus, sw.col_groups);
        PamArgs a{};
        a.X = d_x; a.M = d_M; a.arow_off = ws.arow_off; a.arow = ws.arow; a.rows = d_rows ? d_rows + row0 : nullptr;
        a.d1 = ws.d1; a.d2 = ws.d2; a.n = (uint32_t)n; a.K = K; a.q = (uint32_t)qs; a.row0 = (uint32_t)row0; a.Y = plan.Y; a.d = d;
        a.metric = metric; a.ws_a = ws.a; a.ws_b = ws.b; a.flags = &ws.rec->nan;
        a.btot = out.btot + row0; a.best = out.best + row0; a.arg = out.arg + row0;
        { Prof p(c, KX_PAM_SCAN); launch_pam_scan(a, diag, plan, c->stream); }
        { Prof p(c, KX_PAM_FOLD); launch_pam_fold(a, c->stream); }
        if (pick.kind != PamPick::NONE) {
            const double* val = pick.kind == PamPick::BEST ? a.best : pick.kind == PamPick::BTOT ? a.btot : ws.a;
            Prof p(c, KX_PAM_PICK);
            launch_pam_pick(val, pick.kind == PamPick::A0 ? K : 1u, pick.kind == PamPick::BEST ? a.arg : nullptr, a.rows, a.row0, a.q,
                            pick.skip_medoids ? ws.ismed : nullptr, row0 == 0, ws.rec, c->stream);
        }
        HIP_TRY(hipGetLastError());
        if (out.host_a || out.host_b) {
            const size_t bytes = (size_t)qs * K * sizeof(double);
            if (out.host_a) s.down(out.host_a + row0 * K, ws.a, bytes);
            if (out.host_b) s.down(out.host_b + row0 * K, ws.b, bytes);
            if (int e = s.landed()) return e;  // (the next slab overwrites A and B)
        }
    }
    return BLISSGPU_OK;
}

static int pam_scalars_ok(const char* who, uint64_t n, uint32_t d, uint32_t k, int metric, const float* M) {
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (k == 0 || k > BLISSGPU_KMEANS_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KMEANS_MAX_K");
    if (metric != BLISSGPU_METRIC_EUCLIDEAN && metric != BLISSGPU_METRIC_COSINE && metric != BLISSGPU_METRIC_MAHALANOBIS)
        return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 songs");
    return BLISSGPU_OK;
}

int blissgpu_pam_scan(const float* x, uint64_t n, uint32_t d, const uint32_t* near, const float* d1, const float* d2, uint32_t k, int metric,
                      const float* M, const uint32_t* rows, uint64_t q, double* btot, double* best, uint32_t* arg, double* A, double* B) {
    const char* who = "blissgpu_pam_scan";
    int rc = pam_scalars_ok(who, n, d, k, metric, M);
    if (rc) return rc;
    if (!rows) q = n;
    if (q >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "q must be below 2^32 - 1 candidates");
    if (n == 0 || q == 0) return BLISSGPU_OK;  // nothing to evaluate: nothing is touched
    if (!x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (!near) return fail(BLISSGPU_ERR_INVALID, who, "near is NULL");
    if (!d1) return fail(BLISSGPU_ERR_INVALID, who, "d1 is NULL");
    if (!d2) return fail(BLISSGPU_ERR_INVALID, who, "d2 is NULL");
    if (!btot) return fail(BLISSGPU_ERR_INVALID, who, "btot is NULL");
    if (!best) return fail(BLISSGPU_ERR_INVALID, who, "best is NULL");
    if (!arg) return fail(BLISSGPU_ERR_INVALID, who, "arg is NULL");
    // near, d1, d2 and rows are host memory: what is wrong with them is found here, before the device is touched
    for (uint64_t o = 0; o < n; o++) {
        if (near[o] >= k) return fail(BLISSGPU_ERR_INVALID, who, "a near entry is >= k");
        if (d1[o] != d1[o]) return fail(BLISSGPU_ERR_INVALID, who, "d1 holds a NaN");
        if (d2[o] != d2[o]) return fail(BLISSGPU_ERR_INVALID, who, "d2 holds a NaN");
    }
    if (rows)
        for (uint64_t p = 0; p < q; p++)
            if (rows[p] >= n) return fail(BLISSGPU_ERR_INVALID, who, "a rows entry is >= n");
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const float* dM = nullptr;
    PamWs ws{};
    rc = pam_workspace(c, who, n, d, k, k, q, &ws);
    if (!rc) rc = c->st_b.ensure(n * d);
    if (!rc) rc = c->st_idx.ensure(2 * q);                     // rows | arg
    if (!rc) rc = c->st_out.ensure(2 * q * sizeof(double));    // btot | best
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    int diag = 0;
    if (int e = metric_is_diag(c, dM, d, metric, &diag)) return e;
    uint32_t *d_rows = rows ? c->st_idx.p : nullptr, *d_arg = c->st_idx.p + q;
    double *d_btot = reinterpret_cast<double*>(c->st_out.p), *d_best = d_btot + q;
    HostStage s{c, "pam_scan"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(ws.near, near, n * sizeof(uint32_t));  // (the state goes straight into the workspace)
    s.up(ws.d1, d1, n * sizeof(float));
    s.up(ws.d2, d2, n * sizeof(float));
    s.up(d_rows, rows, q * sizeof(uint32_t));
    rc = s.uploaded();
    const PamSwitches sw;
    auto run = [&]() -> int {
        HIP_TRY(hipMemsetAsync(ws.rec, 0, ws.zero_words * sizeof(uint32_t), c->stream));
        const PamOut out{d_btot, d_best, d_arg, A, B};
        if (int e = pam_scan_core(c, s, who, c->st_b.p, n, d, k, metric, dM, diag, d_rows, q, sw, ws, out, PamPick{})) return e;
        uint32_t nan_word = 0;
        if (int e = read_flags(c, &ws.rec->nan, 1, &nan_word)) return e;
        if (nan_word) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
        return BLISSGPU_OK;
    };
    if (!rc) rc = run();
    if (!rc) {
        s.down(btot, d_btot, q * sizeof(double));
        s.down(best, d_best, q * sizeof(double));
        s.down(arg, d_arg, q * sizeof(uint32_t));
    }
    return s.finish(rc);
}

int blissgpu_kmedoids(const float* x, uint64_t n, uint32_t d, uint32_t k, int metric, const float* M, const uint32_t* init, uint32_t max_swaps,
                      uint32_t* medoids, uint32_t* labels, float* dist, uint32_t* sizes, double* td_trace, uint32_t* n_swaps,
                      int32_t* converged) {
    const char* who = "blissgpu_kmedoids";
    int rc = pam_scalars_ok(who, n, d, k, metric, M);
    if (rc) return rc;
    if (!n_swaps) return fail(BLISSGPU_ERR_INVALID, who, "n_swaps is NULL");
    if (!converged) return fail(BLISSGPU_ERR_INVALID, who, "converged is NULL");
    if (n == 0) {  // no song: nothing for a device to do
        *n_swaps = 0;
        *converged = 1;
        return BLISSGPU_OK;
    }
    if (k > n) return fail(BLISSGPU_ERR_INVALID, who, "k must be at most n: the medoids are distinct songs");
    if (!x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (!medoids) return fail(BLISSGPU_ERR_INVALID, who, "medoids is NULL");
    if (!labels) return fail(BLISSGPU_ERR_INVALID, who, "labels is NULL");
    if (!td_trace) return fail(BLISSGPU_ERR_INVALID, who, "td_trace is NULL");
    if (init) {
        std::vector<uint32_t> sorted(init, init + k);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() >= n) return fail(BLISSGPU_ERR_INVALID, who, "an init entry is >= n");
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(BLISSGPU_ERR_INVALID, who, "init holds a song twice");
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const float* dM = nullptr;
    PamWs ws{};
    rc = pam_workspace(c, who, n, d, init ? k : 1u, k, n, &ws);
    if (!rc) rc = c->st_b.ensure(n * d);
    if (!rc) rc = c->st_idx.ensure(n);                        // arg
    if (!rc) rc = c->st_out.ensure(2 * n * sizeof(double));   // btot | best
    if (!rc) rc = c->pl_tmp.ensure((size_t)knn_plan(n, k, 2, c->n_cus).part_keys * sizeof(unsigned long long));
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    int diag = 0;
    if (int e = metric_is_diag(c, dM, d, metric, &diag)) return e;
    const float* d_x = c->st_b.p;
    const PamOut out{reinterpret_cast<double*>(c->st_out.p), reinterpret_cast<double*>(c->st_out.p) + n, c->st_idx.p, nullptr, nullptr};
    HostStage s{c, "kmedoids"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(ws.med, init, (size_t)k * sizeof(uint32_t));
    rc = s.uploaded();
    const PamSwitches sw;
    const uint32_t nn = (uint32_t)n;
    PamRecord h{};
    // the record of a round: zeroed before the round's first launch, read after its last
    auto reset = [&]() -> int {
        HIP_TRY(hipMemsetAsync(ws.rec, 0, ws.zero_words * sizeof(uint32_t), c->stream));
        return BLISSGPU_OK;
    };
    auto read = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(&h, ws.rec, sizeof(PamRecord), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (h.nan) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
        return BLISSGPU_OK;
    };
    // the state of the first K medoids: their rows (with a swap or an appended slot applied first), the k-nearest core with k =
    // min(2, K) over them, near / d1 / d2, and TD into the record
    auto state = [&](uint32_t K, uint32_t swap_slot, uint32_t swap_c, bool append, bool mark_all) -> int {
        { Prof p(c, KX_PAM_GATHER); launch_pam_gather(d_x, ws.med, K, d, ws.medrows, swap_slot, swap_c, append, mark_all, ws.ismed, c->stream); }
        const uint32_t kk = K >= 2 ? 2u : 1u;
        const KnnPlan plan = knn_plan(n, K, kk, c->n_cus);
        if (int e = c->pl_tmp.ensure((size_t)plan.part_keys * sizeof(unsigned long long))) return e;
        unsigned long long* part = reinterpret_cast<unsigned long long*>(c->pl_tmp.p);
        { Prof p(c, K_KNN_SCAN); launch_knn_scan(d_x, n, ws.medrows, K, d, metric, dM, diag, nullptr, kk, plan, part, &ws.rec->nan, &ws.rec->bad, c->stream); }
        { Prof p(c, K_KNN_MERGE); launch_knn_merge(part, n, kk, plan, ws.kidx, ws.kdist, c->stream); }
        { Prof p(c, KX_PAM_STATE); launch_pam_state(ws.kidx, ws.kdist, nn, kk, ws.near, ws.d1, ws.d2, c->stream); }
        { Prof p(c, KX_PAM_TD); launch_pam_td(ws.d1, nn, ws.rec, c->stream); }
        HIP_TRY(hipGetLastError());
        return BLISSGPU_OK;
    };
    uint32_t swaps = 0;
    int conv = 0;
    auto run = [&]() -> int {
        const auto now = [&]() { return sw.trace ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point{}; };
        const auto t0 = now();
        HIP_TRY(hipMemsetAsync(ws.ismed, 0, n * sizeof(uint32_t), c->stream));
        uint32_t swap_slot = PAM_NONE, swap_c = 0;
        bool append = false;
        if (!init) {
            // BUILD.  Slot 0: the smallest A(c, 0) under near = 0, d1 = 0, d2 = +inf, k = 1
            if (int e = reset()) return e;
            HIP_TRY(hipMemsetAsync(ws.near, 0, n * sizeof(uint32_t), c->stream));
            HIP_TRY(hipMemsetAsync(ws.d1, 0, n * sizeof(float), c->stream));
            HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws.d2), 0x7F800000, n, c->stream));
            if (int e = pam_scan_core(c, s, who, d_x, n, d, 1u, metric, dM, diag, nullptr, n, sw, ws, out, PamPick{PamPick::A0, false})) return e;
            if (int e = read()) return e;
            if (h.c == PAM_NONE) return fail(BLISSGPU_ERR_NAN, who, "no first medoid: every sum of distances is NaN");
            swap_slot = 0; swap_c = h.c; append = true;
            // every further slot: the non-medoid c with the smallest btot(c) under the state so far
            for (uint32_t K = 1; K < k; K++) {
                if (int e = reset()) return e;
                if (int e = state(K, swap_slot, swap_c, true, false)) return e;
                if (int e = pam_scan_core(c, s, who, d_x, n, d, K, metric, dM, diag, nullptr, n, sw, ws, out, PamPick{PamPick::BTOT, true})) return e;
                if (int e = read()) return e;
                if (h.c == PAM_NONE) return fail(BLISSGPU_ERR_NAN, who, "no next medoid: every candidate's change is NaN");
                if (sw.trace) fprintf(stderr, "%s build slot %u: song %u, btot %.17g\n", who, K, h.c, h.val);
                swap_slot = K; swap_c = h.c;
            }
        }
        for (;;) {
            if (int e = reset()) return e;
            if (int e = state(k, swap_slot, swap_c, append, init && swaps == 0)) return e;
            const auto t_scan = now();
            if (int e = pam_scan_core(c, s, who, d_x, n, d, k, metric, dM, diag, nullptr, n, sw, ws, out, PamPick{PamPick::BEST, true})) return e;
            if (int e = read()) return e;
            td_trace[swaps] = h.td;
            if (sw.trace)
                fprintf(stderr, "%s round %u: TD %.17g, winner %u into slot %u, delta %.17g, scan %.3f ms\n", who, swaps, h.td, h.c, h.arg, h.val,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_scan).count());
            if (h.c == PAM_NONE || !(h.val < 0.0)) { conv = 1; break; }
            if (swaps == max_swaps) break;
            swap_slot = h.arg; swap_c = h.c; append = false;
            swaps++;
        }
        if (sw.trace)
            fprintf(stderr, "%s: %u swaps, %.3f ms in all\n", who, swaps, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return BLISSGPU_OK;
    };
    if (!rc) rc = run();
    if (!rc) {
        s.down(medoids, ws.med, (size_t)k * sizeof(uint32_t));
        s.down(labels, ws.near, n * sizeof(uint32_t));
        s.down(dist, ws.d1, n * sizeof(float));
    }
    if ((rc = s.finish(rc))) return rc;
    if (sizes) {
        memset(sizes, 0, (size_t)k * sizeof(uint32_t));
        for (uint64_t o = 0; o < n; o++) sizes[labels[o]]++;
    }
    *n_swaps = swaps;
    *converged = conv;
    return BLISSGPU_OK;
}

int blissgpu_pam_plan(uint64_t n, uint32_t d, uint32_t k, uint64_t q, int build, uint64_t ws_limit, uint64_t* plan) {
    const char* who = "blissgpu_pam_plan";
    int rc = pam_scalars_ok(who, n, d, k, BLISSGPU_METRIC_EUCLIDEAN, nullptr);
    if (rc) return rc;
    if (!plan) return fail(BLISSGPU_ERR_INVALID, who, "plan is NULL");
    const PamLayout L = pam_layout(n, d, build ? 1u : k, k, q, ws_limit);
    plan[0] = L.fixed + L.slab * L.per_row;
    plan[1] = L.slab;
    plan[2] = L.hist_cap;
    plan[3] = L.tiles_cap;
    if (L.slab == 0) return fail(BLISSGPU_ERR_OOM, who, "the state and one candidate's sums do not fit the workspace limit");
    return BLISSGPU_OK;
}

// ---- acoustic fingerprints (kernels_fingerprint.hip): the band energies of every frame and the words from
// them, a group of songs at a time; and the alignment search over candidate pairs ----
uint64_t blissgpu_fingerprint_len(uint64_t n_samples) {
    return n_samples < (uint64_t)(FP_FRAME + FP_HOP) ? 0 : (n_samples - FP_FRAME) / FP_HOP;
}

int blissgpu_fingerprint_bands(uint32_t* edges) {
    static const uint32_t kEdges[FP_BANDS + 1] = {FP_EDGE_LIST};
    if (!edges) return fail(BLISSGPU_ERR_INVALID, "blissgpu_fingerprint_bands", "edges is NULL");
    memcpy(edges, kEdges, sizeof(kEdges));
    return BLISSGPU_OK;
}

static size_t fp_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
static int fp_launched(const char* who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BLISSGPU_OK : fail(BLISSGPU_ERR_HIP, who, hipGetErrorString(e));
}

int blissgpu_fingerprint_batch(const float* pcm, const uint64_t* sample_offsets, const uint64_t* word_offsets, uint32_t n_songs,
                               uint32_t* words, int32_t* status, double* energies) {
    const char* who = "blissgpu_fingerprint_batch";
    if (n_songs == 0) return BLISSGPU_OK;
    if (!sample_offsets) return fail(BLISSGPU_ERR_INVALID, who, "sample_offsets is NULL");
    if (!word_offsets) return fail(BLISSGPU_ERR_INVALID, who, "word_offsets is NULL");
    if (!status) return fail(BLISSGPU_ERR_INVALID, who, "status is NULL");
    if (word_offsets[0] != 0) return fail(BLISSGPU_ERR_INVALID, who, "word_offsets[0] must be 0");
    for (uint32_t s = 0; s < n_songs; s++) {
        if (sample_offsets[s + 1] < sample_offsets[s]) return fail(BLISSGPU_ERR_INVALID, who, "sample_offsets must ascend");
        const uint64_t w = blissgpu_fingerprint_len(sample_offsets[s + 1] - sample_offsets[s]);
        if (w > FP_MAX_WORDS) return fail(BLISSGPU_ERR_INVALID, who, "a song has more than 2^22 words");
        if (word_offsets[s + 1] < word_offsets[s] || word_offsets[s + 1] - word_offsets[s] != w)
            return fail(BLISSGPU_ERR_INVALID, who, "word_offsets[s + 1] - word_offsets[s] must be blissgpu_fingerprint_len of song s");
    }
    if (sample_offsets[n_songs] > sample_offsets[0] && !pcm) return fail(BLISSGPU_ERR_INVALID, who, "pcm is NULL");
    if (word_offsets[n_songs] && !words) return fail(BLISSGPU_ERR_INVALID, who, "words is NULL");
    for (uint32_t s = 0; s < n_songs; s++) status[s] = word_offsets[s + 1] == word_offsets[s] ? BLISSGPU_SONG_TOO_SHORT : BLISSGPU_SONG_OK;
    // a too-short song owns one row of the energies, all zero
    auto zero_short_rows = [&](uint32_t s0, uint32_t s1) {
        if (!energies) return;
        for (uint32_t s = s0; s < s1; s++)
            if (status[s] != BLISSGPU_SONG_OK) memset(energies + (word_offsets[s] + s) * FP_BANDS, 0, FP_BANDS * sizeof(double));
    };
    if (word_offsets[n_songs] == 0) {  // nothing for a device to do
        zero_short_rows(0, n_songs);
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    // the songs go through the device in groups of consecutive songs: at most 1 GiB of energies and 2 GiB of PCM (and a
    // quarter and a half of the workspace limit), one song at the least
    const uint64_t row_bytes = FP_BANDS * sizeof(double);
    const uint64_t e_budget = std::min<uint64_t>(1ull << 30, c->ws_limit / 4), pcm_budget = std::min<uint64_t>(2ull << 30, c->ws_limit / 2);
    std::vector<FpSong> desc;
    std::vector<uint32_t> run_pfx, word_pfx;
    for (uint32_t g0 = 0; g0 < n_songs;) {
        uint32_t g1 = g0;
        uint64_t rows = 0, samples = 0;
        while (g1 < n_songs) {
            const uint64_t r = word_offsets[g1 + 1] - word_offsets[g1] + 1, sm = sample_offsets[g1 + 1] - sample_offsets[g1];
            if (g1 > g0 && ((rows + r) * row_bytes > e_budget || (samples + sm) * sizeof(float) > pcm_budget)) break;
            rows += r;
            samples += sm;
            g1++;
        }
        const uint32_t ng = g1 - g0;
        const uint64_t gw = word_offsets[g1] - word_offsets[g0];
        if (gw == 0) {
            zero_short_rows(g0, g1);
            g0 = g1;
            continue;
        }
        desc.resize(ng);
        run_pfx.assign(ng + 1, 0);
        word_pfx.assign(ng + 1, 0);
        for (uint32_t k = 0; k < ng; k++) {
            const uint32_t w = (uint32_t)(word_offsets[g0 + k + 1] - word_offsets[g0 + k]), frames = w ? w + 1 : 0;
            desc[k] = FpSong{sample_offsets[g0 + k] - sample_offsets[g0], frames, word_pfx[k] + k};
            run_pfx[k + 1] = run_pfx[k] + (frames + FP_RUN - 1) / FP_RUN;
            word_pfx[k + 1] = word_pfx[k] + w;
        }
        const size_t o_pcm = 0, o_e = o_pcm + fp_align(samples * sizeof(float)), o_words = o_e + fp_align(rows * row_bytes),
                     o_desc = o_words + fp_align(gw * sizeof(uint32_t)), o_run = o_desc + fp_align(ng * sizeof(FpSong)),
                     o_wpfx = o_run + fp_align((ng + 1) * sizeof(uint32_t)), total = o_wpfx + fp_align((ng + 1) * sizeof(uint32_t));
        if ((rc = c->fp_ws.ensure(total))) return rc;
        uint8_t* base = c->fp_ws.p;
        float* d_pcm = reinterpret_cast<float*>(base + o_pcm);
        double* d_e = reinterpret_cast<double*>(base + o_e);
        uint32_t* d_words = reinterpret_cast<uint32_t*>(base + o_words);
        FpSong* d_desc = reinterpret_cast<FpSong*>(base + o_desc);
        uint32_t *d_run = reinterpret_cast<uint32_t*>(base + o_run), *d_wpfx = reinterpret_cast<uint32_t*>(base + o_wpfx);
        HostStage s{c, "fingerprint"};
        s.up(d_pcm, pcm + sample_offsets[g0], samples * sizeof(float));
        s.up(d_desc, desc.data(), ng * sizeof(FpSong));
        s.up(d_run, run_pfx.data(), (ng + 1) * sizeof(uint32_t));
        s.up(d_wpfx, word_pfx.data(), (ng + 1) * sizeof(uint32_t));
        rc = s.uploaded();
        if (!rc) {
            { Prof p(c, KX_FP_BANDS); launch_fp_bands(d_pcm, d_desc, ng, d_run, run_pfx[ng], c->tables.hann8192, c->tables.tw8192, d_e, c->stream); }
            rc = fp_launched(who);
        }
        if (!rc) {
            { Prof p(c, KX_FP_BITS); launch_fp_bits(d_e, d_wpfx, ng, (uint32_t)gw, d_words, c->stream); }
            rc = fp_launched(who);
        }
        if (!rc) {
            s.down(words + word_offsets[g0], d_words, gw * sizeof(uint32_t));
            if (energies) s.down(energies + (word_offsets[g0] + g0) * FP_BANDS, d_e, rows * row_bytes);
        }
        if ((rc = s.finish(rc))) return rc;
        zero_short_rows(g0, g1);
        g0 = g1;
    }
    return BLISSGPU_OK;
}

int blissgpu_fingerprint_match(const uint32_t* words, const uint64_t* word_offsets, uint32_t n_songs, const uint32_t* pairs, uint64_t n_pairs,
                               uint32_t max_offset, uint32_t min_overlap, int32_t* offset, uint32_t* errors, uint32_t* bits) {
    const char* who = "blissgpu_fingerprint_match";
    if (max_offset > FP_MAX_OFFSET) return fail(BLISSGPU_ERR_INVALID, who, "max_offset must be <= 4096");
    if (min_overlap == 0) return fail(BLISSGPU_ERR_INVALID, who, "min_overlap must be >= 1");
    if (n_pairs == 0) return BLISSGPU_OK;
    if (n_pairs >= (1ull << 32)) return fail(BLISSGPU_ERR_INVALID, who, "n_pairs must be below 2^32");
    if (!word_offsets) return fail(BLISSGPU_ERR_INVALID, who, "word_offsets is NULL");
    if (!pairs) return fail(BLISSGPU_ERR_INVALID, who, "pairs is NULL");
    if (!offset || !errors || !bits) return fail(BLISSGPU_ERR_INVALID, who, "offset, errors or bits is NULL");
    for (uint32_t s = 0; s < n_songs; s++) {
        if (word_offsets[s + 1] < word_offsets[s]) return fail(BLISSGPU_ERR_INVALID, who, "word_offsets must ascend");
        if (word_offsets[s + 1] - word_offsets[s] > FP_MAX_WORDS) return fail(BLISSGPU_ERR_INVALID, who, "a song has more than 2^22 words");
    }
    for (uint64_t p = 0; p < 2 * n_pairs; p++) {
        if (pairs[p] >= n_songs) return fail(BLISSGPU_ERR_INVALID, who, "a pair names a song >= n_songs");
        if (word_offsets[pairs[p] + 1] == word_offsets[pairs[p]]) return fail(BLISSGPU_ERR_INVALID, who, "a pair names a song without words");
    }
    if (!words) return fail(BLISSGPU_ERR_INVALID, who, "words is NULL");
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    const uint64_t n_words = word_offsets[n_songs];
    const uint32_t n_blocks = (2 * max_offset + 1 + 255) / 256;
    const uint64_t batch = std::min<uint64_t>(n_pairs, 65536);  // pairs per launch: the candidates of a batch are 16 n_blocks bytes a pair
    const size_t o_words = 0, o_off = o_words + fp_align(n_words * sizeof(uint32_t)), o_pairs = o_off + fp_align((n_songs + 1ull) * sizeof(uint64_t)),
                 o_out = o_pairs + fp_align(2 * n_pairs * sizeof(uint32_t)), o_cand = o_out + fp_align(3 * n_pairs * sizeof(uint32_t)),
                 total = o_cand + fp_align(batch * n_blocks * sizeof(FpCand));
    if ((rc = c->fp_ws.ensure(total))) return rc;
    uint8_t* base = c->fp_ws.p;
    uint32_t* d_words = reinterpret_cast<uint32_t*>(base + o_words);
    uint64_t* d_off = reinterpret_cast<uint64_t*>(base + o_off);
    uint32_t* d_pairs = reinterpret_cast<uint32_t*>(base + o_pairs);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(base + o_out);  // offset | errors | bits, n_pairs each
    FpCand* d_cand = reinterpret_cast<FpCand*>(base + o_cand);
    HostStage s{c, "fingerprint_match"};
    s.up(d_words, words, n_words * sizeof(uint32_t));
    s.up(d_off, word_offsets, (n_songs + 1ull) * sizeof(uint64_t));
    s.up(d_pairs, pairs, 2 * n_pairs * sizeof(uint32_t));
    rc = s.uploaded();
    for (uint64_t p0 = 0; !rc && p0 < n_pairs; p0 += batch) {
        const uint32_t np = (uint32_t)std::min<uint64_t>(batch, n_pairs - p0);
        { Prof p(c, KX_FP_MATCH); launch_fp_match(d_words, d_off, n_songs, d_pairs + 2 * p0, np, n_blocks, (int)max_offset, min_overlap, d_cand, c->stream); }
        rc = fp_launched(who);
        if (rc) break;
        { Prof p(c, KX_FP_PICK); launch_fp_pick(d_cand, np, n_blocks, reinterpret_cast<int32_t*>(d_out) + p0, d_out + n_pairs + p0, d_out + 2 * n_pairs + p0, c->stream); }
        rc = fp_launched(who);
    }
    if (!rc) {
        s.down(offset, d_out, n_pairs * sizeof(uint32_t));
        s.down(errors, d_out + n_pairs, n_pairs * sizeof(uint32_t));
        s.down(bits, d_out + 2 * n_pairs, n_pairs * sizeof(uint32_t));
    }
    return s.finish(rc);
}

// ---- loudness (kernels_loudness.hip, loudness_gate.hpp): the device delivers the sub-block energies and the
// peaks of a group of songs at a time; the blocks, the gates and the range behind them are host arithmetic ----
uint64_t blissgpu_loudness_subblocks(uint64_t frames, uint32_t sample_rate) { return loud_subblocks(frames, sample_rate); }

int blissgpu_loudness_kweighting(uint32_t sample_rate, double* coef) {
    const char* who = "blissgpu_loudness_kweighting";
    if (!loud_rate_ok(sample_rate)) return fail(BLISSGPU_ERR_INVALID, who, "sample_rate must be 8000 .. 768000");
    if (!coef) return fail(BLISSGPU_ERR_INVALID, who, "coef is NULL");
    loud_kweighting(sample_rate, coef);
    return BLISSGPU_OK;
}

int blissgpu_true_peak_filter(uint32_t sample_rate, uint32_t* factor, double* h) {
    const char* who = "blissgpu_true_peak_filter";
    if (!loud_rate_ok(sample_rate)) return fail(BLISSGPU_ERR_INVALID, who, "sample_rate must be 8000 .. 768000");
    if (!factor || !h) return fail(BLISSGPU_ERR_INVALID, who, "factor or h is NULL");
    *factor = loud_peak_factor(sample_rate);
    loud_peak_filter(*factor, h);
    return BLISSGPU_OK;
}

int blissgpu_loudness_blocks(const double* z, uint32_t channels, uint64_t n_sub, uint32_t sample_rate, double* P, double* ST) {
    const char* who = "blissgpu_loudness_blocks";
    if (!loud_rate_ok(sample_rate)) return fail(BLISSGPU_ERR_INVALID, who, "sample_rate must be 8000 .. 768000");
    if (channels < 1 || channels > 2) return fail(BLISSGPU_ERR_INVALID, who, "channels must be 1 or 2");
    if (n_sub && !z) return fail(BLISSGPU_ERR_INVALID, who, "z is NULL");
    loud_blocks(z, channels, n_sub, loud_hop(sample_rate), P, ST);
    return BLISSGPU_OK;
}

int blissgpu_loudness_gate(const double* P, uint64_t n, double* power, double* lufs) {
    const char* who = "blissgpu_loudness_gate";
    if (n && !P) return fail(BLISSGPU_ERR_INVALID, who, "P is NULL");
    if (!power || !lufs) return fail(BLISSGPU_ERR_INVALID, who, "power or lufs is NULL");
    *power = loud_gate(P, n);
    *lufs = loud_lufs(*power);
    return BLISSGPU_OK;
}

int blissgpu_loudness_range(const double* ST, uint64_t n, double* range_lu, double* lo, double* hi) {
    const char* who = "blissgpu_loudness_range";
    if (n && !ST) return fail(BLISSGPU_ERR_INVALID, who, "ST is NULL");
    if (!range_lu || !lo || !hi) return fail(BLISSGPU_ERR_INVALID, who, "range_lu, lo or hi is NULL");
    *range_lu = loud_range(ST, n, lo, hi);
    return BLISSGPU_OK;
}

// what can be said about the songs of a call without a device: the arguments, every song's status and where its energies go
// (zoff [n_songs + 1], in doubles: channels * n_sub per song, too-short songs included)
static int loud_songs_ok(const char* who, const blissgpu_decoded_song* songs, uint32_t n_songs, int32_t* status, std::vector<uint64_t>& zoff) {
    if (!songs) return fail(BLISSGPU_ERR_INVALID, who, "songs is NULL");
    if (!status) return fail(BLISSGPU_ERR_INVALID, who, "status is NULL");
    zoff.assign((size_t)n_songs + 1, 0);
    for (uint32_t s = 0; s < n_songs; s++) {
        const blissgpu_decoded_song& d = songs[s];
        if (d.channels < 1 || d.channels > 2)
            return fail(BLISSGPU_ERR_INVALID, who, "channels must be 1 or 2 (surround weights need a channel layout)");
        if (!loud_rate_ok(d.sample_rate)) return fail(BLISSGPU_ERR_INVALID, who, "sample_rate must be 8000 .. 768000");
        if (d.sample_format != BLISSGPU_SAMPLE_F32 && d.sample_format != BLISSGPU_SAMPLE_S16 && d.sample_format != BLISSGPU_SAMPLE_S32)
            return fail(BLISSGPU_ERR_INVALID, who, "sample_format must be F32, S16 or S32");
        if (d.frames > (1ull << 40)) return fail(BLISSGPU_ERR_INVALID, who, "a song has more than 2^40 frames");
        if (d.frames && !d.pcm) return fail(BLISSGPU_ERR_INVALID, who, "a song's pcm is NULL");
        const uint64_t n_sub = loud_subblocks(d.frames, d.sample_rate);
        status[s] = n_sub < LOUD_BLOCK_SUBS ? BLISSGPU_SONG_TOO_SHORT : BLISSGPU_SONG_OK;
        zoff[s + 1] = zoff[s] + n_sub * d.channels;
    }
    return BLISSGPU_OK;
}

// The device half on the context and device pointers: the energies and the peaks of one group of songs whose PCM, descriptors,
// class lists and taps are already there.  classes: per (format, channels) the offset of its list in song_of / row_pfx terms.
struct LoudClass {
    int format, channels;
    uint32_t n_class, n_rows;
    const uint32_t *d_song_of, *d_row_pfx;
};
static int loud_group_device(blissgpu_ctx* c, const char* who, const uint8_t* d_pcm, const LoudSong* d_desc, uint32_t n_songs,
                             const LoudClass* classes, int n_classes, const uint32_t* d_tile_pfx, uint32_t n_tiles,
                             const double* d_htab, double* d_part, double* d_z, double* d_peaks) {
    int rc = BLISSGPU_OK;
    for (int k = 0; k < n_classes && !rc; k++) {
        const LoudClass& lc = classes[k];
        { Prof p(c, KX_LOUD_ENERGY); launch_loud_energy(d_pcm, d_desc, lc.format, lc.channels, lc.d_song_of, lc.d_row_pfx, lc.n_class, lc.n_rows, d_z, c->stream); }
        rc = fp_launched(who);
    }
    if (!rc) {
        { Prof p(c, KX_LOUD_PEAK); launch_loud_peak(d_pcm, d_desc, n_songs, d_tile_pfx, n_tiles, d_htab, d_part, c->stream); }
        rc = fp_launched(who);
    }
    if (!rc) {
        { Prof p(c, KX_LOUD_FOLD); launch_loud_fold(d_part, d_tile_pfx, n_songs, d_peaks, c->stream); }
        rc = fp_launched(who);
    }
    return rc;
}

static int loud_energies_host(const char* who, const blissgpu_decoded_song* songs, uint32_t n_songs, const std::vector<uint64_t>& zoff,
                              double* z, double* sample_peak, double* true_peak, const int32_t* status) {
    if (zoff[n_songs] && !z) return fail(BLISSGPU_ERR_INVALID, who, "z is NULL");
    if (!sample_peak || !true_peak) return fail(BLISSGPU_ERR_INVALID, who, "sample_peak or true_peak is NULL");
    // a too-short song never reaches the device: its energies and peaks are zero.  Its energies are cleared once, when its group
    // is done (a group's z comes back in one copy that runs over them)
    auto zero_short = [&](uint32_t s0, uint32_t s1) {
        for (uint32_t s = s0; s < s1; s++)
            if (status[s] != BLISSGPU_SONG_OK && zoff[s + 1] > zoff[s]) memset(z + zoff[s], 0, (zoff[s + 1] - zoff[s]) * sizeof(double));
    };
    bool any = false;
    for (uint32_t s = 0; s < n_songs; s++) {
        sample_peak[s] = true_peak[s] = 0.0;
        any = any || status[s] == BLISSGPU_SONG_OK;
    }
    if (!any) {
        zero_short(0, n_songs);
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    static const std::vector<double> htab = [] {
        std::vector<double> h(3 * LOUD_TAPS);
        loud_peak_filter(4, h.data());
        loud_peak_filter(2, h.data() + LOUD_TAPS);
        loud_peak_filter(1, h.data() + 2 * LOUD_TAPS);
        return h;
    }();
    // groups of consecutive songs: at most 8 GiB of PCM (and half the workspace limit), one song at the least.  The energy kernel
    // is bound by the latency of its longest row, not by throughput, until a launch has several workgroups per CU: large groups
    const uint64_t pcm_budget = std::min<uint64_t>(8ull << 30, c->ws_limit / 2);
    auto pcm_bytes = [&](uint32_t s) {
        const blissgpu_decoded_song& d = songs[s];
        return status[s] == BLISSGPU_SONG_OK ? (uint64_t)fp_align(d.frames * d.channels * (d.sample_format == BLISSGPU_SAMPLE_S16 ? 2 : 4)) : 0ull;
    };
    std::vector<LoudSong> desc;
    std::vector<uint32_t> ok, tile_pfx, lists;  // lists: per class song_of | row_pfx, one after the other
    std::vector<double> peaks;
    for (uint32_t g0 = 0; g0 < n_songs;) {
        uint32_t g1 = g0;
        uint64_t bytes = 0;
        while (g1 < n_songs && (g1 == g0 || bytes + pcm_bytes(g1) <= pcm_budget)) bytes += pcm_bytes(g1++);
        ok.clear();
        for (uint32_t s = g0; s < g1; s++)
            if (status[s] == BLISSGPU_SONG_OK) ok.push_back(s);
        const uint32_t ng = (uint32_t)ok.size();
        if (ng == 0) {
            zero_short(g0, g1);
            g0 = g1;
            continue;
        }
        desc.resize(ng);
        tile_pfx.assign(ng + 1, 0);
        uint64_t off = 0;
        for (uint32_t k = 0; k < ng; k++) {
            const blissgpu_decoded_song& d = songs[ok[k]];
            LoudSong& L = desc[k];
            L.pcm_off = off;
            L.frames = d.frames;
            L.z_off = zoff[ok[k]] - zoff[g0];
            L.hop = loud_hop(d.sample_rate);
            L.n_sub = (uint32_t)loud_subblocks(d.frames, d.sample_rate);
            L.channels = d.channels;
            L.format = d.sample_format;
            L.factor = loud_peak_factor(d.sample_rate);
            loud_kweighting(d.sample_rate, L.coef);
            off += pcm_bytes(ok[k]);
            const uint64_t tiles = (uint64_t)tile_pfx[k] + loud_peak_tiles(d.frames, d.channels);
            if (tiles >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "a group of songs has 2^32 peak tiles or more");
            tile_pfx[k + 1] = (uint32_t)tiles;
        }
        // the classes present in the group, each with its songs and the rows in front of them
        LoudClass classes[6];
        size_t list_at[6];
        int n_classes = 0;
        lists.clear();
        for (int fmt = 0; fmt < 3; fmt++)
            for (int ch = 1; ch <= 2; ch++) {
                const size_t at = lists.size();
                for (uint32_t k = 0; k < ng; k++)
                    if (desc[k].format == fmt && desc[k].channels == ch) lists.push_back(k);
                const uint32_t nc = (uint32_t)(lists.size() - at);
                if (!nc) continue;
                uint64_t rows = 0;
                lists.push_back(0);
                for (uint32_t i = 0; i < nc; i++) {
                    rows += (desc[lists[at + i]].n_sub + BLISSGPU_LOUDNESS_SEGMENT - 1) / BLISSGPU_LOUDNESS_SEGMENT;
                    lists.push_back((uint32_t)rows);
                }
                if (rows >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "a group of songs has 2^32 segments or more");
                classes[n_classes] = LoudClass{fmt, ch, nc, (uint32_t)rows, nullptr, nullptr};
                list_at[n_classes++] = at;
            }
        const uint64_t gz = zoff[g1] - zoff[g0];
        const uint32_t n_tiles = tile_pfx[ng];
        const size_t o_pcm = 0, o_z = o_pcm + fp_align(off + 256), o_desc = o_z + fp_align(gz * sizeof(double)),
                     o_lists = o_desc + fp_align(ng * sizeof(LoudSong)), o_tile = o_lists + fp_align(lists.size() * sizeof(uint32_t)),
                     o_part = o_tile + fp_align((ng + 1) * sizeof(uint32_t)), o_peaks = o_part + fp_align(2 * (size_t)n_tiles * sizeof(double)),
                     o_htab = o_peaks + fp_align(2 * (size_t)ng * sizeof(double)), total = o_htab + fp_align(htab.size() * sizeof(double));
        if ((rc = c->ld_ws.ensure(total))) return rc;
        uint8_t* base = c->ld_ws.p;
        uint32_t* d_lists = reinterpret_cast<uint32_t*>(base + o_lists);
        for (int k = 0; k < n_classes; k++) {
            classes[k].d_song_of = d_lists + list_at[k];
            classes[k].d_row_pfx = d_lists + list_at[k] + classes[k].n_class;
        }
        HostStage s{c, "loudness"};
        for (uint32_t k = 0; k < ng; k++) {
            const blissgpu_decoded_song& d = songs[ok[k]];
            s.up(base + o_pcm + desc[k].pcm_off, d.pcm, d.frames * d.channels * (d.sample_format == BLISSGPU_SAMPLE_S16 ? 2 : 4));
        }
        s.up(base + o_desc, desc.data(), ng * sizeof(LoudSong));
        s.up(d_lists, lists.data(), lists.size() * sizeof(uint32_t));
        s.up(base + o_tile, tile_pfx.data(), (ng + 1) * sizeof(uint32_t));
        s.up(base + o_htab, htab.data(), htab.size() * sizeof(double));
        rc = s.uploaded();
        if (!rc)
            rc = loud_group_device(c, who, base + o_pcm, reinterpret_cast<const LoudSong*>(base + o_desc), ng, classes, n_classes,
                                   reinterpret_cast<const uint32_t*>(base + o_tile), n_tiles, reinterpret_cast<const double*>(base + o_htab),
                                   reinterpret_cast<double*>(base + o_part), reinterpret_cast<double*>(base + o_z),
                                   reinterpret_cast<double*>(base + o_peaks));
        peaks.assign(2 * (size_t)ng, 0.0);
        if (!rc) {
            s.down(z + zoff[g0], base + o_z, gz * sizeof(double));
            s.down(peaks.data(), base + o_peaks, peaks.size() * sizeof(double));
        }
        if ((rc = s.finish(rc))) return rc;
        for (uint32_t k = 0; k < ng; k++) {
            sample_peak[ok[k]] = peaks[2 * (size_t)k];
            true_peak[ok[k]] = peaks[2 * (size_t)k + 1];
        }
        zero_short(g0, g1);  // (the device wrote nothing there)
        g0 = g1;
    }
    return BLISSGPU_OK;
}

int blissgpu_loudness_energies(const blissgpu_decoded_song* songs, uint32_t n_songs, double* z, double* sample_peak, double* true_peak,
                               int32_t* status) {
    const char* who = "blissgpu_loudness_energies";
    if (n_songs == 0) return BLISSGPU_OK;
    std::vector<uint64_t> zoff;
    const int rc = loud_songs_ok(who, songs, n_songs, status, zoff);
    if (rc) return rc;
    return loud_energies_host(who, songs, n_songs, zoff, z, sample_peak, true_peak, status);
}

int blissgpu_loudness_batch(const blissgpu_decoded_song* songs, uint32_t n_songs, const uint32_t* album, uint32_t n_albums,
                            double* song_out, double* album_out, int32_t* status) {
    const char* who = "blissgpu_loudness_batch";
    if (album) {
        if (!album_out) return fail(BLISSGPU_ERR_INVALID, who, "album labels without album_out");
        for (uint32_t s = 0; s < n_songs; s++)
            if (album[s] >= n_albums) return fail(BLISSGPU_ERR_INVALID, who, "an album label is >= n_albums");
    }
    std::vector<uint64_t> zoff(1, 0);
    std::vector<double> z, sp(n_songs), tp(n_songs);
    if (n_songs) {
        if (!song_out) return fail(BLISSGPU_ERR_INVALID, who, "song_out is NULL");
        int rc = loud_songs_ok(who, songs, n_songs, status, zoff);
        if (rc) return rc;
        z.resize(std::max<uint64_t>(1, zoff[n_songs]));
        if ((rc = loud_energies_host(who, songs, n_songs, zoff, z.data(), sp.data(), tp.data(), status))) return rc;
    }
    // the gates: per song over its own blocks, per album over the concatenation of its OK songs' blocks in song order
    std::vector<std::vector<double>> aP(album ? n_albums : 0), aST(album ? n_albums : 0);
    std::vector<double> P, ST, apk(album ? 2 * (size_t)n_albums : 0, 0.0);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint32_t s = 0; s < n_songs; s++) {
        double* row = song_out + 5 * (size_t)s;
        if (status[s] != BLISSGPU_SONG_OK) {
            for (int k = 0; k < 5; k++) row[k] = nan;
            continue;
        }
        const uint64_t n_sub = (zoff[s + 1] - zoff[s]) / songs[s].channels;
        P.assign(n_sub - (LOUD_BLOCK_SUBS - 1), 0.0);
        ST.assign(n_sub >= LOUD_SHORT_SUBS ? n_sub - (LOUD_SHORT_SUBS - 1) : 0, 0.0);
        loud_blocks(z.data() + zoff[s], songs[s].channels, n_sub, loud_hop(songs[s].sample_rate), P.data(), ST.data());
        double lo, hi;
        row[0] = loud_gate(P.data(), P.size());
        row[1] = loud_lufs(row[0]);
        row[2] = loud_range(ST.data(), ST.size(), &lo, &hi);
        row[3] = sp[s];
        row[4] = tp[s];
        if (album) {
            const uint32_t a = album[s];
            aP[a].insert(aP[a].end(), P.begin(), P.end());
            aST[a].insert(aST[a].end(), ST.begin(), ST.end());
            apk[2 * (size_t)a] = std::max(apk[2 * (size_t)a], sp[s]);
            apk[2 * (size_t)a + 1] = std::max(apk[2 * (size_t)a + 1], tp[s]);
        }
    }
    if (album)
        for (uint32_t a = 0; a < n_albums; a++) {
            double* row = album_out + 5 * (size_t)a;
            double lo, hi;
            row[0] = loud_gate(aP[a].data(), aP[a].size());
            row[1] = loud_lufs(row[0]);
            row[2] = loud_range(aST[a].data(), aST[a].size(), &lo, &hi);
            row[3] = apk[2 * (size_t)a];
            row[4] = apk[2 * (size_t)a + 1];
        }
    return BLISSGPU_OK;
}

// ---- the moments of a library: counts, means, squared deviations and extrema per group of a labelling, and the pooled scatter
// matrix (kernels_moments.hip); the k-means sort of the labels, then one launch per level of the blocked sum ----
// everything that can be said about the scalar arguments and the pointers without a device
static int moments_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, const void* labels, uint32_t k, const void* counts,
                           const void* mean, const void* mn, const void* mx) {
    if (k == 0 || k > BLISSGPU_KMEANS_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KMEANS_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 rows");
    if (n && !labels && k != 1) return fail(BLISSGPU_ERR_INVALID, who, "without labels k must be 1");
    if (n && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (!counts) return fail(BLISSGPU_ERR_INVALID, who, "counts is NULL");
    if (!mean) return fail(BLISSGPU_ERR_INVALID, who, "mean is NULL");
    if (!mn != !mx) return fail(BLISSGPU_ERR_INVALID, who, "min and max go together: both or neither");
    return BLISSGPU_OK;
}

int blissgpu_moments_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const uint32_t* d_labels, uint32_t k,
                            uint32_t* d_counts, double* d_mean, double* d_m2, float* d_min, float* d_max, double* d_S) {
    const char* who = "blissgpu_moments_device";
    int rc = moments_args_ok(who, d_x, n, d, d_labels, k, d_counts, d_mean, d_min, d_max);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    CTX_ENTER(c, who);
    const size_t kd = (size_t)k * d;
    const uint32_t w = d * (d + 1) / 2;
    HIP_TRY(hipMemsetAsync(d_mean, 0, kd * sizeof(double), c->stream));  // (an empty group keeps these zeros)
    if (d_m2) HIP_TRY(hipMemsetAsync(d_m2, 0, kd * sizeof(double), c->stream));
    if (n == 0) {  // no row: every group is empty
        HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)k * sizeof(uint32_t), c->stream));
        if (d_S) HIP_TRY(hipMemsetAsync(d_S, 0, (size_t)d * d * sizeof(double), c->stream));
        if (d_min) { Prof p(c, KX_MOMENTS_FINISH); launch_moments_finish(d_counts, nullptr, nullptr, k, d, d_min, d_max, c->stream); }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        return BLISSGPU_OK;
    }
    // workspace: flags u32[4] ([0] not finite, [1] MO_ERR_*) | with labels: hist u32[K][W] | scan totals | arow_off u32[K + 1] |
    // arow u32[n] | off u32[levels][K + 1] | keys u32[2][K d] | (8-byte aligned) the groups' partials A f64[items_0][d], B
    // f64[items_1][d] | the scatter's partials A f64[blocks_0][w], B f64[blocks_1][w].  Level l writes A when l is even, B when odd
    const MomentsPlan plan = moments_plan(n, k);
    LabelSort sort(kmeans_plan(n, k, c->n_cus), k, n);
    const size_t o_off = d_labels ? sort.end : sort.o_hist,  // (without labels the sort has no tables: the flags alone)
                 o_keys = o_off + (size_t)plan.levels * (k + 1), o_pa = (o_keys + 2 * kd + 1) & ~(size_t)1,
                 o_pb = o_pa + 2 * (size_t)plan.items[0] * d, o_sa = o_pb + 2 * (size_t)(plan.levels > 1 ? plan.items[1] : 0) * d,
                 o_sb = o_sa + 2 * (d_S ? (size_t)plan.blocks[0] * w : 0),
                 words = o_sb + 2 * (d_S && plan.levels > 1 ? (size_t)plan.blocks[1] * w : 0);
    rc = c->mo_ws.ensure(words * sizeof(uint32_t));
    if (rc) return rc;
    uint32_t* ws = reinterpret_cast<uint32_t*>(c->mo_ws.p);
    sort.bind(ws);
    uint32_t *flags = ws, *arow_off = d_labels ? sort.arow_off : nullptr, *arow = d_labels ? sort.arow : nullptr, *off = ws + o_off,
             *keys = ws + o_keys;
    double* gpart[2] = {reinterpret_cast<double*>(ws + o_pa), reinterpret_cast<double*>(ws + o_pb)};
    double* spart[2] = {reinterpret_cast<double*>(ws + o_sa), reinterpret_cast<double*>(ws + o_sb)};
    MomentsArgs a{};
    a.X = d_x; a.labels = d_labels; a.arow_off = arow_off; a.arow = arow; a.off = off; a.mean = d_mean;
    a.n = (uint32_t)n; a.K = k; a.d = d; a.key_min = keys; a.key_max = keys + kd; a.flags = flags;
    HIP_TRY(hipMemsetAsync(ws, 0, (d_labels ? sort.zero_words() : sort.o_hist) * sizeof(uint32_t), c->stream));
    if (d_labels) sort.launch(c, d_labels);
    { Prof p(c, KX_MOMENTS_PLAN); launch_moments_plan(arow_off, (uint32_t)n, k, plan, off, d_counts, c->stream); }
    // the levels above level 0 of one per-group quantity, and its last step into dst
    auto group_levels = [&](int mode, double* dst) {
        for (uint32_t l = 1; l < plan.levels; l++) {
            Prof p(c, KX_MOMENTS_REDUCE);
            launch_moments_reduce(gpart[(l - 1) & 1], off + (size_t)(l - 1) * (k + 1), 0, gpart[l & 1], off + (size_t)l * (k + 1), 0,
                                  plan.items[l], k, d, MO_RED_PART, d_counts, nullptr, d, c->stream);
        }
        const uint32_t* last = off + (size_t)(plan.levels - 1) * (k + 1);
        Prof p(c, KX_MOMENTS_REDUCE);
        launch_moments_reduce(gpart[(plan.levels - 1) & 1], last, 0, nullptr, last, 0, plan.items[plan.levels - 1], k, d, mode, d_counts,
                              dst, d, c->stream);
    };
    { Prof p(c, KX_MOMENTS_SUM); launch_moments_sum(a, plan, gpart[0], c->stream); }
    group_levels(MO_RED_MEAN, d_mean);
    if (d_m2 || d_min) {
        if (d_min) {
            HIP_TRY(hipMemsetAsync(a.key_min, 0xFF, kd * sizeof(uint32_t), c->stream));
            HIP_TRY(hipMemsetAsync(a.key_max, 0, kd * sizeof(uint32_t), c->stream));
        }
        { Prof p(c, KX_MOMENTS_M2); launch_moments_m2(a, plan, gpart[0], d_min != nullptr, c->stream); }
        if (d_m2) group_levels(MO_RED_M2, d_m2);
        if (d_min) { Prof p(c, KX_MOMENTS_FINISH); launch_moments_finish(d_counts, a.key_min, a.key_max, k, d, d_min, d_max, c->stream); }
    }
    if (d_S) {
        { Prof p(c, KX_MOMENTS_SCATTER); launch_moments_scatter(a, plan, spart[0], c->stream); }
        for (uint32_t l = 1; l < plan.levels; l++) {
            Prof p(c, KX_MOMENTS_REDUCE);
            launch_moments_reduce(spart[(l - 1) & 1], nullptr, plan.blocks[l - 1], spart[l & 1], nullptr, plan.blocks[l], plan.blocks[l], 1, w,
                                  MO_RED_PART, nullptr, nullptr, d, c->stream);
        }
        Prof p(c, KX_MOMENTS_REDUCE);
        launch_moments_reduce(spart[(plan.levels - 1) & 1], nullptr, plan.blocks[plan.levels - 1], nullptr, nullptr, 1, 1, 1, w,
                              MO_RED_SCATTER, nullptr, d_S, d, c->stream);
    }
    HIP_TRY(hipGetLastError());
    // the one synchronisation: the data-dependent errors
    uint32_t h_flags[2];
    if ((rc = read_flags(c, flags, 2, h_flags))) return rc;
    if (h_flags[1] & MO_ERR_LABEL) return fail(BLISSGPU_ERR_INVALID, who, "a label is >= k");
    if (h_flags[0]) return fail(BLISSGPU_ERR_NAN, who, "a NaN or an infinity in x");
    return BLISSGPU_OK;
}

int blissgpu_moments(const float* x, uint64_t n, uint32_t d, const uint32_t* labels, uint32_t k, uint32_t* counts, double* mean,
                     double* m2, float* mn, float* mx, double* S) {
    const char* who = "blissgpu_moments";
    int rc = moments_args_ok(who, x, n, d, labels, k, counts, mean, mn, mx);
    if (rc) return rc;
    const size_t kd = (size_t)k * d, dd = (size_t)d * d;
    if (n == 0) {  // no row: nothing for a device to do
        memset(counts, 0, (size_t)k * sizeof(uint32_t));
        for (size_t e = 0; e < kd; e++) {
            mean[e] = 0.0;
            if (m2) m2[e] = 0.0;
            if (mn) { mn[e] = INFINITY; mx[e] = -INFINITY; }
        }
        if (S) for (size_t e = 0; e < dd; e++) S[e] = 0.0;
        return BLISSGPU_OK;
    }
    if (labels)  // host memory: what the device form finds at its synchronisation is found here, before the device is touched
        for (uint64_t i = 0; i < n; i++)
            if (labels[i] >= k) return fail(BLISSGPU_ERR_INVALID, who, "a label is >= k");
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    // staging: x | labels, counts | mean, m2, S (f64), then min, max (f32)
    rc = c->st_b.ensure(n * d);
    if (!rc) rc = c->st_idx.ensure(n + k);
    if (!rc) rc = c->st_out.ensure((2 * kd + dd) * sizeof(double) + 2 * kd * sizeof(float));
    if (rc) return rc;
    uint32_t *d_labels = labels ? c->st_idx.p : nullptr, *d_counts = c->st_idx.p + n;
    double *d_mean = reinterpret_cast<double*>(c->st_out.p), *d_m2 = d_mean + kd, *d_S = d_m2 + kd;
    float *d_mn = reinterpret_cast<float*>(d_S + dd), *d_mx = d_mn + kd;
    HostStage s{c, "moments"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(d_labels, labels, n * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc)
        rc = blissgpu_moments_device(c, c->st_b.p, n, d, d_labels, k, d_counts, d_mean, m2 ? d_m2 : nullptr, mn ? d_mn : nullptr,
                                     mn ? d_mx : nullptr, S ? d_S : nullptr);
    if (!rc) {
        s.down(counts, d_counts, (size_t)k * sizeof(uint32_t));
        s.down(mean, d_mean, kd * sizeof(double));
        s.down(m2, d_m2, kd * sizeof(double));
        s.down(mn, d_mn, kd * sizeof(float));
        s.down(mx, d_mx, kd * sizeof(float));  // (min and max go together)
        s.down(S, d_S, dd * sizeof(double));
    }
    return s.finish(rc);
}

// a scatter matrix turned into a Mahalanobis M (covariance_metric.hpp): host arithmetic only, no device is touched
int blissgpu_covariance_metric(const double* S, uint32_t d, uint64_t dof, int form, double shrink, float* M, int32_t* status) {
    const char* who = "blissgpu_covariance_metric";
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (dof == 0) return fail(BLISSGPU_ERR_INVALID, who, "dof must be positive");
    if (!(shrink >= 0.0 && shrink <= 1.0)) return fail(BLISSGPU_ERR_INVALID, who, "shrink must be within 0 .. 1");
    if (form != BLISSGPU_METRIC_FORM_DIAGONAL && form != BLISSGPU_METRIC_FORM_FULL) return fail(BLISSGPU_ERR_INVALID, who, "unknown form");
    if (!S || !M || !status) return fail(BLISSGPU_ERR_INVALID, who, "S, M and status must not be NULL");
    static_assert(bg::covmetric::FORM_DIAGONAL == BLISSGPU_METRIC_FORM_DIAGONAL && bg::covmetric::FORM_FULL == BLISSGPU_METRIC_FORM_FULL &&
                      bg::covmetric::STATUS_OK == BLISSGPU_COV_OK && bg::covmetric::STATUS_NOT_POSITIVE == BLISSGPU_COV_NOT_POSITIVE,
                  "covariance_metric.hpp and blissgpu.h agree");
    *status = bg::covmetric::solve(S, d, dof, form, shrink, M);
    return BLISSGPU_OK;
}

// ---- triplet metric learning (kernels_metric.hip, metric_learn.hpp): one gradient evaluation on the device, and the projected
// gradient loop around it with X and the triplets resident; the host holds the d x d state ----
static int triplet_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, const void* triplets, uint64_t T, double margin) {
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(BLISSGPU_ERR_INVALID, who, "margin must be finite and >= 0");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 rows");
    if (T >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "T must be below 2^32 - 1 triplets");
    if (T && !triplets) return fail(BLISSGPU_ERR_INVALID, who, "triplets is NULL");
    if (T && n && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    return BLISSGPU_OK;
}

static int learn_args_ok(const char* who, uint32_t d, int form, const float* init, double lr, double reg, const void* M,
                         const void* n_iter, const void* best_iter, const void* status) {
    if (form != BLISSGPU_METRIC_FORM_DIAGONAL && form != BLISSGPU_METRIC_FORM_FULL) return fail(BLISSGPU_ERR_INVALID, who, "unknown form");
    if (!(reg >= 0.0) || !std::isfinite(reg)) return fail(BLISSGPU_ERR_INVALID, who, "reg must be finite and >= 0");
    if (!std::isfinite(lr)) return fail(BLISSGPU_ERR_INVALID, who, "lr must be finite");
    if (init)
        for (uint32_t r = 0; r < d; r++)
            if (!(init[r] >= 0.0f) || !std::isfinite(init[r])) return fail(BLISSGPU_ERR_INVALID, who, "init must be finite and >= 0");
    if (!M || !n_iter || !best_iter || !status) return fail(BLISSGPU_ERR_INVALID, who, "M / n_iter / best_iter / status is NULL");
    return BLISSGPU_OK;
}

// the workspace of one evaluation: partials f64 [W][pairs + 1] | counts u64 [W][2] | result f64 [d d + 3] | M f32 [64 x 64]
struct TripletWs {
    TripletPlan plan;
    double *part, *out;
    unsigned long long* cnt;
    float* m;
};

static int triplet_ws(blissgpu_ctx* c, uint64_t T, uint32_t d, TripletWs* w) {
    w->plan = triplet_plan(T, d);
    const size_t o_cnt = w->plan.part_doubles, o_out = o_cnt + 2 * (size_t)w->plan.W, o_m = o_out + (size_t)d * d + 3, words = o_m + 2048;
    int rc = c->mt_ws.ensure(words * sizeof(double));
    if (rc) return rc;
    double* base = reinterpret_cast<double*>(c->mt_ws.p);
    w->part = base;
    w->cnt = reinterpret_cast<unsigned long long*>(base + o_cnt);
    w->out = base + o_out;
    w->m = reinterpret_cast<float*>(base + o_m);
    return BLISSGPU_OK;
}

// launches the two kernels and downloads the result block in ONE copy.  T > 0.  h_out: d d + 3 doubles
static int triplet_eval(blissgpu_ctx* c, const char* who, const TripletWs& w, const float* d_x, uint64_t n, uint32_t d,
                        const uint32_t* d_trip, uint64_t T, const float* d_M, int mode, double margin, uint8_t* d_flags, double* h_out,
                        uint64_t* n_active, double* loss) {
    {
        Prof p(c, KX_TRIPLET_STEP);
        launch_triplet_step(d_x, n, d, d_trip, T, d_M, mode, margin, w.plan, d_flags, w.part, w.cnt, c->stream);
    }
    {
        Prof p(c, KX_TRIPLET_REDUCE);
        launch_triplet_reduce(w.part, w.cnt, w.plan, d, w.out, c->stream);
    }
    HIP_TRY(hipGetLastError());
    const size_t bytes = ((size_t)d * d + 3) * sizeof(double);
    HIP_TRY(hipMemcpyAsync(h_out, w.out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mt_downloads++;
    c->mt_bytes += bytes;
    uint64_t words[2];
    memcpy(words, h_out + (size_t)d * d + 1, sizeof(words));
    if (words[1] & TRIPLET_ERR_INDEX) return fail(BLISSGPU_ERR_INVALID, who, "a triplet names a row >= n");
    if (words[1] & TRIPLET_ERR_NAN) return fail(BLISSGPU_ERR_NAN, who, "NaN hinge");
    *n_active = words[0];
    *loss = h_out[(size_t)d * d];
    return BLISSGPU_OK;
}

static int m_mode(const float* hM, uint32_t d) {
    if (!hM) return TRIPLET_M_IDENTITY;
    return is_diag(hM, d) ? TRIPLET_M_DIAG : TRIPLET_M_FULL;
}

int blissgpu_triplet_step_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const uint32_t* d_triplets, uint64_t T,
                                 const float* d_M, double margin, uint8_t* d_flags, uint64_t* n_active, double* loss, double* G) {
    const char* who = "blissgpu_triplet_step_device";
    int rc = triplet_args_ok(who, d_x, n, d, d_triplets, T, margin);
    if (rc) return rc;
    if (!n_active || !loss || !G) return fail(BLISSGPU_ERR_INVALID, who, "n_active / loss / G is NULL");
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (T == 0) {
        *n_active = 0;
        *loss = 0.0;
        memset(G, 0, (size_t)d * d * sizeof(double));
        return BLISSGPU_OK;
    }
    CTX_ENTER(c, who);
    std::vector<float> hM;
    if (d_M) {  // how M is read is decided on its values, as everywhere else
        hM.resize((size_t)d * d);
        HIP_TRY(hipMemcpyAsync(hM.data(), d_M, hM.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    TripletWs w;
    if ((rc = triplet_ws(c, T, d, &w))) return rc;
    std::vector<double> h_out((size_t)d * d + 3);
    rc = triplet_eval(c, who, w, d_x, n, d, d_triplets, T, d_M, m_mode(d_M ? hM.data() : nullptr, d), margin, d_flags, h_out.data(),
                      n_active, loss);
    if (rc) return rc;
    memcpy(G, h_out.data(), (size_t)d * d * sizeof(double));
    return BLISSGPU_OK;
}

// X and the triplets of a host-pointer form, uploaded into the context's staging buffers
static int stage_triplets(blissgpu_ctx* c, const float* x, uint64_t n, uint32_t d, const uint32_t* triplets, uint64_t T) {
    int rc = c->st_b.ensure(std::max<size_t>(n * d, 1));
    if (!rc) rc = c->st_idx.ensure(3 * T);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(c->st_b.p, x, n * d * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->st_idx.p, triplets, 3 * T * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    return BLISSGPU_OK;
}

int blissgpu_triplet_step(const float* x, uint64_t n, uint32_t d, const uint32_t* triplets, uint64_t T, const float* M, double margin,
                          uint8_t* flags, uint64_t* n_active, double* loss, double* G) {
    const char* who = "blissgpu_triplet_step";
    int rc = triplet_args_ok(who, x, n, d, triplets, T, margin);
    if (rc) return rc;
    if (!n_active || !loss || !G) return fail(BLISSGPU_ERR_INVALID, who, "n_active / loss / G is NULL");
    if (T == 0) {
        *n_active = 0;
        *loss = 0.0;
        memset(G, 0, (size_t)d * d * sizeof(double));
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    TripletWs w;
    if ((rc = triplet_ws(c, T, d, &w))) return rc;
    if ((rc = stage_triplets(c, x, n, d, triplets, T))) return rc;
    if (M) HIP_TRY(hipMemcpyAsync(w.m, M, (size_t)d * d * sizeof(float), hipMemcpyHostToDevice, c->stream));
    uint8_t* d_flags = nullptr;
    if (flags) {
        if ((rc = c->st_out.ensure(T))) return rc;
        d_flags = c->st_out.p;
    }
    std::vector<double> h_out((size_t)d * d + 3);
    rc = triplet_eval(c, who, w, c->st_b.p, n, d, c->st_idx.p, T, M ? w.m : nullptr, m_mode(M, d), margin, d_flags, h_out.data(),
                      n_active, loss);
    if (rc) return rc;
    memcpy(G, h_out.data(), (size_t)d * d * sizeof(double));
    if (flags) {
        HIP_TRY(hipMemcpyAsync(flags, d_flags, T, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return BLISSGPU_OK;
}

int blissgpu_learn_metric_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const uint32_t* d_triplets, uint64_t T,
                                 int form, const float* init, double margin, double lr, double reg, uint32_t max_iter, float* M,
                                 double* obj, uint64_t* active, uint32_t* n_iter, uint32_t* best_iter, int32_t* status) {
    const char* who = "blissgpu_learn_metric_device";
    int rc = triplet_args_ok(who, d_x, n, d, d_triplets, T, margin);
    if (!rc) rc = learn_args_ok(who, d, form, init, lr, reg, M, n_iter, best_iter, status);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    CTX_ENTER(c, who);
    TripletWs w{};
    if (T && (rc = triplet_ws(c, T, d, &w))) return rc;
    c->mt_uploads = c->mt_downloads = c->mt_bytes = 0;
    std::vector<double> h_out((size_t)d * d + 3);
    const size_t m_bytes = (size_t)d * d * sizeof(float);
    auto step = [&](const float* hM, double* loss, uint64_t* act, double* G) -> int {
        if (T == 0) {  // no triplet: no hinge
            *loss = 0.0;
            *act = 0;
            return BLISSGPU_OK;
        }
        // (pageable memory: the copy has left hM when the call returns)
        HIP_TRY(hipMemcpyAsync(w.m, hM, m_bytes, hipMemcpyHostToDevice, c->stream));
        c->mt_uploads++;
        int r = triplet_eval(c, who, w, d_x, n, d, d_triplets, T, w.m, m_mode(hM, d), margin, nullptr, h_out.data(), act, loss);
        if (!r) memcpy(G, h_out.data(), (size_t)d * d * sizeof(double));
        return r;
    };
    return bg::metric::learn(form, d, init, T, lr, reg, max_iter, step, M, obj, active, n_iter, best_iter, status);
}

int blissgpu_learn_metric(const float* x, uint64_t n, uint32_t d, const uint32_t* triplets, uint64_t T, int form, const float* init,
                          double margin, double lr, double reg, uint32_t max_iter, float* M, double* obj, uint64_t* active,
                          uint32_t* n_iter, uint32_t* best_iter, int32_t* status) {
    const char* who = "blissgpu_learn_metric";
    int rc = triplet_args_ok(who, x, n, d, triplets, T, margin);
    if (!rc) rc = learn_args_ok(who, d, form, init, lr, reg, M, n_iter, best_iter, status);
    if (rc) return rc;
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    if (T && (rc = stage_triplets(c, x, n, d, triplets, T))) return rc;
    return blissgpu_learn_metric_device(c, c->st_b.p, n, d, c->st_idx.p, T, form, init, margin, lr, reg, max_iter, M, obj, active,
                                        n_iter, best_iter, status);
}

// ---- k nearest candidates per seed GROUP: closest_to_songs(&group, candidates, metric) cut after k (src/playlist.rs:36-59,
// 256-270), the primitive behind Library::playlist_from(&[several songs]).take(k) (src/library.rs:762-842), for every group of
// a library in one call ----
// everything that can be said about the arguments without a device (both forms check it BEFORE the device is touched)
static int group_knn_args_ok(const char* who, const void* seeds, const uint64_t* off, uint64_t n_groups, const void* cand,
                             uint64_t n, uint32_t d, int metric, const float* M, uint32_t k, const void* idx) {
    if (k == 0 || k > BLISSGPU_KNN_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KNN_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 candidates");
    if (n_groups >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n_groups must be below 2^32 - 1");
    if (n_groups == 0) return BLISSGPU_OK;
    if (!off) return fail(BLISSGPU_ERR_INVALID, who, "group_offsets is NULL");
    if (off[0] != 0) return fail(BLISSGPU_ERR_INVALID, who, "group_offsets[0] must be 0");
    for (uint64_t g = 0; g < n_groups; g++)
        if (off[g + 1] < off[g]) return fail(BLISSGPU_ERR_INVALID, who, "group_offsets must not decrease");
    if (off[n_groups] > 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "2^32 seeds or more");
    if (off[n_groups] && !seeds) return fail(BLISSGPU_ERR_INVALID, who, "seeds is NULL");
    if (n && !cand) return fail(BLISSGPU_ERR_INVALID, who, "cand is NULL");
    if (!idx) return fail(BLISSGPU_ERR_INVALID, who, "idx is NULL");
    return BLISSGPU_OK;
}

int blissgpu_group_knn_plan(const uint64_t* group_offsets, uint64_t n_groups, uint64_t n, uint32_t k, uint32_t n_cus,
                            uint32_t* items, uint64_t max_items, uint64_t* n_items, uint32_t* cand_block, uint32_t* seed_tile) {
    const char* who = "blissgpu_group_knn_plan";
    const float some = 0.0f;  // (the plan reads neither seeds nor candidates)
    uint32_t none = 0;
    int rc = group_knn_args_ok(who, &some, group_offsets, n_groups, &some, n, 1, 0, nullptr, k, &none);
    if (rc) return rc;
    if (n_cus == 0) return fail(BLISSGPU_ERR_INVALID, who, "n_cus must be at least 1");
    if (!n_items || (max_items && !items)) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    const GroupKnnPlan p = group_knn_plan(group_offsets, n_groups, n, k, n_cus);
    *n_items = p.items.size();
    if (cand_block) *cand_block = p.cand_block;
    if (seed_tile) *seed_tile = p.seed_tile;
    for (uint64_t i = 0; i < p.items.size() && i < max_items; i++) {
        items[4 * i + 0] = p.items[i].g_lo;
        items[4 * i + 1] = p.items[i].g_hi;
        items[4 * i + 2] = p.items[i].c_lo;
        items[4 * i + 3] = p.items[i].c_hi;
    }
    return BLISSGPU_OK;
}

// both device forms after their argument checks.  weighted: the metric is Mahalanobis with one diagonal M per group, rows of
// d_weights ([n_groups][d]) or, with d_weights == NULL, the variance-based weights of each group's own seeds, computed into
// the workspace by one more launch; d_status (may be NULL) is then written
static int group_knn_run(blissgpu_ctx* c, const char* who, const float* d_seeds, const uint64_t* group_offsets, uint64_t n_groups,
                         const float* d_cand, uint64_t n, uint32_t d, int metric, const float* d_M, bool weighted,
                         const float* d_weights, int32_t* d_status, const uint32_t* d_skip, uint32_t k, uint32_t* d_idx,
                         float* d_dist) {
    int rc;
    int diag = 0;
    if (weighted) {
        metric = BLISSGPU_METRIC_MAHALANOBIS;
        diag = GROUP_KNN_M_PER_GROUP;
    } else if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // the plan and its tables: group offsets (32 bits: fewer than 2^32 seeds) | list offsets | items.  Workspace: the sorted k
    // best keys of every (group, item that covers it) -- no seeds x n or groups x n array exists anywhere
    const GroupKnnPlan plan = group_knn_plan(group_offsets, n_groups, n, k, (uint32_t)std::max(1, c->n_cus));
    const size_t n_off = (size_t)n_groups + 1, n_item_words = plan.items.size() * (sizeof(GroupKnnItem) / sizeof(uint32_t));
    std::vector<uint32_t> table(2 * n_off + n_item_words);
    for (size_t g = 0; g < n_off; g++) table[g] = (uint32_t)group_offsets[g];
    std::copy(plan.list_off.begin(), plan.list_off.end(), table.begin() + n_off);
    if (n_item_words) memcpy(table.data() + 2 * n_off, plan.items.data(), n_item_words * sizeof(uint32_t));
    const uint64_t n_lists = plan.list_off[n_groups];
    // (derived weights: n_groups x d floats behind the lists)
    const bool derive = weighted && !d_weights;
    const size_t part_bytes = std::max<size_t>(8, (size_t)n_lists * k * sizeof(unsigned long long));
    rc = c->pl_sync.ensure(4);
    if (!rc) rc = c->pl_keys.ensure(table.size());
    if (!rc) rc = c->pl_tmp.ensure(part_bytes + (derive ? (size_t)n_groups * d * sizeof(float) : 0));
    if (rc) return rc;
    const uint32_t *d_goff = c->pl_keys.p, *d_list_off = d_goff + n_off;
    const GroupKnnItem* d_items = reinterpret_cast<const GroupKnnItem*>(d_list_off + n_off);
    unsigned long long* part = reinterpret_cast<unsigned long long*>(c->pl_tmp.p);
    HIP_TRY(hipMemcpyAsync(c->pl_keys.p, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    // pl_sync: [1] NaN among the scores of eligible pairs, [3] a skip entry >= n
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    if (derive) {
        float* w = reinterpret_cast<float*>(c->pl_tmp.p + part_bytes);
        {
            Prof p(c, K_GROUP_WEIGHTS);
            launch_group_weights(d_seeds, d_goff, n_groups, d, w, d_status, c->stream);
        }
        HIP_TRY(hipGetLastError());
        d_M = w;
    } else if (weighted) {
        if (d_status) HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)n_groups * sizeof(int32_t), c->stream));  // BLISSGPU_GROUP_OK
        d_M = d_weights;
    }
    {
        Prof p(c, K_GROUP_KNN_SCAN);
        launch_group_knn_scan(d_seeds, d_goff, d_cand, (uint32_t)n, d, metric, d_M, diag, d_skip, k, plan, d_items, d_list_off,
                              part, c->pl_sync.p + 1, c->pl_sync.p + 3, c->stream);
    }
    HIP_TRY(hipGetLastError());
    {
        Prof p(c, K_GROUP_KNN_MERGE);
        launch_group_knn_merge(part, d_list_off, n_groups, k, plan, d_idx, d_dist, c->stream);
    }
    HIP_TRY(hipGetLastError());
    uint32_t flags[4];
    if ((rc = read_flags(c, c->pl_sync.p, 4, flags))) return rc;  // (the tables above have left the host by now too)
    if (flags[3]) return fail(BLISSGPU_ERR_INVALID, who, "skip entries must be < n or 0xFFFFFFFF");
    if (flags[1]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

int blissgpu_group_knn_device(blissgpu_ctx* c, const float* d_seeds, const uint64_t* group_offsets, uint64_t n_groups,
                              const float* d_cand, uint64_t n, uint32_t d, int metric, const float* d_M, const uint32_t* d_skip,
                              uint32_t k, uint32_t* d_idx, float* d_dist) {
    const char* who = "blissgpu_group_knn_device";
    int rc = group_knn_args_ok(who, d_seeds, group_offsets, n_groups, d_cand, n, d, metric, d_M, k, d_idx);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_groups == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    return group_knn_run(c, who, d_seeds, group_offsets, n_groups, d_cand, n, d, metric, d_M, false, nullptr, nullptr, d_skip, k,
                         d_idx, d_dist);
}

int blissgpu_group_knn(const float* seeds, const uint64_t* group_offsets, uint64_t n_groups, const float* cand, uint64_t n,
                       uint32_t d, int metric, const float* M, const uint32_t* skip, uint32_t k, uint32_t* idx, float* dist) {
    const char* who = "blissgpu_group_knn";
    int rc = group_knn_args_ok(who, seeds, group_offsets, n_groups, cand, n, d, metric, M, k, idx);
    if (rc) return rc;
    if (n_groups == 0) return BLISSGPU_OK;
    const uint64_t n_seeds = group_offsets[n_groups];
    if ((rc = skip_entries_ok(who, skip, n_seeds, n))) return rc;
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    const size_t out_n = (size_t)n_groups * k;
    GroupLists g;
    if ((rc = group_lists_stage(c, n_seeds, true, n, d, metric, M, skip != nullptr, out_n, dist ? out_n : 0, &g))) return rc;
    HostStage s{c, "group_knn"};
    rc = group_lists_host(s, g, seeds, n_seeds, cand, n, d, skip, out_n, idx, dist, [&]() {
        return blissgpu_group_knn_device(c, g.seeds, group_offsets, n_groups, g.cand, n, d, metric, g.M, g.skip, k, g.idx, g.dist);
    });
    return s.finish(rc);
}

// ---- one diagonal metric per seed group: variance_based_weight_matrix (src/playlist.rs:173-221) of every group on the device,
// and the k-nearest search per group under M_g = diag(weights[g]) ----
static int group_weights_args_ok(const char* who, const void* seeds, const uint64_t* off, uint64_t n_groups, uint32_t d,
                                 const void* weights) {
    const float some = 0.0f;  // (no candidates, no k, no metric here)
    int rc = group_knn_args_ok(who, seeds, off, n_groups, &some, 0, d, BLISSGPU_METRIC_EUCLIDEAN, nullptr, 1, &some);
    if (rc) return rc;
    if (n_groups && !weights) return fail(BLISSGPU_ERR_INVALID, who, "weights is NULL");
    return BLISSGPU_OK;
}

int blissgpu_group_weights_device(blissgpu_ctx* c, const float* d_seeds, const uint64_t* group_offsets, uint64_t n_groups,
                                  uint32_t d, float* d_weights, int32_t* d_group_status) {
    const char* who = "blissgpu_group_weights_device";
    int rc = group_weights_args_ok(who, d_seeds, group_offsets, n_groups, d, d_weights);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_groups == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    std::vector<uint32_t> goff((size_t)n_groups + 1);  // 32 bits: fewer than 2^32 seeds
    for (size_t g = 0; g < goff.size(); g++) goff[g] = (uint32_t)group_offsets[g];
    rc = c->pl_keys.ensure(goff.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->pl_keys.p, goff.data(), goff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    {
        Prof p(c, K_GROUP_WEIGHTS);
        launch_group_weights(d_seeds, c->pl_keys.p, n_groups, d, d_weights, d_group_status, c->stream);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the offsets have left the host)
    return BLISSGPU_OK;
}

// the host forms' staging of weights and status: st_out holds [n_groups][d] floats, then n_groups status words
static int stage_group_weights(blissgpu_ctx* c, uint64_t n_groups, uint32_t d, float** d_w, int32_t** d_status) {
    const size_t w_bytes = (size_t)n_groups * d * sizeof(float);
    int rc = c->st_out.ensure(w_bytes + (size_t)n_groups * sizeof(int32_t));
    if (rc) return rc;
    *d_w = reinterpret_cast<float*>(c->st_out.p);
    *d_status = reinterpret_cast<int32_t*>(c->st_out.p + w_bytes);
    return BLISSGPU_OK;
}

int blissgpu_group_weights(const float* seeds, const uint64_t* group_offsets, uint64_t n_groups, uint32_t d, float* weights,
                           int32_t* group_status) {
    const char* who = "blissgpu_group_weights";
    int rc = group_weights_args_ok(who, seeds, group_offsets, n_groups, d, weights);
    if (rc) return rc;
    if (n_groups == 0) return BLISSGPU_OK;
    const uint64_t n_seeds = group_offsets[n_groups];
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    float* d_w = nullptr;
    int32_t* d_status = nullptr;
    rc = c->st_a.ensure(std::max<size_t>(1, n_seeds * d));
    if (!rc) rc = stage_group_weights(c, n_groups, d, &d_w, &d_status);
    if (rc) return rc;
    HostStage s{c, "group_weights"};
    s.up(c->st_a.p, seeds, n_seeds * d * sizeof(float));
    rc = s.uploaded();
    if (!rc) rc = blissgpu_group_weights_device(c, c->st_a.p, group_offsets, n_groups, d, d_w, d_status);
    if (!rc) {
        s.down(weights, d_w, (size_t)n_groups * d * sizeof(float));
        s.down(group_status, d_status, (size_t)n_groups * sizeof(int32_t));
    }
    return s.finish(rc);
}

int blissgpu_group_knn_weighted_device(blissgpu_ctx* c, const float* d_seeds, const uint64_t* group_offsets, uint64_t n_groups,
                                       const float* d_cand, uint64_t n, uint32_t d, const float* d_weights,
                                       const uint32_t* d_skip, uint32_t k, uint32_t* d_idx, float* d_dist,
                                       int32_t* d_group_status) {
    const char* who = "blissgpu_group_knn_weighted_device";
    int rc = group_knn_args_ok(who, d_seeds, group_offsets, n_groups, d_cand, n, d, BLISSGPU_METRIC_EUCLIDEAN, nullptr, k, d_idx);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_groups == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    return group_knn_run(c, who, d_seeds, group_offsets, n_groups, d_cand, n, d, BLISSGPU_METRIC_MAHALANOBIS, nullptr, true,
                         d_weights, d_group_status, d_skip, k, d_idx, d_dist);
}

int blissgpu_group_knn_weighted(const float* seeds, const uint64_t* group_offsets, uint64_t n_groups, const float* cand,
                                uint64_t n, uint32_t d, const float* weights, const uint32_t* skip, uint32_t k, uint32_t* idx,
                                float* dist, int32_t* group_status) {
    const char* who = "blissgpu_group_knn_weighted";
    int rc = group_knn_args_ok(who, seeds, group_offsets, n_groups, cand, n, d, BLISSGPU_METRIC_EUCLIDEAN, nullptr, k, idx);
    if (rc) return rc;
    if (n_groups == 0) return BLISSGPU_OK;
    const uint64_t n_seeds = group_offsets[n_groups];
    if ((rc = skip_entries_ok(who, skip, n_seeds, n))) return rc;
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    const size_t out_n = (size_t)n_groups * k;
    float* d_w = nullptr;
    int32_t* d_status = nullptr;
    GroupLists g;
    rc = group_lists_stage(c, n_seeds, true, n, d, BLISSGPU_METRIC_EUCLIDEAN, nullptr, skip != nullptr, out_n, dist ? out_n : 0, &g);
    if (!rc) rc = stage_group_weights(c, n_groups, d, &d_w, &d_status);
    if (rc) return rc;
    HostStage s{c, "group_knn_weighted"};
    rc = group_lists_host(s, g, seeds, n_seeds, cand, n, d, skip, out_n, idx, dist, [&]() {
        s.up(d_w, weights, (size_t)n_groups * d * sizeof(float));  // (the weights travel behind seeds, candidates and skip)
        if (int r = s.uploaded()) return r;
        return blissgpu_group_knn_weighted_device(c, g.seeds, group_offsets, n_groups, g.cand, n, d, weights ? d_w : nullptr, g.skip, k,
                                                  g.idx, g.dist, group_status ? d_status : nullptr);
    });
    if (!rc) s.down(group_status, d_status, (size_t)n_groups * sizeof(int32_t));
    return s.finish(rc);
}

// ---- k nearest ALBUMS per seed group: closest_album_to_group (src/playlist.rs:424-485) cut after k albums, the primitive behind
// Library::album_playlist_from (src/library.rs:850-893), for every group of a library in one call (kernels_albums.hip,
// DESIGN.md 3.16) ----
// everything that can be said about the arguments without a device (both forms check it BEFORE the device is touched)
static int album_knn_args_ok(const char* who, const void* seeds, const uint64_t* off, uint64_t n_groups, const void* cand,
                             uint64_t n, uint32_t d, const void* album_of, uint64_t n_albums, uint32_t k, const void* idx) {
    int rc = group_knn_args_ok(who, seeds, off, n_groups, cand, n, d, BLISSGPU_METRIC_EUCLIDEAN, nullptr, k, idx);
    if (rc) return rc;
    if (n_albums > n) return fail(BLISSGPU_ERR_INVALID, who, "n_albums must be at most n");
    if (n_groups == 0) return BLISSGPU_OK;
    for (uint64_t g = 0; g < n_groups; g++)
        if (off[g + 1] == off[g]) return fail(BLISSGPU_ERR_INVALID, who, "empty group (the reference's \"Mean of empty slice\")");
    if (n && !album_of) return fail(BLISSGPU_ERR_INVALID, who, "album_of is NULL");
    return BLISSGPU_OK;
}

// album_of and skip, on the host
static int album_knn_data_ok(const char* who, const uint32_t* album_of, uint64_t n, uint64_t n_albums, const uint32_t* skip,
                             uint64_t n_seeds) {
    for (uint64_t i = 0; i < n; i++)
        if (album_of[i] != 0xFFFFFFFFu && album_of[i] >= n_albums)
            return fail(BLISSGPU_ERR_INVALID, who, "album_of entries must be < n_albums or 0xFFFFFFFF");
    return skip_entries_ok(who, skip, n_seeds, n);
}

// The tables of bg::AlbumTables in one array of words, in this order: goff | arow_off | arow | patch_off | patch_album |
// patch_cnt | pskip_off | pskip.  The album row lists are a stable counting sort of the candidates by album; a group's patches
// come from the sorted, deduplicated (album, row) pairs of its skip entries -- at most one patch and one lost row per seed row.
struct AlbumTablesHost {
    std::vector<uint32_t> words;
    size_t o_arow_off, o_arow, o_patch_off, o_patch_album, o_patch_cnt, o_pskip_off, o_pskip;
    uint32_t n_patches;
};
static void album_tables_build(const uint64_t* off, uint64_t n_groups, const uint32_t* album_of, uint64_t n, uint64_t n_albums,
                               const uint32_t* skip, AlbumTablesHost& h) {
    std::vector<uint32_t> arow_off(n_albums + 1, 0u);
    for (uint64_t i = 0; i < n; i++)
        if (album_of[i] != 0xFFFFFFFFu) arow_off[album_of[i] + 1u]++;
    for (uint64_t a = 0; a < n_albums; a++) arow_off[a + 1] += arow_off[a];
    std::vector<uint32_t> arow(arow_off[n_albums]), fill(arow_off.begin(), arow_off.end() - 1);
    for (uint64_t i = 0; i < n; i++)
        if (album_of[i] != 0xFFFFFFFFu) arow[fill[album_of[i]]++] = (uint32_t)i;
    std::vector<uint32_t> patch_off(n_groups + 1, 0u), patch_album, patch_cnt, pskip_off(1, 0u), pskip;
    std::vector<std::pair<uint32_t, uint32_t>> lost;  // (album, row) pairs of one group
    for (uint64_t g = 0; g < n_groups; g++) {
        lost.clear();
        if (skip)
            for (uint64_t s = off[g]; s < off[g + 1]; s++)
                if (skip[s] != 0xFFFFFFFFu && album_of[skip[s]] != 0xFFFFFFFFu) lost.emplace_back(album_of[skip[s]], skip[s]);
        std::sort(lost.begin(), lost.end());
        lost.erase(std::unique(lost.begin(), lost.end()), lost.end());
        for (size_t i = 0; i < lost.size();) {
            const uint32_t a = lost[i].first;
            size_t j = i;
            for (; j < lost.size() && lost[j].first == a; j++) pskip.push_back(lost[j].second);
            patch_album.push_back(a);
            patch_cnt.push_back(arow_off[a + 1] - arow_off[a] - (uint32_t)(j - i));
            pskip_off.push_back((uint32_t)pskip.size());
            i = j;
        }
        patch_off[g + 1] = (uint32_t)patch_album.size();
    }
    h.n_patches = (uint32_t)patch_album.size();
    h.words.clear();
    for (uint64_t g = 0; g <= n_groups; g++) h.words.push_back((uint32_t)off[g]);
    auto put = [&](const std::vector<uint32_t>& v) {
        const size_t at = h.words.size();
        h.words.insert(h.words.end(), v.begin(), v.end());
        return at;
    };
    h.o_arow_off = put(arow_off);
    h.o_arow = put(arow);
    h.o_patch_off = put(patch_off);
    h.o_patch_album = put(patch_album);
    h.o_patch_cnt = put(patch_cnt);
    h.o_pskip_off = put(pskip_off);
    h.o_pskip = put(pskip);
}

// both forms after their checks: seeds, candidates and outputs on the device, album_of and skip (checked) on the host.
// d_gmeans / d_cent may be NULL: the means then live in the workspace only
static int album_knn_run(blissgpu_ctx* c, const char* who, const float* d_seeds, const uint64_t* group_offsets, uint64_t n_groups,
                         const float* d_cand, uint64_t n, uint32_t d, const uint32_t* h_album_of, uint64_t n_albums,
                         const uint32_t* h_skip, uint32_t k, uint32_t* d_idx, float* d_dist, float* d_gmeans, float* d_cent) {
    AlbumTablesHost h;
    album_tables_build(group_offsets, n_groups, h_album_of, n, n_albums, h_skip, h);
    // workspace: the sorted k best keys of every (group, split) | the means that have no output of their own | the patched
    // centroids -- O(A d + G d + touched pairs x d + items x k); no n_groups x n_albums array exists anywhere
    const KnnPlan plan = knn_plan(n_groups, n_albums, k, c->n_cus);
    const size_t part_bytes = std::max<size_t>(8, (size_t)plan.part_keys * sizeof(unsigned long long));
    const size_t cent_floats = d_cent ? 0 : (size_t)n_albums * d, gm_floats = d_gmeans ? 0 : (size_t)n_groups * d;
    int rc = c->pl_sync.ensure(4);
    if (!rc) rc = c->pl_keys.ensure(h.words.size());
    if (!rc) rc = c->pl_tmp.ensure(part_bytes + (cent_floats + gm_floats + (size_t)h.n_patches * d) * sizeof(float));
    if (rc) return rc;
    unsigned long long* part = reinterpret_cast<unsigned long long*>(c->pl_tmp.p);
    float* ws = reinterpret_cast<float*>(c->pl_tmp.p + part_bytes);
    float* cent = d_cent ? d_cent : ws;
    float* gmeans = d_gmeans ? d_gmeans : ws + cent_floats;
    float* pcent = ws + cent_floats + gm_floats;
    const uint32_t* w = c->pl_keys.p;
    const AlbumTables t{w,
                        w + h.o_arow_off,
                        w + h.o_arow,
                        w + h.o_patch_off,
                        w + h.o_patch_album,
                        w + h.o_patch_cnt,
                        w + h.o_pskip_off,
                        w + h.o_pskip,
                        (uint32_t)n_albums,
                        (uint32_t)n_groups,
                        h.n_patches};
    HIP_TRY(hipMemcpyAsync(c->pl_keys.p, h.words.data(), h.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    // pl_sync: [1] NaN distance of an existing (group, album) pair
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    {
        Prof p(c, KX_SEGMENT_MEAN);
        launch_segment_mean(d_cand, d_seeds, d, t, cent, gmeans, pcent, c->stream);
    }
    HIP_TRY(hipGetLastError());
    {
        Prof p(c, KX_ALBUM_KNN_SCAN);
        launch_album_knn_scan(gmeans, cent, d, t, pcent, k, plan, part, c->pl_sync.p + 1, c->stream);
    }
    HIP_TRY(hipGetLastError());
    {
        Prof p(c, K_KNN_MERGE);
        launch_knn_merge(part, n_groups, k, plan, d_idx, d_dist, c->stream);
    }
    HIP_TRY(hipGetLastError());
    uint32_t flags[4];
    if ((rc = read_flags(c, c->pl_sync.p, 4, flags))) return rc;  // (the tables above have left the host by now too)
    if (flags[1]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

int blissgpu_album_knn_device(blissgpu_ctx* c, const float* d_seeds, const uint64_t* group_offsets, uint64_t n_groups,
                              const float* d_cand, uint64_t n, uint32_t d, const uint32_t* d_album_of, uint64_t n_albums,
                              const uint32_t* d_skip, uint32_t k, uint32_t* d_idx, float* d_dist, float* d_group_means,
                              float* d_centroids) {
    const char* who = "blissgpu_album_knn_device";
    int rc = album_knn_args_ok(who, d_seeds, group_offsets, n_groups, d_cand, n, d, d_album_of, n_albums, k, d_idx);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_groups == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    // the album row lists and the patches are built on the host: album_of and skip come back first (this synchronises the
    // stream, as the argument / NaN check at the end does anyway)
    const uint64_t n_seeds = group_offsets[n_groups];
    std::vector<uint32_t> album_of(n), skip(d_skip ? n_seeds : 0);
    if (n) HIP_TRY(hipMemcpyAsync(album_of.data(), d_album_of, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (d_skip) HIP_TRY(hipMemcpyAsync(skip.data(), d_skip, n_seeds * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = album_knn_data_ok(who, album_of.data(), n, n_albums, d_skip ? skip.data() : nullptr, n_seeds);
    if (rc) return rc;
    return album_knn_run(c, who, d_seeds, group_offsets, n_groups, d_cand, n, d, album_of.data(), n_albums,
                         d_skip ? skip.data() : nullptr, k, d_idx, d_dist, d_group_means, d_centroids);
}

int blissgpu_album_knn(const float* seeds, const uint64_t* group_offsets, uint64_t n_groups, const float* cand, uint64_t n,
                       uint32_t d, const uint32_t* album_of, uint64_t n_albums, const uint32_t* skip, uint32_t k, uint32_t* idx,
                       float* dist, float* group_means, float* centroids) {
    const char* who = "blissgpu_album_knn";
    int rc = album_knn_args_ok(who, seeds, group_offsets, n_groups, cand, n, d, album_of, n_albums, k, idx);
    if (rc) return rc;
    if (n_groups == 0) return BLISSGPU_OK;
    const uint64_t n_seeds = group_offsets[n_groups];
    rc = album_knn_data_ok(who, album_of, n, n_albums, skip, n_seeds);
    if (rc) return rc;
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    // staging: st_dist holds dist | group_means | centroids, each only when asked for
    const size_t out_n = (size_t)n_groups * k, gm_n = (size_t)n_groups * d, cent_n = (size_t)n_albums * d;
    const size_t o_gm = dist ? out_n : 0, o_cent = o_gm + (group_means ? gm_n : 0);
    // (skip stays on the host, where the patches are built from it; the metric is the Euclidean one)
    GroupLists g;
    rc = group_lists_stage(c, n_seeds, true, n, d, BLISSGPU_METRIC_EUCLIDEAN, nullptr, false, out_n,
                           std::max<size_t>(1, o_cent + (centroids ? cent_n : 0)), &g);
    if (rc) return rc;
    float *d_gm = group_means ? g.dist + o_gm : nullptr, *d_cent = centroids ? g.dist + o_cent : nullptr;
    HostStage s{c, "album_knn"};
    rc = group_lists_host(s, g, seeds, n_seeds, cand, n, d, nullptr, out_n, idx, dist, [&]() {
        return album_knn_run(c, who, g.seeds, group_offsets, n_groups, g.cand, n, d, album_of, n_albums, skip, k, g.idx,
                             dist ? g.dist : nullptr, d_gm, d_cent);
    });
    if (!rc) {
        s.down(group_means, d_gm, gm_n * sizeof(float));
        s.down(centroids, d_cent, cent_n * sizeof(float));
    }
    return s.finish(rc);
}

// ---- song-to-song chains cut after k, one per seed group: song_to_song(&group, candidates, metric).take(k)
// (src/playlist.rs:272-326) for every group in one call, without a grid barrier (kernels_chains.hip) ----
// The lists route pays n x n pairs (one k-nearest search of the candidates among themselves) plus the walk, the steps route
// (k - 1) x n_groups x n pairs.  LISTS is taken when c x n < (k - 1) x n_groups, c = CHAINS_LISTS_COST_NUM / _DEN = 1/2: measured
// at n = 10^5, d = 23, k = 20 (tests/tools/chains_bench.py, profiles/chains_bench_100k.json) the two routes
// cross between n/64 chains (break-even c = 0.33, steps faster) and n/16 (0.88, lists faster), near 2 650 chains.  c is below 1
// because a step over few chains runs an under-filled device (80 ms per 10^10 pairs at n/64 chains against 17 at n).
constexpr uint64_t CHAINS_LISTS_COST_NUM = 1, CHAINS_LISTS_COST_DEN = 2;

// L = k + largest group - 1: entries of a candidate's list that always hold the chain's next song
static uint64_t chains_list_len(const uint64_t* off, uint64_t n_groups, uint32_t k) {
    uint64_t gmax = 0;
    for (uint64_t g = 0; g < n_groups; g++) gmax = std::max(gmax, off[g + 1] - off[g]);
    return (uint64_t)k + gmax - 1u;  // (k >= 1)
}
// what the lists route keeps on the device beside the outputs: the lists' indices and distances, the keys of the search that
// makes them, and the candidates' own indices as its skip array
static unsigned __int128 chains_lists_bytes(uint64_t n, uint64_t L) {
    return (unsigned __int128)n * L * (sizeof(uint32_t) + sizeof(float) + sizeof(unsigned long long)) + (unsigned __int128)n * sizeof(uint32_t);
}
static bool chains_lists_fit(uint64_t n, uint32_t k, uint64_t L, uint64_t workspace_bytes) {
    return k >= 2 && n > 0 && L >= 1 && L <= BLISSGPU_KNN_MAX_K && chains_lists_bytes(n, L) <= (unsigned __int128)workspace_bytes;
}
static int chains_route(uint64_t n_groups, uint64_t n, uint32_t k, uint64_t L, uint64_t workspace_bytes) {
    if (!chains_lists_fit(n, k, L, workspace_bytes)) return BLISSGPU_CHAINS_STEPS;
    const unsigned __int128 lists = (unsigned __int128)CHAINS_LISTS_COST_NUM * n;
    const unsigned __int128 steps = (unsigned __int128)CHAINS_LISTS_COST_DEN * (k - 1u) * n_groups;
    return lists < steps ? BLISSGPU_CHAINS_LISTS : BLISSGPU_CHAINS_STEPS;
}

// everything that can be said about the arguments without a device (every form checks it BEFORE the device is touched)
static int chains_args_ok(const char* who, const void* seeds, const uint64_t* off, uint64_t n_groups, const void* cand, uint64_t n,
                          uint32_t d, int metric, const float* M, uint32_t k, int route, const void* idx) {
    if (route != BLISSGPU_CHAINS_AUTO && route != BLISSGPU_CHAINS_STEPS && route != BLISSGPU_CHAINS_LISTS)
        return fail(BLISSGPU_ERR_INVALID, who, "unknown route");
    int rc = group_knn_args_ok(who, seeds, off, n_groups, cand, n, d, metric, M, k, idx);
    if (rc) return rc;
    if (route == BLISSGPU_CHAINS_LISTS && n_groups && k >= 2 && chains_list_len(off, n_groups, k) > BLISSGPU_KNN_MAX_K)
        return fail(BLISSGPU_ERR_INVALID, who, "the lists route needs k + largest group - 1 <= BLISSGPU_KNN_MAX_K");
    return BLISSGPU_OK;
}

int blissgpu_chains_plan(const uint64_t* group_offsets, uint64_t n_groups, uint64_t n, uint32_t k, uint64_t workspace_bytes,
                         int* route, uint32_t* list_len) {
    const char* who = "blissgpu_chains_plan";
    const float some = 0.0f;  // (the plan reads neither seeds nor candidates)
    uint32_t none = 0;
    int rc = chains_args_ok(who, &some, group_offsets, n_groups, &some, n, 1, 0, nullptr, k, BLISSGPU_CHAINS_AUTO, &none);
    if (rc) return rc;
    if (!route) return fail(BLISSGPU_ERR_INVALID, who, "route is NULL");
    const uint64_t L = n_groups ? chains_list_len(group_offsets, n_groups, k) : (uint64_t)k - 1u;
    if (list_len) *list_len = (uint32_t)std::min<uint64_t>(L, 0xFFFFFFFFull);
    *route = n_groups ? chains_route(n_groups, n, k, L, workspace_bytes) : BLISSGPU_CHAINS_STEPS;
    return BLISSGPU_OK;
}

int blissgpu_chains_device(blissgpu_ctx* c, const float* d_seeds, const uint64_t* group_offsets, uint64_t n_groups,
                           const float* d_cand, uint64_t n, uint32_t d, int metric, const float* d_M, const uint32_t* d_skip,
                           uint32_t k, int route, uint32_t* d_idx, float* d_dist) {
    const char* who = "blissgpu_chains_device";
    int rc = chains_args_ok(who, d_seeds, group_offsets, n_groups, d_cand, n, d, metric, d_M, k, route, d_idx);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_groups == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    const uint64_t L = chains_list_len(group_offsets, n_groups, k);
    if (route == BLISSGPU_CHAINS_LISTS && k >= 2 && n && !chains_lists_fit(n, k, L, c->ws_limit))
        return fail(BLISSGPU_ERR_INVALID, who, "the lists do not fit the context's workspace limit");
    if (route == BLISSGPU_CHAINS_AUTO) route = chains_route(n_groups, n, k, L, c->ws_limit);
    if (k < 2 || n == 0) route = BLISSGPU_CHAINS_STEPS;  // (step 0 alone: nothing to walk)
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // pl_chain: minima u64[G] | flags u32[4] ([0] NaN on a chain, [1] a list too short) | offsets u32[G + 1] | step 0: idx u32[G],
    // dist f32[G] | lists route: the candidates' own indices u32[n], lists u32[n][L], their distances f32[n][L]
    const size_t G = (size_t)n_groups, out_n = G * k;
    const bool lists = route == BLISSGPU_CHAINS_LISTS;
    const size_t o_flags = G * sizeof(unsigned long long), o_goff = o_flags + 4 * sizeof(uint32_t);
    const size_t o_idx0 = o_goff + (G + 1) * sizeof(uint32_t), o_dist0 = o_idx0 + G * sizeof(uint32_t);
    const size_t o_self = o_dist0 + G * sizeof(float), o_lists = o_self + (lists ? (size_t)n * sizeof(uint32_t) : 0);
    const size_t o_ldist = o_lists + (lists ? (size_t)n * L * sizeof(uint32_t) : 0);
    const size_t total = o_ldist + (lists && d_dist ? (size_t)n * L * sizeof(float) : 0);
    rc = c->pl_chain.ensure(total);
    if (rc) return rc;
    unsigned long long* best = reinterpret_cast<unsigned long long*>(c->pl_chain.p);
    uint32_t* flags = reinterpret_cast<uint32_t*>(c->pl_chain.p + o_flags);
    uint32_t* d_goff = reinterpret_cast<uint32_t*>(c->pl_chain.p + o_goff);
    uint32_t* idx0 = reinterpret_cast<uint32_t*>(c->pl_chain.p + o_idx0);
    float* dist0 = d_dist ? reinterpret_cast<float*>(c->pl_chain.p + o_dist0) : nullptr;
    std::vector<uint32_t> table(G + 1 + (lists ? (size_t)n : 0));
    for (size_t g = 0; g <= G; g++) table[g] = (uint32_t)group_offsets[g];
    for (size_t j = 0; lists && j < (size_t)n; j++) table[G + 1 + j] = (uint32_t)j;
    HIP_TRY(hipMemcpyAsync(d_goff, table.data(), (G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (lists)
        HIP_TRY(hipMemcpyAsync(c->pl_chain.p + o_self, table.data() + G + 1, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    auto pad = [&]() -> hipError_t {  // every row: 0xFFFFFFFF / +inf until a step writes it
        hipError_t e = hipMemsetAsync(d_idx, 0xFF, out_n * sizeof(uint32_t), c->stream);
        if (e == hipSuccess && d_dist) e = hipMemsetD32Async((hipDeviceptr_t)d_dist, 0x7F800000, out_n, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(flags, 0, 4 * sizeof(uint32_t), c->stream);
        return e;
    };
    HIP_TRY(pad());
    // step 0: the group search with k = 1 (it synchronises: the tables above have left the host when it returns)
    rc = group_knn_run(c, who, d_seeds, group_offsets, n_groups, d_cand, n, d, metric, d_M, false, nullptr, nullptr, d_skip, 1u, idx0,
                       dist0);
    if (rc) return rc;
    uint32_t h_flags[4] = {0, 0, 0, 0};
    if (lists) {
        uint32_t* self = reinterpret_cast<uint32_t*>(c->pl_chain.p + o_self);
        uint32_t* l_idx = reinterpret_cast<uint32_t*>(c->pl_chain.p + o_lists);
        float* l_dist = d_dist ? reinterpret_cast<float*>(c->pl_chain.p + o_ldist) : nullptr;
        rc = blissgpu_knn_device(c, d_cand, n, d_cand, n, d, metric, d_M, self, (uint32_t)L, l_idx, l_dist);
        if (rc == BLISSGPU_OK) {
            {
                Prof p(c, K_CHAIN_WALK);
                launch_chain_walk(l_idx, l_dist, (uint32_t)L, d_goff, d_skip, idx0, dist0, (uint32_t)n_groups, k, d_idx, d_dist, flags + 1,
                                  c->stream);
            }
            HIP_TRY(hipGetLastError());
            if ((rc = read_flags(c, flags, 4, h_flags))) return rc;
            if (!h_flags[1]) return BLISSGPU_OK;
        } else if (rc != BLISSGPU_ERR_NAN) {
            return rc;
        }
        // the all-pairs search met a NaN that perhaps no chain evaluates (or a list was too short): the steps decide
        HIP_TRY(pad());
    }
    const ChainPlan plan = chain_plan(n_groups, n, c->n_cus);
    HIP_TRY(hipMemsetAsync(best, 0xFF, G * sizeof(unsigned long long), c->stream));
    {
        Prof p(c, K_CHAIN_STEP);
        launch_chain_first(idx0, dist0, (uint32_t)n_groups, k, d_idx, d_dist, c->stream);
    }
    HIP_TRY(hipGetLastError());
    const uint32_t steps = (uint32_t)std::min<uint64_t>(k, n);  // (a chain is no longer than the candidates)
    for (uint32_t t = 1; t < steps; t++) {
        Prof p(c, K_CHAIN_STEP);
        launch_chain_step(d_cand, (uint32_t)n, d, metric, d_M, diag, d_goff, d_skip, (uint32_t)n_groups, k, t, plan, d_idx, d_dist, best,
                          flags, c->stream);
    }
    HIP_TRY(hipGetLastError());
    if ((rc = read_flags(c, flags, 4, h_flags))) return rc;
    if (h_flags[0]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance (the reference panics here)");
    return BLISSGPU_OK;
}

int blissgpu_chains(const float* seeds, const uint64_t* group_offsets, uint64_t n_groups, const float* cand, uint64_t n, uint32_t d,
                    int metric, const float* M, const uint32_t* skip, uint32_t k, int route, uint32_t* idx, float* dist) {
    const char* who = "blissgpu_chains";
    int rc = chains_args_ok(who, seeds, group_offsets, n_groups, cand, n, d, metric, M, k, route, idx);
    if (rc) return rc;
    if (n_groups == 0) return BLISSGPU_OK;
    const uint64_t n_seeds = group_offsets[n_groups];
    if ((rc = skip_entries_ok(who, skip, n_seeds, n))) return rc;
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    const size_t out_n = (size_t)n_groups * k;
    GroupLists g;
    if ((rc = group_lists_stage(c, n_seeds, true, n, d, metric, M, skip != nullptr, out_n, dist ? out_n : 0, &g))) return rc;
    HostStage s{c, "chains"};
    rc = group_lists_host(s, g, seeds, n_seeds, cand, n, d, skip, out_n, idx, dist, [&]() {
        return blissgpu_chains_device(c, g.seeds, group_offsets, n_groups, g.cand, n, d, metric, g.M, g.skip, k, route, g.idx, g.dist);
    });
    return s.finish(rc);
}

// ---- journeys: waypoint and directed song-to-song playlists (kernels_chains.hip): the chains' steps with a
// step 0 of their own, a waypoint query or a gate on one feature ----
// everything that can be said about the arguments without a device (both forms check it BEFORE the device is touched)
static int journeys_args_ok(const char* who, const void* from, const void* to, uint64_t n_journeys, const void* cand, uint64_t n,
                            uint32_t d, int metric, const float* M, uint32_t k, int mode, int gate, uint32_t gate_feature,
                            const void* idx) {
    if (k == 0 || k > BLISSGPU_KNN_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KNN_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 candidates");
    if (n_journeys >= 0x80000000ull) return fail(BLISSGPU_ERR_INVALID, who, "n_journeys must be below 2^31");
    if (mode != BLISSGPU_JOURNEY_CHAIN && mode != BLISSGPU_JOURNEY_WAYPOINT) return fail(BLISSGPU_ERR_INVALID, who, "unknown mode");
    if (gate != BLISSGPU_GATE_NONE && gate != BLISSGPU_GATE_UP && gate != BLISSGPU_GATE_DOWN)
        return fail(BLISSGPU_ERR_INVALID, who, "unknown gate");
    if (gate != BLISSGPU_GATE_NONE && mode == BLISSGPU_JOURNEY_WAYPOINT)
        return fail(BLISSGPU_ERR_INVALID, who, "a gate cannot be combined with the waypoint mode");
    if (gate != BLISSGPU_GATE_NONE && gate_feature >= d) return fail(BLISSGPU_ERR_INVALID, who, "gate_feature must be below d");
    if (mode == BLISSGPU_JOURNEY_WAYPOINT && !to) return fail(BLISSGPU_ERR_INVALID, who, "the waypoint mode needs to");
    if (mode != BLISSGPU_JOURNEY_WAYPOINT && to) return fail(BLISSGPU_ERR_INVALID, who, "to must be NULL unless the mode is waypoint");
    if (n_journeys == 0) return BLISSGPU_OK;
    if (!from) return fail(BLISSGPU_ERR_INVALID, who, "from is NULL");
    if (n && !cand) return fail(BLISSGPU_ERR_INVALID, who, "cand is NULL");
    if (!idx) return fail(BLISSGPU_ERR_INVALID, who, "idx is NULL");
    return BLISSGPU_OK;
}

int blissgpu_journeys_device(blissgpu_ctx* c, const float* d_from, const float* d_to, uint64_t n_journeys, const float* d_cand,
                             uint64_t n, uint32_t d, int metric, const float* d_M, const uint32_t* d_skip, uint32_t k, int mode,
                             int gate, uint32_t gate_feature, uint32_t* d_idx, float* d_dist) {
    const char* who = "blissgpu_journeys_device";
    int rc = journeys_args_ok(who, d_from, d_to, n_journeys, d_cand, n, d, metric, d_M, k, mode, gate, gate_feature, d_idx);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_journeys == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // pl_chain: minima u64[G] | flags u32[4] ([0] NaN on a journey)
    const size_t G = (size_t)n_journeys, out_n = G * k;
    rc = c->pl_chain.ensure(G * sizeof(unsigned long long) + 4 * sizeof(uint32_t));
    if (rc) return rc;
    unsigned long long* best = reinterpret_cast<unsigned long long*>(c->pl_chain.p);
    uint32_t* flags = reinterpret_cast<uint32_t*>(c->pl_chain.p + G * sizeof(unsigned long long));
    // every row: 0xFFFFFFFF / +inf until a step writes it
    HIP_TRY(hipMemsetAsync(d_idx, 0xFF, out_n * sizeof(uint32_t), c->stream));
    if (d_dist) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_dist, 0x7F800000, out_n, c->stream));
    HIP_TRY(hipMemsetAsync(flags, 0, 4 * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(best, 0xFF, G * sizeof(unsigned long long), c->stream));
    const ChainPlan plan = chain_plan(n_journeys, n, c->n_cus);
    const uint32_t steps = (uint32_t)std::min<uint64_t>(k, n);  // (a journey is no longer than the candidates)
    for (uint32_t t = 0; t < steps; t++) {
        const JourneyStep j{d_from, d_to, (float)(t + 1u) / (float)(k + 1u), gate, gate != BLISSGPU_GATE_NONE ? gate_feature : 0u};
        Prof p(c, KX_JOURNEY_STEP);
        launch_journey_step(d_cand, (uint32_t)n, d, metric, d_M, diag, d_skip, (uint32_t)n_journeys, k, t, plan, j, d_idx, d_dist, best,
                            flags, c->stream);
    }
    HIP_TRY(hipGetLastError());
    uint32_t h_flags[4];
    if ((rc = read_flags(c, flags, 4, h_flags))) return rc;
    if (h_flags[0]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance");
    return BLISSGPU_OK;
}

int blissgpu_journeys(const float* from, const float* to, uint64_t n_journeys, const float* cand, uint64_t n, uint32_t d, int metric,
                      const float* M, const uint32_t* skip, uint32_t k, int mode, int gate, uint32_t gate_feature, uint32_t* idx,
                      float* dist) {
    const char* who = "blissgpu_journeys";
    int rc = journeys_args_ok(who, from, to, n_journeys, cand, n, d, metric, M, k, mode, gate, gate_feature, idx);
    if (rc) return rc;
    if (n_journeys == 0) return BLISSGPU_OK;
    if ((rc = skip_entries_ok(who, skip, 2 * n_journeys, n))) return rc;
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    const size_t G = (size_t)n_journeys, out_n = G * k, row_n = G * d;
    const float* dM = nullptr;
    rc = c->st_b.ensure(std::max<size_t>(1, n * d));
    if (!rc) rc = c->st_a.ensure(row_n * (to ? 2 : 1));  // from, then to
    if (!rc) rc = c->st_idx.ensure(out_n + (skip ? 2 * G : 0));
    if (!rc && dist) rc = c->st_dist.ensure(out_n);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    uint32_t *d_idx = c->st_idx.p, *d_skip = skip ? c->st_idx.p + out_n : nullptr;
    HostStage s{c, "journeys"};
    s.up(c->st_b.p, cand, n * d * sizeof(float));
    s.up(c->st_a.p, from, row_n * sizeof(float));
    s.up(c->st_a.p + row_n, to, row_n * sizeof(float));
    s.up(d_skip, skip, 2 * G * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc)
        rc = blissgpu_journeys_device(c, c->st_a.p, to ? c->st_a.p + row_n : nullptr, n_journeys, c->st_b.p, n, d, metric, dM, d_skip, k,
                                      mode, gate, gate_feature, d_idx, dist ? c->st_dist.p : nullptr);
    if (!rc) {
        s.down(idx, d_idx, out_n * sizeof(uint32_t));
        s.down(dist, c->st_dist.p, out_n * sizeof(float));
    }
    return s.finish(rc);
}

// ---- radio playlists: chains (or the k nearest of the start song) under label rules -- no artist twice within w tracks, no
// album twice within w tracks, at most c songs per artist (kernels_radio.hip) ----
// everything that can be said about the arguments without a device (both forms check it BEFORE the device is touched)
static int radio_args_ok(const char* who, const void* from, uint64_t n_radios, const void* cand, uint64_t n, uint32_t d, int metric,
                         const float* M, const void* labels, uint32_t n_rules, const uint32_t* window, const uint32_t* limit,
                         uint32_t k, int mode, const void* idx) {
    if (k == 0 || k > BLISSGPU_KNN_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KNN_MAX_K");
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 candidates");
    if (n_radios >= 0x80000000ull) return fail(BLISSGPU_ERR_INVALID, who, "n_radios must be below 2^31");
    if (mode != BLISSGPU_RADIO_CHAIN && mode != BLISSGPU_RADIO_NEAREST) return fail(BLISSGPU_ERR_INVALID, who, "unknown mode");
    if (n_rules > BLISSGPU_RADIO_MAX_RULES) return fail(BLISSGPU_ERR_INVALID, who, "n_rules must be at most BLISSGPU_RADIO_MAX_RULES");
    if (n_rules) {
        if (!window) return fail(BLISSGPU_ERR_INVALID, who, "window is NULL");
        if (!limit) return fail(BLISSGPU_ERR_INVALID, who, "limit is NULL");
        if (!labels) return fail(BLISSGPU_ERR_INVALID, who, "labels is NULL");
        for (uint32_t r = 0; r < n_rules; r++)
            if (limit[r] == 0) return fail(BLISSGPU_ERR_INVALID, who, "limit must be at least 1");
    }
    if (n_radios == 0) return BLISSGPU_OK;
    if (!from) return fail(BLISSGPU_ERR_INVALID, who, "from is NULL");
    if (n && !cand) return fail(BLISSGPU_ERR_INVALID, who, "cand is NULL");
    if (!idx) return fail(BLISSGPU_ERR_INVALID, who, "idx is NULL");
    return BLISSGPU_OK;
}

// the rules that can ban anything in a list of k songs: window >= 1 (cut to k + 1: the whole list and the start) and
// limit <= min(window, k), the most history positions a step's window holds
static RadioRules radio_rules(uint32_t n_rules, const uint32_t* window, const uint32_t* limit, uint32_t k) {
    RadioRules r{};
    r.n_total = n_rules;
    r.cap = 1;
    for (uint32_t i = 0; i < n_rules; i++) {
        const uint32_t w = std::min(window[i], k + 1u), most = std::min(w, k);
        if (w == 0 || limit[i] > most) continue;
        r.rule[r.n] = i;
        r.window[r.n] = w;
        r.limit[r.n] = limit[i];
        r.cap = std::max(r.cap, most / limit[i]);
        r.n++;
    }
    return r;
}

int blissgpu_radio_device(blissgpu_ctx* c, const float* d_from, uint64_t n_radios, const float* d_cand, uint64_t n, uint32_t d,
                          int metric, const float* d_M, const uint32_t* d_labels, const uint32_t* d_from_labels, uint32_t n_rules,
                          const uint32_t* window, const uint32_t* limit, const uint32_t* d_skip, uint32_t k, int mode,
                          uint32_t* d_idx, float* d_dist) {
    const char* who = "blissgpu_radio_device";
    int rc = radio_args_ok(who, d_from, n_radios, d_cand, n, d, metric, d_M, d_labels, n_rules, window, limit, k, mode, d_idx);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_radios == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    const RadioRules rules = radio_rules(n_rules, window, limit, k);
    // pl_chain: minima u64[G] | flags u32[4] ([0] NaN) | ban counts u32[G * rules] | banned labels u32[G * rules * cap]
    const uint64_t G = n_radios, out_n = G * k, work = G * rules.n;
    const uint64_t bytes = G * sizeof(unsigned long long) + 4 * sizeof(uint32_t) + (work + work * rules.cap) * sizeof(uint32_t);
    if (bytes > c->ws_limit) return fail(BLISSGPU_ERR_OOM, who, "the banned labels of every radio do not fit the workspace limit");
    rc = c->pl_chain.ensure((size_t)bytes);
    if (rc) return rc;
    unsigned long long* best = reinterpret_cast<unsigned long long*>(c->pl_chain.p);
    uint32_t* flags = reinterpret_cast<uint32_t*>(c->pl_chain.p + G * sizeof(unsigned long long));
    uint32_t* ban_cnt = flags + 4;
    uint32_t* ban = ban_cnt + work;
    // every row: 0xFFFFFFFF / +inf until a step writes it
    HIP_TRY(hipMemsetAsync(d_idx, 0xFF, out_n * sizeof(uint32_t), c->stream));
    if (d_dist) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_dist, 0x7F800000, out_n, c->stream));
    HIP_TRY(hipMemsetAsync(flags, 0, 4 * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(best, 0xFF, G * sizeof(unsigned long long), c->stream));
    const ChainPlan plan = chain_plan(n_radios, n, c->n_cus);
    const RadioArgs a{d_cand, (uint32_t)n, d, metric, d_M, diag, d_from, d_skip, d_labels, d_from_labels, rules, ban, ban_cnt,
                      mode == BLISSGPU_RADIO_NEAREST, (uint32_t)n_radios, k, d_idx, d_dist, best, flags};
    const uint32_t steps = (uint32_t)std::min<uint64_t>(k, n);  // (a radio is no longer than the candidates)
    for (uint32_t t = 0; t < steps; t++) {
        if (rules.n) {
            Prof p(c, KX_RADIO_BAN);
            launch_radio_ban(a, t, c->stream);
        }
        Prof p(c, KX_RADIO_STEP);
        launch_radio_step(a, t, plan, c->stream);
    }
    HIP_TRY(hipGetLastError());
    uint32_t h_flags[4];
    if ((rc = read_flags(c, flags, 4, h_flags))) return rc;
    if (h_flags[0]) return fail(BLISSGPU_ERR_NAN, who, "NaN distance");
    return BLISSGPU_OK;
}

int blissgpu_radio(const float* from, uint64_t n_radios, const float* cand, uint64_t n, uint32_t d, int metric, const float* M,
                   const uint32_t* labels, const uint32_t* from_labels, uint32_t n_rules, const uint32_t* window,
                   const uint32_t* limit, const uint32_t* skip, uint32_t k, int mode, uint32_t* idx, float* dist) {
    const char* who = "blissgpu_radio";
    int rc = radio_args_ok(who, from, n_radios, cand, n, d, metric, M, labels, n_rules, window, limit, k, mode, idx);
    if (rc) return rc;
    if (n_radios == 0) return BLISSGPU_OK;
    if ((rc = skip_entries_ok(who, skip, 2 * n_radios, n))) return rc;
    if (n == 0) {  // no candidate: every row is padding, and no device is needed to say so
        std::fill(idx, idx + (size_t)n_radios * k, 0xFFFFFFFFu);
        if (dist) std::fill(dist, dist + (size_t)n_radios * k, INFINITY);
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    // start rows that ARE the candidate matrix travel once
    const bool shared = (const void*)from == (const void*)cand && n_radios <= n;
    const size_t G = (size_t)n_radios, out_n = G * k, row_n = G * d;
    const size_t lab_n = (size_t)n_rules * n, fl_n = from_labels ? G * n_rules : 0;
    const float* dM = nullptr;
    rc = c->st_b.ensure(std::max<size_t>(1, n * d));
    if (!rc && !shared) rc = c->st_a.ensure(row_n);
    if (!rc) rc = c->st_idx.ensure(out_n + (skip ? 2 * G : 0) + lab_n + fl_n);  // idx | skip | labels | from_labels
    if (!rc && dist) rc = c->st_dist.ensure(out_n);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    uint32_t *d_idx = c->st_idx.p, *d_skip = skip ? c->st_idx.p + out_n : nullptr;
    uint32_t* d_lab = c->st_idx.p + out_n + (skip ? 2 * G : 0);
    uint32_t* d_fl = d_lab + lab_n;
    HostStage s{c, "radio"};
    s.up(c->st_b.p, cand, n * d * sizeof(float));
    if (!shared) s.up(c->st_a.p, from, row_n * sizeof(float));
    s.up(d_skip, skip, 2 * G * sizeof(uint32_t));
    s.up(d_lab, labels, lab_n * sizeof(uint32_t));
    s.up(d_fl, from_labels, fl_n * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc)
        rc = blissgpu_radio_device(c, shared ? c->st_b.p : c->st_a.p, n_radios, c->st_b.p, n, d, metric, dM, n_rules ? d_lab : nullptr,
                                   fl_n ? d_fl : nullptr, n_rules, window, limit, d_skip, k, mode, d_idx,
                                   dist ? c->st_dist.p : nullptr);
    if (!rc) {
        s.down(idx, d_idx, out_n * sizeof(uint32_t));
        s.down(dist, c->st_dist.p, out_n * sizeof(float));
    }
    return s.finish(rc);
}

// ---- the 2-D map of a library: exact t-SNE gradients and the momentum / gain loop around them (kernels_map.hip, DESIGN.md
// 3.31).  Host-pointer forms only; map_step_core / map_layout_core take the context and device pointers, so a device-pointer
// form is an export away ----
int blissgpu_map_plan(uint64_t n, uint32_t n_cus, uint32_t* col_groups) {
    const char* who = "blissgpu_map_plan";
    if (!col_groups) return fail(BLISSGPU_ERR_INVALID, who, "col_groups is NULL");
    if (n >= (1ull << 24)) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^24 rows");
    *col_groups = map_plan_col_groups(n, (int)std::min<uint32_t>(n_cus, 1u << 20));
    return BLISSGPU_OK;
}

// everything that can be said about y and the CSR arrays in host memory; long_rows: the rows of more than MAP_LONG_ROW entries
static int map_input_ok(const char* who, const float* y, uint64_t n, const uint64_t* row_offsets, const uint32_t* cols, const float* vals,
                        uint32_t col_groups, std::vector<uint32_t>* long_rows) {
    if (n >= (1ull << 24)) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^24 rows");
    if (col_groups > MAP_MAX_COL_GROUPS) return fail(BLISSGPU_ERR_INVALID, who, "col_groups must be 0 .. 64");
    if (n == 0) return BLISSGPU_OK;
    if (!y) return fail(BLISSGPU_ERR_INVALID, who, "y is NULL");
    if (!row_offsets) return fail(BLISSGPU_ERR_INVALID, who, "row_offsets is NULL");
    if (row_offsets[0] != 0) return fail(BLISSGPU_ERR_INVALID, who, "row_offsets[0] must be 0");
    for (uint64_t i = 0; i < n; i++)
        if (row_offsets[i + 1] < row_offsets[i]) return fail(BLISSGPU_ERR_INVALID, who, "row_offsets must not decrease");
    const uint64_t nnz = row_offsets[n];
    if (nnz >= (1ull << 32)) return fail(BLISSGPU_ERR_INVALID, who, "nnz must be below 2^32 entries");
    if (nnz && !cols) return fail(BLISSGPU_ERR_INVALID, who, "cols is NULL");
    if (nnz && !vals) return fail(BLISSGPU_ERR_INVALID, who, "vals is NULL");
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t e0 = row_offsets[i], e1 = row_offsets[i + 1];
        for (uint64_t e = e0; e < e1; e++) {
            if (cols[e] >= n) return fail(BLISSGPU_ERR_INVALID, who, "a column index is >= n");
            if (cols[e] == i) return fail(BLISSGPU_ERR_INVALID, who, "a row holds itself");
            if (e > e0 && cols[e] <= cols[e - 1]) return fail(BLISSGPU_ERR_INVALID, who, "a row's columns must be strictly ascending");
            if (!(vals[e] >= 0.0f) || !std::isfinite(vals[e])) return fail(BLISSGPU_ERR_INVALID, who, "vals must be finite and >= 0");
        }
        if (e1 - e0 > MAP_LONG_ROW) long_rows->push_back((uint32_t)i);
    }
    return BLISSGPU_OK;
}

// how the scan is fed y_j (for the bench tool: no bit of the result depends on it)
static int map_feed() {
    const char* e = getenv("BLISSGPU_MAP_FEED");
    if (e && !strcmp(e, "scalar")) return MAP_FEED_SCALAR;
    return MAP_FEED_LDS;  // the measured choice
}

// the scratch of the gradient: col_groups == 0 resolved, the plan, and sums | part | zb | att | U | gain carved out of map_ws;
// counted against the workspace limit together with the trace the caller keeps on the device (trace_doubles)
static int map_scratch(blissgpu_ctx* c, const char* who, uint32_t col_groups, size_t trace_doubles, MapArgs* a, MapPlan* plan) {
    const size_t n = a->n;
    *plan = map_plan(n, col_groups ? col_groups : map_plan_col_groups(n, c->n_cus));
    const size_t part = plan->chunks > 1 ? (size_t)plan->chunks * 3 * n : 0;
    const size_t doubles = 3 * n + part + plan->blocks + 6 * n;
    if ((doubles + trace_doubles) * sizeof(double) > c->ws_limit)
        return fail(BLISSGPU_ERR_OOM, who, "the column groups' partial sums and the trace do not fit the workspace limit");
    int rc = c->map_ws.ensure(doubles * sizeof(double));
    if (rc) return rc;
    double* w = reinterpret_cast<double*>(c->map_ws.p);
    a->sums = w;
    a->part = w + 3 * n;
    a->zb = a->part + part;
    a->att = a->zb + plan->blocks;
    a->U = a->att + 2 * n;
    a->gain = a->U + 2 * n;
    return BLISSGPU_OK;
}

// one gradient evaluation and what follows it (a.grad: stored; else the update), queued on the context's stream
static void map_eval(blissgpu_ctx* c, const MapArgs& a, const MapPlan& plan, int feed) {
    { Prof p(c, KX_MAP_REPULSE); launch_map_repulse(a, plan, feed, c->stream); }
    { Prof p(c, KX_MAP_ATTRACT); launch_map_attract(a, plan, c->stream); }
    if (a.n_long) { Prof p(c, KX_MAP_ATTRACT); launch_map_attract_long(a, c->stream); }
    { Prof p(c, KX_MAP_UPDATE); launch_map_update(a, plan, c->stream); }
}

// The cores, on device pointers (a: Y, the CSR, the long rows, n >= 2).  Neither synchronises.
static int map_step_core(blissgpu_ctx* c, const char* who, MapArgs a, float exaggeration, uint32_t col_groups, double* d_grad,
                         double* d_z_rows, double* d_Z) {
    MapPlan plan;
    int rc = map_scratch(c, who, col_groups, 0, &a, &plan);
    if (rc) return rc;
    a.grad = d_grad;
    a.z_out = d_Z;
    a.exaggeration = (double)exaggeration;
    map_eval(c, a, plan, map_feed());
    HIP_TRY(hipGetLastError());
    if (d_z_rows) HIP_TRY(hipMemcpyAsync(d_z_rows, a.sums, (size_t)a.n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return BLISSGPU_OK;
}

static int map_layout_core(blissgpu_ctx* c, const char* who, MapArgs a, uint32_t n_iter, uint32_t exag_iters, float exaggeration,
                           double lr, double momentum0, double momentum1, double min_gain, uint32_t col_groups, double* d_trace) {
    MapPlan plan;
    int rc = map_scratch(c, who, col_groups, n_iter, &a, &plan);
    if (rc) return rc;
    const int feed = map_feed();
    a.grad = nullptr;
    a.lr = lr;
    a.min_gain = min_gain;
    for (uint32_t it = 0; it < n_iter; it++) {  // no host synchronisation in here
        a.exaggeration = it < exag_iters ? (double)exaggeration : 1.0;
        a.momentum = it < exag_iters ? momentum0 : momentum1;
        a.first = it == 0;
        a.z_out = d_trace + it;
        map_eval(c, a, plan, feed);
    }
    HIP_TRY(hipGetLastError());
    return BLISSGPU_OK;
}

// y | vals in st_b, cols | long rows in st_idx, row_offsets and `extra` doubles behind them in st_out
static int map_stage(blissgpu_ctx* c, HostStage& s, const float* y, uint64_t n, const uint64_t* row_offsets, const uint32_t* cols,
                     const float* vals, const std::vector<uint32_t>& long_rows, size_t extra, MapArgs* a, double** d_extra) {
    const size_t nnz = row_offsets[n];
    int rc = c->st_b.ensure(2 * n + nnz);
    if (!rc) rc = c->st_idx.ensure(std::max<size_t>(1, nnz + long_rows.size()));
    if (!rc) rc = c->st_out.ensure((n + 1 + extra) * sizeof(double));
    if (rc) return rc;
    *a = MapArgs{};
    a->Y = c->st_b.p;
    float* d_vals = c->st_b.p + 2 * n;
    uint32_t *d_cols = c->st_idx.p, *d_long = c->st_idx.p + nnz;
    unsigned long long* d_ro = reinterpret_cast<unsigned long long*>(c->st_out.p);
    a->row_offsets = d_ro;
    a->cols = d_cols;
    a->vals = d_vals;
    a->long_rows = d_long;
    a->n = (uint32_t)n;
    a->n_long = (uint32_t)long_rows.size();
    *d_extra = reinterpret_cast<double*>(d_ro + n + 1);
    s.up(a->Y, y, 2 * n * sizeof(float));
    s.up(d_vals, vals, nnz * sizeof(float));
    s.up(d_cols, cols, nnz * sizeof(uint32_t));
    s.up(d_long, long_rows.data(), long_rows.size() * sizeof(uint32_t));
    s.up(d_ro, row_offsets, (n + 1) * sizeof(uint64_t));
    return s.uploaded();
}

int blissgpu_map_step(const float* y, uint64_t n, const uint64_t* row_offsets, const uint32_t* cols, const float* vals,
                      float exaggeration, uint32_t col_groups, double* grad, double* z_rows, double* Z) {
    const char* who = "blissgpu_map_step";
    if (!std::isfinite(exaggeration)) return fail(BLISSGPU_ERR_INVALID, who, "exaggeration must be finite");
    std::vector<uint32_t> long_rows;
    int rc = map_input_ok(who, y, n, row_offsets, cols, vals, col_groups, &long_rows);
    if (rc) return rc;
    if (!Z) return fail(BLISSGPU_ERR_INVALID, who, "Z is NULL");
    if (n && !grad) return fail(BLISSGPU_ERR_INVALID, who, "grad is NULL");
    if (n < 2) {  // no pair: nothing for a device to do
        *Z = 0.0;
        for (uint64_t e = 0; e < 2 * n; e++) grad[e] = 0.0;
        if (z_rows && n) z_rows[0] = 0.0;
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    HostStage s{c, "map_step"};
    MapArgs a;
    double* d_out;  // grad [n][2] | z_rows [n] | Z
    rc = map_stage(c, s, y, n, row_offsets, cols, vals, long_rows, 3 * n + 1, &a, &d_out);
    if (!rc) rc = map_step_core(c, who, a, exaggeration, col_groups, d_out, z_rows ? d_out + 2 * n : nullptr, d_out + 3 * n);
    if (!rc) {
        s.down(grad, d_out, 2 * n * sizeof(double));
        s.down(z_rows, d_out + 2 * n, n * sizeof(double));
        s.down(Z, d_out + 3 * n, sizeof(double));
    }
    return s.finish(rc);
}

int blissgpu_map_layout(const float* y0, uint64_t n, const uint64_t* row_offsets, const uint32_t* cols, const float* vals,
                        uint32_t n_iter, uint32_t exag_iters, float exaggeration, double learning_rate, double momentum0,
                        double momentum1, double min_gain, uint32_t col_groups, float* y_out, double* z_trace) {
    const char* who = "blissgpu_map_layout";
    if (!std::isfinite(exaggeration) || !std::isfinite(learning_rate) || !std::isfinite(momentum0) || !std::isfinite(momentum1) ||
        !std::isfinite(min_gain))
        return fail(BLISSGPU_ERR_INVALID, who, "exaggeration, learning_rate, the momenta and min_gain must be finite");
    std::vector<uint32_t> long_rows;
    int rc = map_input_ok(who, y0, n, row_offsets, cols, vals, col_groups, &long_rows);
    if (rc) return rc;
    if (n == 0) return BLISSGPU_OK;
    if (!y_out) return fail(BLISSGPU_ERR_INVALID, who, "y_out is NULL");
    if (n < 2 || n_iter == 0) {  // no pair (every gradient is 0, every Z is 0) or no iteration: y_out = y0
        if (y_out != y0) memmove(y_out, y0, 2 * n * sizeof(float));
        if (z_trace) for (uint32_t it = 0; it < n_iter; it++) z_trace[it] = 0.0;
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    HostStage s{c, "map_layout"};
    MapArgs a;
    double* d_trace;
    // (checked here as well as in the core: the trace is staged before the core runs)
    if (((size_t)n_iter + 9 * n) * sizeof(double) > c->ws_limit)
        return fail(BLISSGPU_ERR_OOM, who, "the column groups' partial sums and the trace do not fit the workspace limit");
    std::vector<double> trace;
    if (!z_trace) {
        try {
            trace.resize(n_iter);
        } catch (const std::bad_alloc&) {
            return fail(BLISSGPU_ERR_OOM, who, "no host memory for the trace");
        }
    }
    double* h_trace = z_trace ? z_trace : trace.data();
    rc = map_stage(c, s, y0, n, row_offsets, cols, vals, long_rows, n_iter, &a, &d_trace);
    if (!rc) rc = map_layout_core(c, who, a, n_iter, exag_iters, exaggeration, learning_rate, momentum0, momentum1, min_gain, col_groups, d_trace);
    if (!rc) {
        s.down(y_out, a.Y, 2 * n * sizeof(float));
        s.down(h_trace, d_trace, (size_t)n_iter * sizeof(double));
    }
    if ((rc = s.finish(rc))) return rc;  // the one synchronisation
    for (uint32_t it = 0; it < n_iter; it++)
        if (!std::isfinite(h_trace[it]) || !(h_trace[it] > 0.0)) return fail(BLISSGPU_ERR_NAN, who, "the normaliser Z of an iteration is not finite and positive");
    return BLISSGPU_OK;
}

// ---- duplicate groups of a collection: the rule of dedup_playlist_custom_distance (src/playlist.rs:381-388) over EVERY pair
// i < j of the rows, and the connected components of those edges ----
// everything that can be said about the arguments without a device (both forms check it BEFORE the device is touched)
static int dup_args_ok(const char* who, const void* x, uint64_t n, uint32_t d, int metric, const float* M, float threshold,
                       const void* label, const void* n_pairs) {
    if (d == 0 || d > 64) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. 64");
    if (metric < 0 || metric > 2) return fail(BLISSGPU_ERR_INVALID, who, "unknown metric");
    if (metric == BLISSGPU_METRIC_MAHALANOBIS && !M) return fail(BLISSGPU_ERR_INVALID, who, "mahalanobis needs M");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 rows");
    if (threshold != threshold) return fail(BLISSGPU_ERR_INVALID, who, "threshold is NaN");
    if (!n_pairs) return fail(BLISSGPU_ERR_INVALID, who, "n_pairs is NULL");
    if (n && !x) return fail(BLISSGPU_ERR_INVALID, who, "x is NULL");
    if (n && !label) return fail(BLISSGPU_ERR_INVALID, who, "label is NULL");
    return BLISSGPU_OK;
}

int blissgpu_duplicate_groups_device(blissgpu_ctx* c, const float* d_x, uint64_t n, uint32_t d, const uint32_t* d_meta,
                                     int metric, const float* d_M, float threshold, uint32_t* d_label, uint64_t* d_n_pairs,
                                     uint32_t* d_pairs, float* d_pair_dist, uint64_t max_pairs) {
    const char* who = "blissgpu_duplicate_groups_device";
    int rc = dup_args_ok(who, d_x, n, d, metric, d_M, threshold, d_label, d_n_pairs);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    CTX_ENTER(c, who);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_n_pairs, 0, sizeof(uint64_t), c->stream));
        return BLISSGPU_OK;
    }
    int diag = 0;
    if (int e = metric_is_diag(c, d_M, d, metric, &diag)) return e;
    // workspace: none but the caller's label array (the union-find's parents) and pair buffer, and eight words of the context
    // -- pl_sync: [1] NaN among the distances of the pairs i < j, [4..5] the pair list's cursor
    rc = c->pl_sync.ensure(8);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 8 * sizeof(uint32_t), c->stream));
    unsigned long long* cursor = reinterpret_cast<unsigned long long*>(c->pl_sync.p + 4);
    unsigned long long* np = reinterpret_cast<unsigned long long*>(d_n_pairs);
    if (!d_pairs || max_pairs == 0) {
        d_pairs = nullptr;
        d_pair_dist = nullptr;
        max_pairs = 0;
    }
    const DupPlan plan = dup_plan(n, c->n_cus);
    {
        Prof p(c, K_DUP_INIT);
        launch_dup_init(d_label, (uint32_t)n, np, cursor, c->stream);
    }
    HIP_TRY(hipGetLastError());
    {
        Prof p(c, K_DUP_JOIN);
        launch_dup_join(d_x, (uint32_t)n, d, metric, d_M, diag, d_meta, threshold, plan, d_label, np, cursor, d_pairs, d_pair_dist,
                        max_pairs, c->pl_sync.p + 1, c->stream);
    }
    HIP_TRY(hipGetLastError());
    {
        Prof p(c, K_DUP_FLATTEN);
        launch_dup_flatten(d_label, (uint32_t)n, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return nan_check(c, c->pl_sync.p + 1, who);
}

int blissgpu_duplicate_groups(const float* x, uint64_t n, uint32_t d, const uint32_t* meta, int metric, const float* M,
                              float threshold, uint32_t* label, uint64_t* n_pairs, uint32_t* pairs, float* pair_dist,
                              uint64_t max_pairs) {
    const char* who = "blissgpu_duplicate_groups";
    int rc = dup_args_ok(who, x, n, d, metric, M, threshold, label, n_pairs);
    if (rc) return rc;
    *n_pairs = 0;
    if (n == 0) return BLISSGPU_OK;
    blissgpu_ctx* c;
    rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    if (!pairs) max_pairs = 0;
    // st_idx: n_pairs (two words) | label[n] | meta[n] | pairs[max_pairs][2]
    const size_t o_label = 2, o_meta = o_label + n, o_pairs = o_meta + (meta ? n : 0);
    const float* dM = nullptr;
    rc = c->st_b.ensure(n * d);
    if (!rc) rc = c->st_idx.ensure(o_pairs + 2 * max_pairs);
    if (!rc && pair_dist && max_pairs) rc = c->st_dist.ensure(max_pairs);
    if (!rc) rc = stage_matrix(c, M, d, metric, &dM);
    if (rc) return rc;
    uint32_t* idx = c->st_idx.p;
    float* d_dist = (pair_dist && max_pairs) ? c->st_dist.p : nullptr;
    HostStage s{c, "duplicates"};
    s.up(c->st_b.p, x, n * d * sizeof(float));
    s.up(idx + o_meta, meta, n * sizeof(uint32_t));
    rc = s.uploaded();
    if (!rc)
        rc = blissgpu_duplicate_groups_device(c, c->st_b.p, n, d, meta ? idx + o_meta : nullptr, metric, dM, threshold,
                                              idx + o_label, reinterpret_cast<uint64_t*>(idx), max_pairs ? idx + o_pairs : nullptr,
                                              d_dist, max_pairs);
    if (!rc) {  // the device form has synchronised: the count is there
        uint64_t np = 0;
        s.down(&np, idx, sizeof(np));
        s.down(label, idx + o_label, n * sizeof(uint32_t));
        rc = s.landed();
        if (!rc && np && np <= max_pairs) {
            // the list in ascending (i, j): the device appends in the order the wavefronts meet the edges
            std::vector<uint32_t> hp(2 * np);
            std::vector<float> hd(d_dist ? np : 0);
            s.down(hp.data(), idx + o_pairs, hp.size() * sizeof(uint32_t));
            s.down(d_dist ? hd.data() : nullptr, d_dist, np * sizeof(float));
            rc = s.landed();
            if (!rc) {
                std::vector<uint64_t> at(np);
                for (uint64_t k = 0; k < np; k++) at[k] = k;
                std::sort(at.begin(), at.end(), [&](uint64_t a, uint64_t b) {
                    return hp[2 * a] != hp[2 * b] ? hp[2 * a] < hp[2 * b] : hp[2 * a + 1] < hp[2 * b + 1];
                });
                for (uint64_t k = 0; k < np; k++) {
                    pairs[2 * k] = hp[2 * at[k]];
                    pairs[2 * k + 1] = hp[2 * at[k] + 1];
                    if (d_dist) pair_dist[k] = hd[at[k]];
                }
            }
        }
        if (!rc) *n_pairs = np;
    }
    return s.finish(rc);
}

// ---- extended isolation forest (ForestOptions, src/playlist.rs:230-251): build / info / export are host-only ----
int blissgpu_forest_build(const float* seeds, uint64_t n_seeds, uint32_t d, uint32_t n_trees, uint32_t sample_size,
                          uint32_t max_tree_depth, uint32_t extension_level, uint64_t seed, void** forest) {
    if (!forest) return fail(BLISSGPU_ERR_INVALID, "blissgpu_forest_build", "NULL argument");
    *forest = nullptr;
    Forest* f = nullptr;
    int rc = forest_build(seeds, n_seeds, d, n_trees, sample_size, max_tree_depth, extension_level, seed, &f);
    if (!rc) *forest = f;
    return rc;
}

int blissgpu_forest_destroy(void* forest) {
    forest_destroy(static_cast<Forest*>(forest));
    return BLISSGPU_OK;
}

int blissgpu_forest_info(const void* forest, uint32_t* d, uint32_t* n_trees, uint32_t* psi, uint32_t* depth_limit,
                         uint32_t* extension_level, uint64_t* n_nodes) {
    if (!forest) return fail(BLISSGPU_ERR_INVALID, "blissgpu_forest_info", "forest is NULL");
    const Forest* f = static_cast<const Forest*>(forest);
    if (d) *d = f->d;
    if (n_trees) *n_trees = f->n_trees;
    if (psi) *psi = f->psi;
    if (depth_limit) *depth_limit = f->limit;
    if (extension_level) *extension_level = f->ext;
    if (n_nodes) *n_nodes = f->right.size();
    return BLISSGPU_OK;
}

int blissgpu_forest_export(const void* forest, uint32_t* sample_idx, uint64_t* tree_first, float* normal, float* b, uint32_t* left,
                           uint32_t* right, uint32_t* leaf_size, uint32_t* leaf_q) {
    if (!forest) return fail(BLISSGPU_ERR_INVALID, "blissgpu_forest_export", "forest is NULL");
    forest_export(static_cast<const Forest*>(forest), sample_idx, tree_first, normal, b, left, right, leaf_size, leaf_q);
    return BLISSGPU_OK;
}

// everything that can be said about a scoring call without a device
static int forest_args_ok(const char* who, const void* forest, const void* cand, uint64_t n, const void* out) {
    if (!forest) return fail(BLISSGPU_ERR_INVALID, who, "forest is NULL");
    if (n > 0xFFFFFF00ull) return fail(BLISSGPU_ERR_INVALID, who, "more than 0xFFFFFF00 candidates");
    if (n && (!cand || !out)) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    return BLISSGPU_OK;
}

// walk + finish on the context's stream: d_sum (may be NULL: context scratch), d_score (may be NULL), keys / idx (both or none)
static int forest_run(blissgpu_ctx* c, Forest* f, const float* d_cand, uint32_t n, float* d_score, uint64_t* d_sum, uint32_t* keys,
                      uint32_t* idx, const char* who) {
    const ForestImage* im = nullptr;
    int rc = forest_device_image(f, c->device, c->stream, &im);
    if (rc) return rc;
    if (!d_sum) {
        if ((rc = c->pl_slots.ensure(n))) return rc;
        d_sum = reinterpret_cast<uint64_t*>(c->pl_slots.p);
    }
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(d_sum);
    const uint32_t split = forest_split_plan(f, n, c->n_cus, c->forest_split);
    if (split > 1) HIP_TRY(hipMemsetAsync(sum, 0, (size_t)n * sizeof(unsigned long long), c->stream));
    {
        Prof p(c, K_FOREST_WALK);
        HIP_TRY(launch_forest_walk(f, *im, d_cand, n, split, !c->forest_global, sum, c->stream));
    }
    {
        Prof p(c, K_FOREST_FINISH);
        launch_forest_finish(f, sum, n, d_score, keys, idx, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return BLISSGPU_OK;
}

int blissgpu_forest_score_device(blissgpu_ctx* c, void* forest, const float* d_cand, uint64_t n, float* d_score,
                                 uint64_t* d_path_sum) {
    const char* who = "blissgpu_forest_score_device";
    int rc = forest_args_ok(who, forest, d_cand, n, d_score);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    return forest_run(c, static_cast<Forest*>(forest), d_cand, (uint32_t)n, d_score, d_path_sum, nullptr, nullptr, who);
}

int blissgpu_forest_closest_to_songs_device(blissgpu_ctx* c, void* forest, const float* d_cand, uint64_t n, uint32_t* d_order,
                                            float* d_score) {
    const char* who = "blissgpu_forest_closest_to_songs_device";
    int rc = forest_args_ok(who, forest, d_cand, n, d_order);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    const uint32_t n32 = (uint32_t)n;
    size_t tmp_bytes = 0;
    HIP_TRY(sort_pairs_u32(nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, n32, c->stream));
    rc = c->pl_sync.ensure(4);
    if (!rc) rc = c->pl_keys.ensure((size_t)3 * n32);  // keys in | keys out | indices in
    if (!rc) rc = c->pl_tmp.ensure(tmp_bytes);
    if (rc) return rc;
    uint32_t *keys_in = c->pl_keys.p, *keys_out = keys_in + n32, *idx_in = keys_out + n32;
    HIP_TRY(hipMemsetAsync(c->pl_sync.p, 0, 4 * sizeof(uint32_t), c->stream));
    rc = forest_run(c, static_cast<Forest*>(forest), d_cand, n32, d_score, nullptr, keys_in, idx_in, who);
    if (rc) return rc;
    // the same stable radix sort as blissgpu_closest_to_songs_device (single launch only while its workgroups are co-resident)
    HIP_TRY(sort_pairs_u32(c->pl_tmp.p, &tmp_bytes, keys_in, keys_out, idx_in, d_order, n32, c->stream, c->pl_sync.p + 2,
                           live_contexts(c->device) <= 2 ? (uint32_t)std::max(1, c->n_cus) : 0u));
    return BLISSGPU_OK;
}

// host-pointer forms: candidates staged in st_b, results in st_dist (scores), st_out (path sums or the order)
static int forest_host(const char* who, void* forest, const float* cand, uint64_t n, float* score, uint64_t* path_sum,
                       uint32_t* order) {
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    Forest* f = static_cast<Forest*>(forest);
    rc = c->st_b.ensure(n * f->d);
    if (!rc) rc = c->st_dist.ensure(n);
    if (!rc) rc = c->st_out.ensure(n * sizeof(uint64_t));
    if (rc) return rc;
    HostStage s{c, "forest"};
    s.up(c->st_b.p, cand, n * f->d * sizeof(float));
    if ((rc = s.uploaded())) return rc;
    if (order) rc = blissgpu_forest_closest_to_songs_device(c, forest, c->st_b.p, n, reinterpret_cast<uint32_t*>(c->st_out.p), c->st_dist.p);
    else rc = blissgpu_forest_score_device(c, forest, c->st_b.p, n, c->st_dist.p, path_sum ? reinterpret_cast<uint64_t*>(c->st_out.p) : nullptr);
    if (!rc) {
        s.down(score, c->st_dist.p, n * sizeof(float));
        s.down(order, c->st_out.p, n * sizeof(uint32_t));
        s.down(path_sum, c->st_out.p, n * sizeof(uint64_t));
    }
    return s.finish(rc);
}

int blissgpu_forest_score(void* forest, const float* cand, uint64_t n, float* score, uint64_t* path_sum) {
    int rc = forest_args_ok("blissgpu_forest_score", forest, cand, n, score);
    if (rc || n == 0) return rc;
    return forest_host("blissgpu_forest_score", forest, cand, n, score, path_sum, nullptr);
}

int blissgpu_forest_closest_to_songs(void* forest, const float* cand, uint64_t n, uint32_t* order, float* score) {
    int rc = forest_args_ok("blissgpu_forest_closest_to_songs", forest, cand, n, order);
    if (rc || n == 0) return rc;
    return forest_host("blissgpu_forest_closest_to_songs", forest, cand, n, score, nullptr, order);
}

// ---- one forest per seed GROUP: the k lowest forest scores of every group in one call ----
// everything that can be said about the arguments without a device and without building a forest
static int group_forest_args_ok(const char* who, const float* h_seeds, bool seeds_given, const uint64_t* off, uint64_t n_groups,
                                const void* cand, uint64_t n, uint32_t d, uint32_t n_trees, uint32_t max_tree_depth,
                                uint32_t extension_level, uint32_t k, const void* idx) {
    if (k == 0 || k > BLISSGPU_KNN_MAX_K) return fail(BLISSGPU_ERR_INVALID, who, "k must be 1 .. BLISSGPU_KNN_MAX_K");
    if (d == 0 || d > BLISSGPU_FOREST_MAX_D) return fail(BLISSGPU_ERR_INVALID, who, "d must be 1 .. BLISSGPU_FOREST_MAX_D");
    if (n_trees == 0 || n_trees > BLISSGPU_FOREST_MAX_TREES) return fail(BLISSGPU_ERR_INVALID, who, "n_trees must be 1 .. BLISSGPU_FOREST_MAX_TREES");
    if (extension_level > d - 1) return fail(BLISSGPU_ERR_INVALID, who, "extension_level must be 0 .. d - 1");
    if (max_tree_depth > BLISSGPU_FOREST_MAX_DEPTH) return fail(BLISSGPU_ERR_INVALID, who, "max_tree_depth must be 1 .. 128 (0: none)");
    if (n >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n must be below 2^32 - 1 candidates");
    if (n_groups >= 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "n_groups must be below 2^32 - 1");
    if (n_groups == 0) return BLISSGPU_OK;
    if (!off) return fail(BLISSGPU_ERR_INVALID, who, "group_offsets is NULL");
    if (off[0] != 0) return fail(BLISSGPU_ERR_INVALID, who, "group_offsets[0] must be 0");
    for (uint64_t g = 0; g < n_groups; g++)
        if (off[g + 1] < off[g]) return fail(BLISSGPU_ERR_INVALID, who, "group_offsets must not decrease");
    if (off[n_groups] > 0xFFFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "2^32 seeds or more");
    if (off[n_groups] && !seeds_given) return fail(BLISSGPU_ERR_INVALID, who, "seeds is NULL");
    if (n && !cand) return fail(BLISSGPU_ERR_INVALID, who, "cand is NULL");
    if (!idx) return fail(BLISSGPU_ERR_INVALID, who, "idx is NULL");
    if (h_seeds)
        for (uint64_t i = 0; i < off[n_groups] * d; i++)
            if (!std::isfinite(h_seeds[i])) return fail(BLISSGPU_ERR_INVALID, who, "seed rows must be finite");
    return BLISSGPU_OK;
}

int blissgpu_group_forest_plan(const uint64_t* group_offsets, uint64_t n_groups, uint32_t d, uint32_t n_trees, uint32_t sample_size,
                               uint32_t max_tree_depth, uint32_t extension_level, uint64_t node_budget, uint64_t* batch_first,
                               uint64_t max_batches, uint64_t* n_batches) {
    const char* who = "blissgpu_group_forest_plan";
    uint32_t none = 0;  // (the plan reads neither seeds nor candidates)
    int rc = group_forest_args_ok(who, nullptr, true, group_offsets, n_groups, nullptr, 0, d, n_trees, max_tree_depth, extension_level, 1,
                                  &none);
    if (rc) return rc;
    if (!n_batches || (max_batches && !batch_first)) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (n_groups == 0) { *n_batches = 0; return BLISSGPU_OK; }
    if (node_budget == 0) node_budget = group_forest_budget(~0ull, extension_level);
    const std::vector<uint64_t> first = group_forest_batches(group_offsets, n_groups, n_trees, sample_size, node_budget);
    *n_batches = first.size() - 1;
    for (uint64_t i = 0; i < first.size() && i < max_batches; i++) batch_first[i] = first[i];
    return BLISSGPU_OK;
}

int blissgpu_group_forest_knn_device(blissgpu_ctx* c, const float* d_seeds, const float* h_seeds, const uint64_t* group_offsets,
                                     uint64_t n_groups, const float* d_cand, uint64_t n, uint32_t d, uint32_t n_trees,
                                     uint32_t sample_size, uint32_t max_tree_depth, uint32_t extension_level, uint64_t seed,
                                     const uint32_t* d_skip, uint32_t k, uint32_t* d_idx, float* d_score, int32_t* d_group_status) {
    const char* who = "blissgpu_group_forest_knn_device";
    int rc = group_forest_args_ok(who, h_seeds, d_seeds || h_seeds, group_offsets, n_groups, d_cand, n, d, n_trees, max_tree_depth,
                                  extension_level, k, d_idx);
    if (rc) return rc;
    if (!c) return fail(BLISSGPU_ERR_INVALID, who, "ctx is NULL");
    if (n_groups == 0) return BLISSGPU_OK;
    CTX_ENTER(c, who);
    std::vector<float> copy;
    const uint64_t n_seeds = group_offsets[n_groups];
    if (!h_seeds && n_seeds) {  // the forests are built on the host: the one device-to-host copy of the seed rows
        copy.resize((size_t)n_seeds * d);
        HIP_TRY(hipMemcpyAsync(copy.data(), d_seeds, copy.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (float v : copy)
            if (!std::isfinite(v)) return fail(BLISSGPU_ERR_INVALID, who, "seed rows must be finite");
        h_seeds = copy.data();
    }
    const GroupForestOpts o{d, n_trees, sample_size, max_tree_depth, extension_level, seed};
    return group_forest_run(c, who, h_seeds, group_offsets, n_groups, d_cand, n, o, d_skip, k, d_idx, d_score, d_group_status, nullptr);
}

int blissgpu_group_forest_knn(const float* seeds, const uint64_t* group_offsets, uint64_t n_groups, const float* cand, uint64_t n,
                              uint32_t d, uint32_t n_trees, uint32_t sample_size, uint32_t max_tree_depth, uint32_t extension_level,
                              uint64_t seed, const uint32_t* skip, uint32_t k, uint32_t* idx, float* score, int32_t* group_status) {
    const char* who = "blissgpu_group_forest_knn";
    int rc = group_forest_args_ok(who, seeds, seeds != nullptr, group_offsets, n_groups, cand, n, d, n_trees, max_tree_depth,
                                  extension_level, k, idx);
    if (rc) return rc;
    if (n_groups == 0) return BLISSGPU_OK;
    const uint64_t n_seeds = group_offsets[n_groups];
    if ((rc = skip_entries_ok(who, skip, n_seeds, n))) return rc;
    const size_t out_n = (size_t)n_groups * k;
    if (n == 0) {  // no candidates: rows of padding and the status, written here -- no forest, no device
        std::fill(idx, idx + out_n, 0xFFFFFFFFu);
        if (score) std::fill(score, score + out_n, INFINITY);
        if (group_status)
            for (uint64_t g = 0; g < n_groups; g++)
                group_status[g] = std::min<uint64_t>(sample_size, group_offsets[g + 1] - group_offsets[g]) < 2 ? BLISSGPU_GROUP_TOO_FEW_SEEDS
                                                                                                            : BLISSGPU_GROUP_OK;
        return BLISSGPU_OK;
    }
    blissgpu_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    CTX_ENTER(c, who);
    // (the seed rows stay on the host, where the forests are built, and so does the status they are built with)
    GroupLists g;
    rc = group_lists_stage(c, n_seeds, false, n, d, BLISSGPU_METRIC_EUCLIDEAN, nullptr, skip != nullptr, out_n, score ? out_n : 0, &g);
    if (rc) return rc;
    HostStage s{c, "group_forest_knn"};
    rc = group_lists_host(s, g, nullptr, n_seeds, cand, n, d, skip, out_n, idx, score, [&]() {
        const GroupForestOpts o{d, n_trees, sample_size, max_tree_depth, extension_level, seed};
        return group_forest_run(c, who, seeds, group_offsets, n_groups, g.cand, n, o, n_seeds ? g.skip : nullptr, k, g.idx, g.dist, nullptr,
                                group_status);
    });
    return s.finish(rc);
}

int blissgpu_debug_group_forest_stats(blissgpu_ctx* c, double* build_ms, double* wait_ms, uint64_t* n_batches) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_group_forest_stats", "ctx is NULL");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (build_ms) *build_ms = c->gf_build_ms;
    if (wait_ms) *wait_ms = c->gf_wait_ms;
    if (n_batches) *n_batches = c->gf_batches;
    return BLISSGPU_OK;
}

int blissgpu_debug_kmeans_stats(blissgpu_ctx* c, uint64_t* loop_copies, uint64_t* loop_bytes) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_kmeans_stats", "ctx is NULL");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (loop_copies) *loop_copies = c->km_loop_copies;
    if (loop_bytes) *loop_bytes = c->km_loop_bytes;
    return BLISSGPU_OK;
}

int blissgpu_debug_metric_stats(blissgpu_ctx* c, uint64_t* loop_uploads, uint64_t* loop_downloads, uint64_t* loop_bytes) {
    if (!c) return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_metric_stats", "ctx is NULL");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (loop_uploads) *loop_uploads = c->mt_uploads;
    if (loop_downloads) *loop_downloads = c->mt_downloads;
    if (loop_bytes) *loop_bytes = c->mt_bytes;
    return BLISSGPU_OK;
}

int blissgpu_malloc(void** p, uint64_t bytes) {
    if (!p) return fail(BLISSGPU_ERR_INVALID, "blissgpu_malloc", "NULL");
    hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? BLISSGPU_ERR_OOM : BLISSGPU_ERR_NO_DEVICE, "hipMalloc", hipGetErrorString(e));
    return BLISSGPU_OK;
}
int blissgpu_free(void* p) { HIP_TRY(hipFree(p)); return BLISSGPU_OK; }
int blissgpu_memcpy_h2d(blissgpu_ctx* c, void* dst, const void* src, uint64_t bytes) {
    CTX_ENTER(c, "blissgpu_memcpy_h2d");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BLISSGPU_OK;
}
int blissgpu_memcpy_d2h(blissgpu_ctx* c, void* dst, const void* src, uint64_t bytes) {
    CTX_ENTER(c, "blissgpu_memcpy_d2h");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BLISSGPU_OK;
}

static int synth_impl(blissgpu_ctx* c, float* d_pcm, const uint64_t* offsets, const uint64_t* lengths, uint32_t n_songs,
                      uint32_t first_song_index, const uint32_t* song_index) {
    if (!c || !d_pcm || !offsets || !lengths) return fail(BLISSGPU_ERR_INVALID, "blissgpu_synth_white_noise", "NULL argument");
    if (n_songs == 0) return BLISSGPU_OK;
    CTX_ENTER(c, "blissgpu_synth_white_noise");
    std::vector<SongDesc> songs(n_songs);
    std::vector<uint32_t> pfx(n_songs + 1, 0);
    for (uint32_t i = 0; i < n_songs; i++) {
        songs[i] = SongDesc{};
        songs[i].pcm_off = offsets[i];
        songs[i].n = lengths[i];
        songs[i].n_e = (uint32_t)((lengths[i] + 255) / 256);
        pfx[i + 1] = pfx[i] + (uint32_t)((lengths[i] + 4095) / 4096);
    }
    SongDesc* d_songs = nullptr;
    uint32_t *d_pfx = nullptr, *d_idx = nullptr;
    HIP_TRY(hipMalloc((void**)&d_songs, n_songs * sizeof(SongDesc)));
    hipError_t e = hipMalloc((void**)&d_pfx, (n_songs + 1) * sizeof(uint32_t));
    if (e == hipSuccess && song_index) e = hipMalloc((void**)&d_idx, n_songs * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_songs, songs.data(), n_songs * sizeof(SongDesc), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_pfx, pfx.data(), (n_songs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && song_index) e = hipMemcpy(d_idx, song_index, n_songs * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        Prof p(c, K_SYNTH);
        launch_synth(d_pcm, d_songs, n_songs, d_pfx, pfx[n_songs], first_song_index, d_idx, c->stream);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_songs);
    (void)hipFree(d_pfx);
    (void)hipFree(d_idx);
    if (e != hipSuccess) return fail(BLISSGPU_ERR_HIP, "synth", hipGetErrorString(e));
    return BLISSGPU_OK;
}

int blissgpu_synth_white_noise_device(blissgpu_ctx* c, float* d_pcm, const uint64_t* offsets, const uint64_t* lengths,
                                      uint32_t n_songs, uint32_t first_song_index) {
    return synth_impl(c, d_pcm, offsets, lengths, n_songs, first_song_index, nullptr);
}

int blissgpu_synth_white_noise_indexed_device(blissgpu_ctx* c, float* d_pcm, const uint64_t* offsets, const uint64_t* lengths,
                                              const uint32_t* song_index, uint32_t n_songs) {
    if (!song_index) return fail(BLISSGPU_ERR_INVALID, "blissgpu_synth_white_noise_indexed_device", "NULL argument");
    return synth_impl(c, d_pcm, offsets, lengths, n_songs, 0, song_index);
}

int blissgpu_profile_enable(blissgpu_ctx* c, int enable) {
    CTX_ENTER(c, "blissgpu_profile_enable");
    c->profiling = enable != 0;
    return BLISSGPU_OK;
}

int blissgpu_profile_reset(blissgpu_ctx* c) {
    CTX_ENTER(c, "blissgpu_profile_reset");
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->aux_stream);
    (void)hipStreamSynchronize(c->chr_stream);
    if (c->mask_stream) (void)hipStreamSynchronize(c->mask_stream);
    for (auto& v : c->events) {
        for (auto& ev : v) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
        v.clear();
    }
    return BLISSGPU_OK;
}

int blissgpu_profile_kernel_count(void) { return K_COUNT; }
const char* blissgpu_profile_kernel_name(int k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }

int blissgpu_profile_get(blissgpu_ctx* c, int k, double* total_ms, uint64_t* launches) {
    if (!c || k < 0 || k >= K_COUNT) return fail(BLISSGPU_ERR_INVALID, "blissgpu_profile_get", "bad kernel id");
    CTX_ENTER(c, "blissgpu_profile_get");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->aux_stream));
    HIP_TRY(hipStreamSynchronize(c->chr_stream));
    if (c->mask_stream) HIP_TRY(hipStreamSynchronize(c->mask_stream));
    double tot = 0.0;
    for (auto& ev : c->events[k]) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = c->events[k].size();
    return BLISSGPU_OK;
}

uint64_t blissgpu_debug_last_chunks(blissgpu_ctx* c) { return c ? c->last_chunks : 0; }

int blissgpu_debug_last_tuning(blissgpu_ctx* c, double* tuning, uint32_t* n_bpms, uint32_t n_songs) {
    if (!c || n_songs > c->dbg_n) return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_last_tuning", "no such batch");
    CTX_ENTER(c, "blissgpu_debug_last_tuning");
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int32_t> idx(n_songs);
    HIP_TRY(hipMemcpy(idx.data(), c->dbg_tuning.p, n_songs * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (tuning)
        for (uint32_t i = 0; i < n_songs; i++)
            tuning[i] = idx[i] < 0 ? 0.0 : (-50.0 + (100.0 * 0.01 * (double)idx[i])) / 100.0;
    if (n_bpms) HIP_TRY(hipMemcpy(n_bpms, c->dbg_nbpms.p, n_songs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BLISSGPU_OK;
}

int blissgpu_debug_fetch(blissgpu_ctx* c, int what, uint32_t song, void* dst, uint64_t max_elems, uint64_t* n_elems) {
    if (!c || !dst) return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_fetch", "NULL argument");
    CTX_ENTER(c, "blissgpu_debug_fetch");
    if (what == BLISSGPU_DEBUG_FILTER_BANK) {  // a table of the context, not of a batch: `song` is the tuning slot
        if (song > (uint32_t)N_TUNING) return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_fetch", "tuning slot must be 0..100");
        const uint64_t n = (uint64_t)BANK_ROWS * BANK_PITCH;
        if (n_elems) *n_elems = n;
        const uint64_t k = std::min(n, max_elems);
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (k) HIP_TRY(hipMemcpy(dst, c->chroma_bank + (size_t)song * n, k * sizeof(double), hipMemcpyDeviceToHost));
        return BLISSGPU_OK;
    }
    // `song` is the caller's index into the last batch; the chunk keeps its songs in length order
    size_t pos = c->last_songs.size();
    for (size_t i = 0; i < c->last_songs.size(); i++)
        if (c->last_songs[i].row == song) { pos = i; break; }
    if (pos == c->last_songs.size()) return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_fetch", "no such song in the last chunk");
    HIP_TRY(hipStreamSynchronize(c->stream));
    const SongDesc& d = c->last_songs[pos];
    const Workspace& w = c->last_ws;
    const void* src = nullptr;
    uint64_t n = 0, esz = 4;
    const uint64_t runs = d.ok ? (d.n_b >= (uint32_t)BT_STEP ? (d.n_b - BT_STEP) / BT_STEP + 1 : 0) : 0;
    switch (what) {
        case BLISSGPU_DEBUG_CENTROID: src = w.centroid + d.t_off; n = d.n_t; break;
        case BLISSGPU_DEBUG_ROLLOFF: src = w.rolloff + d.t_off; n = d.n_t; break;
        case BLISSGPU_DEBUG_FLATNESS: src = w.flatness + d.t_off; n = d.n_t; break;
        case BLISSGPU_DEBUG_FLUX: src = w.flux + d.b_off; n = d.n_b; break;
        case BLISSGPU_DEBUG_THRESHOLDED: src = w.thresholded + d.b_off; n = d.n_b; break;
        case BLISSGPU_DEBUG_RUN_BPM: src = w.run_bpm + pos * w.runs_pitch; n = runs; break;
        case BLISSGPU_DEBUG_RUN_COUNT: src = w.run_cnt + pos * w.runs_pitch; n = runs; break;
        case BLISSGPU_DEBUG_SPECTROGRAM: src = w.spec + d.c_off * (size_t)CBINS_PAD; n = (uint64_t)d.n_c * CBINS_PAD; break;
        case BLISSGPU_DEBUG_ENERGY256: src = w.e256 + d.e_off; n = d.n_e; break;
        case BLISSGPU_DEBUG_CROSSINGS256: src = w.zc256 + d.e_off; n = d.n_e; break;
        case BLISSGPU_DEBUG_PITCH_HIST: src = w.hist100 + pos * N_TUNING; n = N_TUNING; break;
        case BLISSGPU_DEBUG_CHROMA:
        case BLISSGPU_DEBUG_INTERVAL:
            if (!w.dbg_chroma || !w.dbg_interval)
                return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_fetch", "set BLISSGPU_OPT_DEBUG_CHROMA before the analysis");
            esz = 8;
            if (what == BLISSGPU_DEBUG_CHROMA) { src = w.dbg_chroma + d.c_off * 12; n = (uint64_t)d.n_c * 12; }
            else { src = w.dbg_interval + pos * 10; n = 10; }
            break;
        default: return fail(BLISSGPU_ERR_INVALID, "blissgpu_debug_fetch", "unknown tap");
    }
    if (!d.ok) n = 0;
    if (n_elems) *n_elems = n;
    const uint64_t k = std::min(n, max_elems);
    if (k) HIP_TRY(hipMemcpy(dst, src, k * esz, hipMemcpyDeviceToHost));
    return BLISSGPU_OK;
}

}  // extern "C"

// ---- FLAC: compressed files in, PCM / feature rows out (flac_index.hpp on the host, kernels_flac.hip on the device) ----
#include <thread>

#include "flac_frame.hpp"
#include "flac_index.hpp"
#include "flac_verify.hpp"

namespace {

struct FlacPlan {  // one file of a call
    const uint8_t* file = nullptr;
    uint64_t nbytes = 0;
    flac::StreamInfo si;
    uint64_t total = 0;  // inter-channel samples the frame table holds
    uint64_t base = 0;   // stream position of the first frame
    std::vector<flac::FrameRow> rows;
    bool error = false;  // not FLAC, unsupported, truncated, or frames that verified mode cannot repair
    bool slow = false;   // the table is verified mode's
    uint64_t byte_off = 0, pcm_off = 0, pcm_bytes = 0;
};

void flac_info_words(const flac::StreamInfo& si, uint64_t* info) {
    info[0] = si.sample_rate; info[1] = si.channels; info[2] = si.bps; info[3] = si.total;
    info[4] = si.min_block; info[5] = si.max_block; info[6] = si.min_frame; info[7] = si.first_frame;
    memcpy(&info[8], si.md5, 16);
    info[10] = 0; info[11] = 0;
}

void flac_index_plan(FlacPlan& p, bool verified) {
    p.error = true;
    int rc = flac::index_frames(p.file, p.nbytes, p.si, verified, &p.rows, &p.total, &p.base);
    if (rc && !verified) {  // (a table the fast filter cannot close, e.g. after a false candidate: the exact mode decides)
        verified = true;
        rc = flac::index_frames(p.file, p.nbytes, p.si, true, &p.rows, &p.total, &p.base);
    }
    p.slow = verified;
    if (rc) return;
    p.pcm_bytes = p.total * p.si.channels * (p.si.bps > 16 ? 4 : 2);
    p.error = false;
}

// (an exception -- no memory for the table of a file with millions of tiny frames -- costs that song, not the process)
void flac_plan(FlacPlan& p) {
    p.error = true;
    try {
        if (!p.file || flac::stream_info(p.file, p.nbytes, &p.si)) return;
        if (p.si.bps < 4 || p.si.bps > 24 || p.si.sample_rate > MAX_SAMPLE_RATE) return;
        flac_index_plan(p, false);
    } catch (...) {
        p.rows.clear();
        p.error = true;
    }
}

// The opt-in checks of a call: what was asked for, and per file of the call the verdict flags (BLISSGPU_FLAC_BAD_CRC16 /
// _BAD_MD5 / _MD5_UNCHECKED; BAD_STREAM is the plan's error), the first frame whose CRC-16 failed, the computed digest.
struct FlacVerify {
    uint32_t checks = 0;
    std::vector<uint32_t> flags, first_bad;
    std::vector<uint8_t> md5;
    FlacVerify(uint32_t checks_, size_t n) : checks(checks_), flags(n, BLISSGPU_FLAC_MD5_UNCHECKED), first_bad(n, 0xFFFFFFFFu), md5(16 * n, 0) {}
};

// what a song keeps resident while its sub-batch is decoded and analysed: compressed bytes, PCM, the mono 22 050 Hz stream
uint64_t flac_resident_bytes(const FlacPlan& p) { return p.pcm_bytes + p.nbytes + 4 * p.total + 64; }

// the frame tables of a call, on at most as many threads as the context's staging ring has workers
void flac_plan_all(blissgpu_ctx* c, std::vector<FlacPlan>& plans) {
    const uint32_t n_songs = (uint32_t)plans.size();
    const uint32_t workers = std::min<uint32_t>(n_songs, (uint32_t)std::max(1, std::min(c->feed.stage_cfg.lanes, MAX_STAGE_LANES)));
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
        for (uint32_t i; (i = next.fetch_add(1)) < n_songs;) flac_plan(plans[i]);
    };
    std::vector<std::thread> pool;
    for (uint32_t w = 1; w < workers; w++) pool.emplace_back(work);
    work();
    for (std::thread& t : pool) t.join();
}

// The next sub-batch of a call: the songs from i0 on whose resident bytes fit the workspace limit together (at least one
// song) -> sel; returns the first song of the sub-batch after it.  A song that does not fit the limit by itself (a few MB of
// CONSTANT frames can claim hundreds of GB) is refused: its plan's error is set
uint32_t flac_next_subbatch(blissgpu_ctx* c, std::vector<FlacPlan>& plans, uint32_t i0, std::vector<uint32_t>* sel) {
    sel->clear();
    uint64_t resident = 0;
    uint32_t i1 = i0;
    for (; i1 < plans.size(); i1++) {
        if (!plans[i1].error && flac_resident_bytes(plans[i1]) > c->ws_limit) plans[i1].error = true;
        const uint64_t b = plans[i1].error ? 0 : flac_resident_bytes(plans[i1]);
        if (!sel->empty() && resident + b > c->ws_limit) break;
        resident += b;
        sel->push_back(i1);
    }
    return i1;
}

// songs | frames into the context's table buffer (through its page-locked staging), asynchronous on the context's stream
int flac_upload_tables(blissgpu_ctx* c, const std::vector<FlacSong>& songs, const std::vector<FlacFrame>& frames,
                       const FlacSong** d_songs, const FlacFrame** d_frames) {
    const size_t sb = songs.size() * sizeof(FlacSong), fb = frames.size() * sizeof(FlacFrame);
    static_assert(sizeof(FlacSong) % 8 == 0 && sizeof(FlacFrame) == 32, "table rows keep their 8-byte alignment");
    int rc = c->fl_tab.ensure(sb + fb + 8);
    if (rc) return rc;
    if (!c->fl_ev) HIP_TRY(hipEventCreateWithFlags(&c->fl_ev, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(c->fl_ev));
    if ((rc = c->fl_htab.ensure(sb + fb + 8))) return rc;
    memcpy(c->fl_htab.p, songs.data(), sb);
    memcpy(c->fl_htab.p + sb, frames.data(), fb);
    HIP_TRY(hipMemcpyAsync(c->fl_tab.p, c->fl_htab.p, sb + fb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->fl_ev, c->stream));
    *d_songs = (const FlacSong*)c->fl_tab.p;
    *d_frames = (const FlacFrame*)(c->fl_tab.p + sb);
    return BLISSGPU_OK;
}

void flac_rows_of(const FlacPlan& p, uint32_t song, std::vector<FlacFrame>* frames) {
    for (const flac::FrameRow& r : p.rows)
        frames->push_back(FlacFrame{r.offset, r.nbytes, r.first_sample, (uint32_t)r.blocksize, song});
    if (!p.rows.empty()) frames->back().song |= FLAC_LAST_FRAME;
}

// Upload, decode and check the planned files `sel` (indices into plans); afterwards plans[i].error says which of them have
// no PCM, the others' PCM sits at c->fl_pcm.p + pcm_off.  Synchronises the context's stream.
// v (may be NULL): the checks to run on the songs that decoded -- the CRC-16 of every frame of the table a song ended with,
// then the MD5 of the PCM of the songs that are sound so far; v's entries of `sel` are filled, plans[i].error is left to the caller.
int flac_run(blissgpu_ctx* c, std::vector<FlacPlan>& plans, const std::vector<uint32_t>& sel, const char* who, FlacVerify* v = nullptr) {
    std::vector<FlacSong> songs;
    std::vector<FlacFrame> frames;
    std::vector<uint32_t> live;  // plans that reach the device
    uint64_t bytes = 0, pcm = 0;
    for (uint32_t i : sel) {
        FlacPlan& p = plans[i];
        if (p.error) continue;
        p.byte_off = bytes;
        p.pcm_off = pcm;
        bytes += (p.nbytes + flac::FILE_PAD + 15) & ~15ull;
        pcm += (p.pcm_bytes + 15) & ~15ull;
        if (frames.size() + p.rows.size() > 0x7FFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "more than 2^31 frames in one sub-batch");
        flac_rows_of(p, (uint32_t)live.size(), &frames);
        if (p.slow) c->fl_slow_songs++;  // (the fast filter could not close its table on the host already)
        songs.push_back(FlacSong{p.byte_off, p.nbytes, p.pcm_off, p.total, p.base, p.si.channels, p.si.bps});
        live.push_back(i);
    }
    if (live.empty()) return BLISSGPU_OK;
    int rc = c->fl_bytes.ensure(bytes + flac::FILE_PAD);
    if (!rc) rc = c->fl_pcm.ensure(pcm + 16);
    if (!rc) rc = c->fl_bad.ensure(live.size());
    if (rc) return rc;
    for (uint32_t k = 0; k < live.size(); k++)
        HIP_TRY(hipMemcpyAsync(c->fl_bytes.p + songs[k].byte_off, plans[live[k]].file, plans[live[k]].nbytes, hipMemcpyHostToDevice, c->stream));
    std::vector<uint32_t> bad(live.size(), 0);
    // the CRC-16 check: [first row | flag | first bad frame] per song, and which songs have rows in this pass
    const bool crc = v && (v->checks & BLISSGPU_FLAC_CHECK_CRC16);
    const size_t ns = live.size();
    std::vector<uint32_t> vsong(crc ? 3 * ns : 0, 0);
    std::vector<uint8_t> in_pass(ns, 1);
    if (crc) {
        if ((rc = c->fl_vsong.ensure(3 * ns))) return rc;
        uint32_t row = 0;
        for (size_t k = 0; k < ns; k++) {
            vsong[k] = row;
            row += (uint32_t)plans[live[k]].rows.size();
        }
    }
    for (int pass = 0; pass < 2 && !frames.empty(); pass++) {
        const FlacSong* d_songs;
        const FlacFrame* d_frames;
        if ((rc = c->fl_status.ensure(frames.size()))) return rc;
        if ((rc = c->fl_end.ensure(frames.size()))) return rc;
        if ((rc = flac_upload_tables(c, songs, frames, &d_songs, &d_frames))) return rc;
        HIP_TRY(hipMemsetAsync(c->fl_bad.p, 0, live.size() * sizeof(uint32_t), c->stream));
        launch_flac_decode(c->fl_bytes.p, d_songs, d_frames, (uint32_t)frames.size(), c->fl_pcm.p, c->fl_status.p, c->fl_end.p, c->stream);
        launch_flac_check(d_frames, (uint32_t)frames.size(), c->fl_status.p, c->fl_end.p, c->fl_bad.p, c->stream);
        if (crc) {
            for (size_t k = 0; k < ns; k++) { vsong[ns + k] = 0; vsong[2 * ns + k] = 0xFFFFFFFFu; }
            HIP_TRY(hipMemcpyAsync(c->fl_vsong.p, vsong.data(), 3 * ns * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            launch_flac_crc(c->fl_bytes.p, d_songs, d_frames, (uint32_t)frames.size(), c->fl_status.p, c->fl_end.p, c->fl_vsong.p,
                            c->fl_vsong.p + ns, c->fl_vsong.p + 2 * ns, nullptr, c->stream);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(bad.data(), c->fl_bad.p, live.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (crc) HIP_TRY(hipMemcpyAsync(vsong.data() + ns, c->fl_vsong.p + ns, 2 * ns * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (crc)  // the verdict of the songs whose table stood in this pass
            for (size_t k = 0; k < ns; k++)
                if (in_pass[k] && !bad[k] && vsong[ns + k]) {
                    v->flags[live[k]] |= BLISSGPU_FLAC_BAD_CRC16;
                    v->first_bad[live[k]] = vsong[2 * ns + k];
                }
        std::fill(in_pass.begin(), in_pass.end(), 0);
        // the songs the device refused go through verified mode and a second, small launch -- each of them alone
        frames.clear();
        for (uint32_t k = 0; k < live.size(); k++) {
            FlacPlan& p = plans[live[k]];
            if (!bad[k]) continue;
            if (p.slow || pass == 1) { p.error = true; continue; }
            c->fl_slow_songs++;
            const uint64_t room = (p.pcm_bytes + 15) & ~15ull;  // the PCM region was sized by the fast table
            try { flac_index_plan(p, true); } catch (...) { p.error = true; }
            if (p.error || p.pcm_bytes > room) { p.error = true; continue; }
            songs[k].total = p.total;
            songs[k].base = p.base;
            if (crc) vsong[k] = (uint32_t)frames.size();
            in_pass[k] = 1;
            flac_rows_of(p, k, &frames);
        }
    }
    if (!v || !(v->checks & BLISSGPU_FLAC_CHECK_MD5)) return BLISSGPU_OK;
    // the MD5 of the songs that are sound so far and whose STREAMINFO digest speaks of exactly these samples; longest first
    std::vector<FlacMd5Job> jobs;
    for (uint32_t k = 0; k < live.size(); k++) {
        const FlacPlan& p = plans[live[k]];
        static const uint8_t zero[16] = {0};
        if (p.error || (v->flags[live[k]] & BLISSGPU_FLAC_BAD_CRC16) || !memcmp(p.si.md5, zero, 16) || p.base != 0 ||
            (p.si.total != 0 && p.si.total != p.total))
            continue;
        jobs.push_back(FlacMd5Job{p.pcm_off, p.total * p.si.channels, p.si.bps, k});
    }
    if (jobs.empty()) return BLISSGPU_OK;
    std::stable_sort(jobs.begin(), jobs.end(), [](const FlacMd5Job& a, const FlacMd5Job& b) {
        return a.n_elems * flac::Md5Pcm::width_of(a.bps) > b.n_elems * flac::Md5Pcm::width_of(b.bps);
    });
    if ((rc = c->fl_md5_jobs.ensure(jobs.size()))) return rc;
    if ((rc = c->fl_md5.ensure(16 * live.size()))) return rc;
    std::vector<uint8_t> digests(16 * live.size());
    HIP_TRY(hipMemcpyAsync(c->fl_md5_jobs.p, jobs.data(), jobs.size() * sizeof(FlacMd5Job), hipMemcpyHostToDevice, c->stream));
    launch_flac_md5(c->fl_pcm.p, c->fl_md5_jobs.p, (uint32_t)jobs.size(), c->fl_md5.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(digests.data(), c->fl_md5.p, digests.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const FlacMd5Job& j : jobs) {
        const uint32_t i = live[j.slot];
        memcpy(&v->md5[16 * (size_t)i], &digests[16 * (size_t)j.slot], 16);
        v->flags[i] &= ~BLISSGPU_FLAC_MD5_UNCHECKED;
        if (memcmp(&digests[16 * (size_t)j.slot], plans[i].si.md5, 16)) v->flags[i] |= BLISSGPU_FLAC_BAD_MD5;
    }
    return BLISSGPU_OK;
}

struct FlacDeviceRestore {
    int prev = -1;
    FlacDeviceRestore() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~FlacDeviceRestore() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

extern "C" {

int blissgpu_flac_info(const void* file, uint64_t nbytes, uint64_t* info) {
    if (!file || !info) return fail(BLISSGPU_ERR_INVALID, "blissgpu_flac_info", "NULL argument");
    flac::StreamInfo si;
    const int rc = flac::stream_info((const uint8_t*)file, nbytes, &si);
    if (rc) return fail(BLISSGPU_ERR_INVALID, "blissgpu_flac_info", rc == flac::INDEX_NOT_FLAC ? "not a FLAC stream" : "truncated in the metadata");
    flac_info_words(si, info);
    return BLISSGPU_OK;
}

int blissgpu_flac_index(const void* file, uint64_t nbytes, int verified, uint64_t* info, uint64_t* frames, uint64_t max_frames,
                        uint64_t* n_frames) {
    const char* who = "blissgpu_flac_index";
    if (!file || !n_frames) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    *n_frames = 0;
    flac::StreamInfo si;
    int rc = flac::stream_info((const uint8_t*)file, nbytes, &si);
    if (rc) return fail(BLISSGPU_ERR_INVALID, who, rc == flac::INDEX_NOT_FLAC ? "not a FLAC stream" : "truncated in the metadata");
    std::vector<flac::FrameRow> rows;
    uint64_t total = 0, base = 0;
    rc = flac::index_frames((const uint8_t*)file, nbytes, si, verified != 0, &rows, &total, &base);
    *n_frames = rows.size();
    if (frames) memcpy(frames, rows.data(), sizeof(flac::FrameRow) * (size_t)std::min<uint64_t>(max_frames, rows.size()));
    if (info) {
        flac_info_words(si, info);
        info[3] = total;
        info[10] = base;
    }
    if (rc) return fail(BLISSGPU_ERR_INVALID, who, rc == flac::INDEX_NO_FRAMES ? "no frame behind the metadata" : "frames are missing (truncated)");
    return BLISSGPU_OK;
}

int blissgpu_flac_decode_device(blissgpu_ctx* c, const void* d_bytes, uint64_t nbytes, const uint64_t* frames, uint64_t n_frames,
                                const uint64_t* info, void* d_pcm, int32_t* d_frame_status, uint64_t* d_frame_end) {
    const char* who = "blissgpu_flac_decode_device";
    if (!d_bytes || !info || (n_frames && (!frames || !d_pcm || !d_frame_status || !d_frame_end))) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (((uintptr_t)d_bytes & 7) != 0 || ((uintptr_t)d_pcm & 3) != 0) return fail(BLISSGPU_ERR_INVALID, who, "d_bytes must be 8-byte, d_pcm 4-byte aligned");
    if (info[1] < 1 || info[1] > 8 || info[2] < 1 || info[2] > 32 || n_frames > 0x7FFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "bad info / n_frames");
    CTX_ENTER(c, who);
    if (n_frames == 0) return BLISSGPU_OK;
    std::vector<FlacSong> songs{FlacSong{0, nbytes, 0, info[3], info[10], (uint32_t)info[1], (uint32_t)info[2]}};
    std::vector<FlacFrame> rows((size_t)n_frames);
    for (uint64_t i = 0; i < n_frames; i++) {
        const uint64_t* r = frames + 4 * i;
        if (r[0] > nbytes || r[1] > nbytes - r[0] || r[3] == 0 || r[3] > 65536) return fail(BLISSGPU_ERR_INVALID, who, "a frame row lies outside the file");
        rows[i] = FlacFrame{r[0], r[1], r[2], (uint32_t)r[3], i + 1 == n_frames ? FLAC_LAST_FRAME : 0u};
    }
    const FlacSong* d_songs;
    const FlacFrame* d_frames;
    const int rc = flac_upload_tables(c, songs, rows, &d_songs, &d_frames);
    if (rc) return rc;
    launch_flac_decode((const uint8_t*)d_bytes, d_songs, d_frames, (uint32_t)n_frames, (uint8_t*)d_pcm, d_frame_status, d_frame_end, c->stream);
    HIP_TRY(hipGetLastError());
    return BLISSGPU_OK;
}

uint64_t blissgpu_ctx_flac_slow_songs(blissgpu_ctx* c) {
    if (!c) return 0;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    return c->fl_slow_songs;
}

int blissgpu_flac_decode(const void* file, uint64_t nbytes, void* pcm, uint64_t max_bytes, uint64_t* info, int32_t* status) {
    const char* who = "blissgpu_flac_decode";
    if (!file || !info || !status) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    std::vector<FlacPlan> plans(1);
    plans[0].file = (const uint8_t*)file;
    plans[0].nbytes = nbytes;
    flac_plan(plans[0]);
    flac_info_words(plans[0].si, info);
    info[3] = plans[0].total;
    info[10] = plans[0].base;
    *status = BLISSGPU_SONG_DECODE_ERROR;
    if (plans[0].error) return BLISSGPU_OK;
    if (!pcm) { *status = BLISSGPU_SONG_OK; return BLISSGPU_OK; }  // sizes only (whether it fits the workspace limit shows with pcm)
    if (max_bytes < plans[0].pcm_bytes) return fail(BLISSGPU_ERR_INVALID, who, "pcm is smaller than total x channels x sample width");
    FlacDeviceRestore restore;
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    if (flac_resident_bytes(plans[0]) > c->ws_limit) return BLISSGPU_OK;  // (*status says DECODE_ERROR)
    if ((rc = flac_run(c, plans, {0}, who))) return rc;
    info[3] = plans[0].total;
    if (plans[0].error) return BLISSGPU_OK;
    const uint64_t nb = plans[0].total * plans[0].si.channels * (plans[0].si.bps > 16 ? 4 : 2);
    if (nb) HIP_TRY(hipMemcpy(pcm, c->fl_pcm.p + plans[0].pcm_off, nb, hipMemcpyDeviceToHost));
    *status = BLISSGPU_SONG_OK;
    return BLISSGPU_OK;
}

int blissgpu_flac_decode_batch(const void* const* files, const uint64_t* nbytes, uint32_t n_songs, void* const* pcm,
                               const uint64_t* max_bytes, uint64_t* info, int32_t* status) {
    const char* who = "blissgpu_flac_decode_batch";
    if (n_songs && (!files || !nbytes || !pcm || !max_bytes || !info || !status)) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (n_songs == 0) return BLISSGPU_OK;
    FlacDeviceRestore restore;
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    std::vector<FlacPlan> plans(n_songs);
    std::vector<uint32_t> sel;
    uint64_t resident = 0;
    for (uint32_t i = 0; i < n_songs; i++) {
        plans[i].file = (const uint8_t*)files[i];
        plans[i].nbytes = nbytes[i];
        flac_plan(plans[i]);
        if (!plans[i].error && (plans[i].pcm_bytes > max_bytes[i] || (plans[i].pcm_bytes && !pcm[i]))) plans[i].error = true;
        if (!plans[i].error && flac_resident_bytes(plans[i]) > c->ws_limit) plans[i].error = true;  // refused alone, as in the bulk form
        if (!plans[i].error) resident += flac_resident_bytes(plans[i]);
        sel.push_back(i);
    }
    if (resident > c->ws_limit) return fail(BLISSGPU_ERR_INVALID, who, "the files do not fit the workspace limit together");
    if ((rc = flac_run(c, plans, sel, who))) return rc;
    for (uint32_t i = 0; i < n_songs; i++) {
        const FlacPlan& p = plans[i];
        flac_info_words(p.si, info + (size_t)i * BLISSGPU_FLAC_INFO_WORDS);
        info[(size_t)i * BLISSGPU_FLAC_INFO_WORDS + 3] = p.total;
        info[(size_t)i * BLISSGPU_FLAC_INFO_WORDS + 10] = p.base;
        status[i] = p.error ? BLISSGPU_SONG_DECODE_ERROR : BLISSGPU_SONG_OK;
        const uint64_t nb = p.error ? 0 : p.total * p.si.channels * (p.si.bps > 16 ? 4 : 2);
        if (nb) HIP_TRY(hipMemcpy(pcm[i], c->fl_pcm.p + p.pcm_off, nb, hipMemcpyDeviceToHost));
    }
    return BLISSGPU_OK;
}

// blissgpu_analyze_batch_flac, and with checks != 0 its verified form: a song that fails a check is refused like one that
// does not decode; nothing else of the call changes
static int flac_analyze(const void* const* files, const uint64_t* nbytes, uint32_t n_songs, uint32_t features_version, uint32_t checks,
                        float* out, int32_t* status, uint32_t* flags, uint32_t* first_bad_frame, const char* who) {
    const uint32_t d = blissgpu_feature_count(features_version);
    if (!d) return fail(BLISSGPU_ERR_INVALID, who, "features_version must be 1 or 2");
    if (n_songs && (!files || !nbytes || !out || (checks && !flags))) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (checks & ~(BLISSGPU_FLAC_CHECK_CRC16 | BLISSGPU_FLAC_CHECK_MD5)) return fail(BLISSGPU_ERR_INVALID, who, "unknown check");
    if (n_songs == 0) return BLISSGPU_OK;
    FlacDeviceRestore restore;
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    FlacVerify verify(checks, checks ? n_songs : 0);
    FlacVerify* v = checks ? &verify : nullptr;
    // 1. the frame tables
    std::vector<FlacPlan> plans(n_songs);
    for (uint32_t i = 0; i < n_songs; i++) {
        plans[i].file = (const uint8_t*)files[i];
        plans[i].nbytes = nbytes[i];
    }
    flac_plan_all(c, plans);
    const float nan = nanf("");
    auto refuse = [&](uint32_t i) {
        for (uint32_t k = 0; k < d; k++) out[(size_t)i * d + k] = nan;
        if (status) status[i] = BLISSGPU_SONG_DECODE_ERROR;
    };
    // 2. - 6. sub-batch by sub-batch: the decoded PCM of one has to fit the workspace limit
    uint32_t i0 = 0;
    while (i0 < n_songs) {
        std::vector<uint32_t> sel;
        const uint32_t i1 = flac_next_subbatch(c, plans, i0, &sel);
        if ((rc = flac_run(c, plans, sel, who, v))) return rc;
        std::vector<uint32_t> good;
        std::vector<uint64_t> offs, lens;
        uint64_t mono = 0;
        for (uint32_t i : sel) {
            if (v) {
                if (plans[i].error) v->flags[i] |= BLISSGPU_FLAC_BAD_STREAM;
                flags[i] = v->flags[i];
                if (first_bad_frame) first_bad_frame[i] = v->first_bad[i];
                if (v->flags[i] & 7u) plans[i].error = true;
            }
            if (plans[i].error) { refuse(i); continue; }
            good.push_back(i);
            offs.push_back(mono);
            lens.push_back(blissgpu_resampled_len(plans[i].total, plans[i].si.sample_rate));
            mono += (lens.back() + 3) & ~3ull;
        }
        if (!good.empty()) {
            const size_t n = good.size();
            if ((rc = c->fl_mono.ensure(mono + 4))) return rc;
            if ((rc = c->fl_rows.ensure(n * d + n))) return rc;
            for (size_t k = 0; k < n; k++) {
                const FlacPlan& p = plans[good[k]];
                if (!lens[k]) continue;
                rc = enqueue_decode(c, c->fl_pcm.p + p.pcm_off, p.si.bps > 16 ? BLISSGPU_SAMPLE_S32 : BLISSGPU_SAMPLE_S16, p.si.channels, p.total,
                                    p.si.sample_rate, c->fl_mono.p + offs[k], lens[k], c->stream, who);
                if (rc) return rc;
            }
            int32_t* d_status = (int32_t*)(c->fl_rows.p + n * d);
            rc = blissgpu_analyze_batch_device(c, c->fl_mono.p, offs.data(), lens.data(), (uint32_t)n, features_version, c->fl_rows.p, d_status);
            if (rc) return rc;
            std::vector<float> rows(n * d);
            std::vector<int32_t> st(n);
            HIP_TRY(hipMemcpyAsync(rows.data(), c->fl_rows.p, n * d * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(st.data(), d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (size_t k = 0; k < n; k++) {
                memcpy(out + (size_t)good[k] * d, rows.data() + k * d, d * sizeof(float));
                if (status) status[good[k]] = st[k];
            }
        }
        i0 = i1;
    }
    return BLISSGPU_OK;
}

int blissgpu_analyze_batch_flac(const void* const* files, const uint64_t* nbytes, uint32_t n_songs, uint32_t features_version,
                                float* out, int32_t* status) {
    return flac_analyze(files, nbytes, n_songs, features_version, 0, out, status, nullptr, nullptr, "blissgpu_analyze_batch_flac");
}

int blissgpu_analyze_batch_flac_verified(const void* const* files, const uint64_t* nbytes, uint32_t n_songs, uint32_t features_version,
                                         uint32_t checks, float* out, int32_t* status, uint32_t* flags, uint32_t* first_bad_frame) {
    return flac_analyze(files, nbytes, n_songs, features_version, checks, out, status, flags, first_bad_frame,
                        "blissgpu_analyze_batch_flac_verified");
}

int blissgpu_flac_verify_batch(const void* const* files, const uint64_t* nbytes, uint32_t n_songs, uint32_t checks, uint32_t* flags,
                               uint32_t* first_bad_frame, void* md5) {
    const char* who = "blissgpu_flac_verify_batch";
    if (n_songs && (!files || !nbytes || !flags)) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (checks & ~(BLISSGPU_FLAC_CHECK_CRC16 | BLISSGPU_FLAC_CHECK_MD5)) return fail(BLISSGPU_ERR_INVALID, who, "unknown check");
    if (n_songs == 0) return BLISSGPU_OK;
    FlacDeviceRestore restore;
    blissgpu_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    CTX_ENTER(c, who);
    FlacVerify v(checks, n_songs);
    std::vector<FlacPlan> plans(n_songs);
    for (uint32_t i = 0; i < n_songs; i++) {
        plans[i].file = (const uint8_t*)files[i];
        plans[i].nbytes = nbytes[i];
    }
    flac_plan_all(c, plans);
    // sub-batch by sub-batch, split like the bulk analysis
    uint32_t i0 = 0;
    while (i0 < n_songs) {
        std::vector<uint32_t> sel;
        const uint32_t i1 = flac_next_subbatch(c, plans, i0, &sel);
        if ((rc = flac_run(c, plans, sel, who, &v))) return rc;
        i0 = i1;
    }
    for (uint32_t i = 0; i < n_songs; i++) {
        flags[i] = v.flags[i] | (plans[i].error ? BLISSGPU_FLAC_BAD_STREAM : 0u);
        if (first_bad_frame) first_bad_frame[i] = v.first_bad[i];
    }
    if (md5) memcpy(md5, v.md5.data(), v.md5.size());
    return BLISSGPU_OK;
}

int blissgpu_flac_crc16_device(blissgpu_ctx* c, const void* d_bytes, uint64_t nbytes, const uint64_t* frames, uint64_t n_frames,
                               const int32_t* d_frame_status, const uint64_t* d_frame_end, int32_t* d_frame_crc_ok) {
    const char* who = "blissgpu_flac_crc16_device";
    if (!d_bytes || (n_frames && (!frames || !d_frame_status || !d_frame_end || !d_frame_crc_ok))) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (((uintptr_t)d_bytes & 7) != 0) return fail(BLISSGPU_ERR_INVALID, who, "d_bytes must be 8-byte aligned");
    if (n_frames > 0x7FFFFFFFull) return fail(BLISSGPU_ERR_INVALID, who, "bad n_frames");
    CTX_ENTER(c, who);
    if (n_frames == 0) return BLISSGPU_OK;
    std::vector<FlacSong> songs{FlacSong{0, nbytes, 0, 0, 0, 1, 16}};
    std::vector<FlacFrame> rows((size_t)n_frames);
    for (uint64_t i = 0; i < n_frames; i++) {
        const uint64_t* r = frames + 4 * i;
        if (r[0] > nbytes || r[1] > nbytes - r[0]) return fail(BLISSGPU_ERR_INVALID, who, "a frame row lies outside the file");
        rows[i] = FlacFrame{r[0], r[1], r[2], (uint32_t)r[3], i + 1 == n_frames ? FLAC_LAST_FRAME : 0u};
    }
    const FlacSong* d_songs;
    const FlacFrame* d_frames;
    const int rc = flac_upload_tables(c, songs, rows, &d_songs, &d_frames);
    if (rc) return rc;
    launch_flac_crc((const uint8_t*)d_bytes, d_songs, d_frames, (uint32_t)n_frames, d_frame_status, d_frame_end, nullptr, nullptr, nullptr,
                    d_frame_crc_ok, c->stream);
    HIP_TRY(hipGetLastError());
    return BLISSGPU_OK;
}

int blissgpu_flac_md5_device(blissgpu_ctx* c, const void* d_pcm, const uint64_t* info, void* d_md5) {
    const char* who = "blissgpu_flac_md5_device";
    if (!info || !d_md5 || (!d_pcm && info[3])) return fail(BLISSGPU_ERR_INVALID, who, "NULL argument");
    if (((uintptr_t)d_pcm & 3) != 0 || ((uintptr_t)d_md5 & 3) != 0) return fail(BLISSGPU_ERR_INVALID, who, "d_pcm and d_md5 must be 4-byte aligned");
    // (a stream codes its total in 36 bits: with 8 channels and 4 bytes per element every size below stays far inside 64 bits)
    if (info[1] < 1 || info[1] > 8 || info[2] < 4 || info[2] > 24 || info[3] >> 36) return fail(BLISSGPU_ERR_INVALID, who, "bad info");
    CTX_ENTER(c, who);
    launch_flac_md5_one((const uint8_t*)d_pcm, FlacMd5Job{0, info[3] * info[1], (uint32_t)info[2], 0}, d_md5, c->stream);
    HIP_TRY(hipGetLastError());
    return BLISSGPU_OK;
}

}  // extern "C"
