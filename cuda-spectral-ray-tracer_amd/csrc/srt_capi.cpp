// srt_capi.cpp -- device half of the C-ABI: one srt_ctx = one GPU's renderer
// (replaces `renderer`, rendering/rendering.cuh:39-155, and the device half of render_manager::step).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "srt_host.h"
#include "srt_internal.h"
#include "srt_light.h"

using namespace srt;

#ifndef SRT_FRINGE_STRIDE_L2
#define SRT_FRINGE_STRIDE_L2 96
#endif
static constexpr uint32_t kFringeStrideL2 = SRT_FRINGE_STRIDE_L2;
// step-choice weights when the inner tree exceeds the LDS cache (256 = an INNER visit)
static constexpr uint32_t kScoreShadeL2 = 320u, kScoreFringeL2 = 800u;   // FRINGE record stride for trees that do not fit LDS

// An owning device allocation: a pointer and its size in bytes, move-only, freed by the destructor.
// The policy of every buffer of this file, stated once:
//  * reserve() never shrinks.  When it has to grow it releases the old block first and the contents are gone; a caller that must survive
//    a refused allocation reserves a fresh buffer and moves it in (the film, srt_accum_reset_spectral).
//  * hipFree waits for the device before it releases, so no site synchronises before a buffer grows or goes.
//  * The device of the owning context must be current: every entry point selects it before it touches a buffer, srt_destroy before the
//    context -- and with it every buffer -- dies.
struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept { swap(o); }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { swap(o); return *this; }      // (the old block goes with o)
    ~DeviceBuffer() { release(); }
    void swap(DeviceBuffer &o) { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&ptr, n);
        if (e == hipSuccess) bytes = n; else ptr = nullptr;
        return e;
    }
    template <typename T> T *as() const { return static_cast<T *>(ptr); }
    explicit operator bool() const { return ptr != nullptr; }
};

// An owning block of pinned host memory (hipHostMalloc), DeviceBuffer's policy: reserve() never shrinks, and growing loses the contents.
struct PinnedBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    ~PinnedBuffer() { release(); }
    void release() { if (ptr) (void)hipHostFree(ptr); ptr = nullptr; bytes = 0; }
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&ptr, n, hipHostMallocDefault);
        if (e == hipSuccess) bytes = n; else ptr = nullptr;
        return e;
    }
};

struct srt_ctx {
    int device = 0;
    std::string err;
    // scene images in HBM (floats)
    DeviceBuffer d_nodes, d_nodes_sw, d_fringe, d_tris, d_mat_sd, d_mat_par, d_shade, d_cmf;
    DeviceBuffer d_mat_col;            // per material one float4 (srt_material.col, 0): the albedo of the first-hit features (MODE 7)
    int root_ref = 0, stack_depth = 1, n_inner = 0, n_records = 0;
    bool paired = false;               // the uploaded tree has no node with exactly one leaf child (srt_scene_is_paired)
    uint32_t fringe_stride = 96;       // bytes between FRINGE records in d_fringe
    uint32_t n_tris = 0;
    uint32_t n_materials = 0;
    bool scene_ready = false, camera_ready = false, params_ready = false;
    srt_camera_data cam;
    // launch geometry (renderer::init_device_params)
    uint32_t tx = 0, ty = 0, bx = 0, by = 0, chunk_w = 0, chunk_h = 0, spp = 0, bounce = 0;
    uint64_t seed = SRT_DEFAULT_SEED;
    uint32_t n_lanes = 0;
    uint32_t rank = 0, world = 1;
    uint32_t gather_planes = 3;          // planes of the exchange unit: 3 = the quantised framebuffer, 9 = + the parity planes
    uint32_t fb_groups_valid = 3;        // plane groups of d_fb the last scatter wrote (or all three, zeroed, right after init_device_params)
    // last chunk
    uint32_t last_w = 0, last_h = 0, last_offx = 0, last_offy = 0;
    uint32_t tiles_x = 0, tiles_y = 0, n_tiles = 0, tiles_local = 0, tiles_padded = 0;
    // buffers
    DeviceBuffer d_rng;             // 6 planes of n_lanes words
    DeviceBuffer d_fb;              // 9 block-linear planes of n_lanes floats
    DeviceBuffer d_tiles;           // compact tile buffer (floats)
    DeviceBuffer d_counters;        // [kCounters] u64 statistics + 1 word pixel-queue head behind them
    int n_cu = 256;
    uint32_t waves_per_cu = 0;                         // experiment knob (env SRT_WAVES_PER_CU)
    // step choice of a wave: serve the kind of work (shade / fringe / inner) with the most waiting lanes per unit of cost;
    // weights = 256 / relative cost of the step (inner = 256).
    // Defaults: 70 / 280 when the whole inner tree is LDS resident, 140 / 560 when inner records beyond the cache come from
    // L2 (an inner step then costs about twice as much, so the other two kinds weigh twice as much relative to it);
    // measured plateaus: profiles/r02/knob_sweeps.txt.  0 = not set by the environment.
    uint32_t score_shade = 0, score_fringe = 0;        // env SRT_SCORE_SHADE / SRT_SCORE_FRINGE
    uint32_t debug_lane_limit = 0;                     // test knob (experiments: partial tiles)
    // Test knobs (srt_set_test_knobs; from the environment -- SRT_WIDE_REFS, SRT_LDS_CACHE_MAX, SRT_DEBUG_LANE_LIMIT -- only when
    // SRT_TEST_KNOBS=1, read once here at srt_create): a stray variable in a user's shell cannot change the kernel variant that runs.
    PlanKnobs knobs;
    bool knobs_from_env = false;
    uint32_t split_load_pct = 200;                    // env SRT_SPLIT_LOAD: load factor (%) of the capacity constraint in order_tiles_kernel's split policy (0 = never split)
    uint32_t probe_spp = 2;                            // samples of the cost probe (env SRT_PROBE_SPP, 0 = no ordering)
    // queue order: tile cost moved this % towards 64 x its most expensive pixel (order_tiles_kernel).  -1 = automatic: 100 when the
    // inner tree is partly served by L2 AND the launch has fewer than 6 tiles per persistent wave (a rank's share of an 8-GPU frame:
    // every step of such a chain is an L2 round trip, and a long pixel inside an average tile ends the launch late: cfg 5 at W = 8
    // 2331 -> 2245 ms; with 8 tiles per wave -- cfg 5 at W = 4 -- it already loses: 3665 -> 3812 ms), else 0 (measured worse on LDS-resident
    // trees: cfg 3 at W = 2 187 -> 196 ms, cfg 2 44.8 -> 45.4 ms).
    // env SRT_ORDER_MAX_PCT
    int order_max_pct = -1;
    DeviceBuffer d_tile_cost, d_tile_order;            // the cost probe's schedule (TileSchedule)
    // what srt_read_tile_schedule reports: the scheduler's arguments, noted when the probe ran (n_rows and cost_max stay on the device),
    // and which queues the LAST launch ran or left behind (choose_queue)
    srt_tile_schedule_info sched_note = {};
    bool sched_probe_queue = false, sched_compacted_queue = false;
    bool count_traversal = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // The order of the context's calls (srt_c_api.h, "Order of a context's calls"; set_device, device_synchronize below): the stream of the
    // work enqueued last, remembered until the context next waits for the device, and the event that carries the order over to another stream
    hipStream_t order_stream = nullptr;
    bool order_pending = false;                         // order_stream is remembered: work since the last device-wide wait may be in flight on it
    hipEvent_t order_ev = nullptr;                      // (created on first use)
    DeviceBuffer d_rowmajor;                            // row-major staging image of srt_read_fb_rowmajor (3 planes), zeroed when its size changes
    uint32_t rowmajor_w = 0, rowmajor_h = 0;
    OrderProfile order_profile = {};                    // non-zero magic: the next instrumented launch collects the child-order profile
    DeviceBuffer d_wave_debug;                          // instrumented launches: [OrderProfile header][4 words per wave]
    uint32_t stats_spp = 0;                             // samples per pixel of the last launch when it was an accumulating pass (0: c->spp)
    bool stats_adaptive = false;                        // the last launch was an adaptive pass: srt_get_stats reads its pixel count
    // The one accumulation of a context (srt_accum_reset*, srt_render_chunk_accum).
    struct Accumulation {
        enum class State { Invalid, Empty, Bound } state = State::Invalid;   // Empty: reset, no pass yet; Bound: passes of one chunk
        enum class Kind { Plain, Adaptive, Spectral, Streams, Features, AdaptiveFeatures, SpectralFeatures, AdaptiveSpectral, AdaptiveSpectralFeatures } kind = Kind::Plain;    // MODE 3 .. 11 passes (streams combine with nothing)
        uint32_t total = 0;                             // samples per pixel in the sums (streamed: over all streams)
        uint32_t n_streams = 1;                         // streamed: the RNG streams per pixel (K); 1 otherwise
        uint32_t w = 0, h = 0, offx = 0, offy = 0;      // the chunk of the first pass
        uint32_t gathered = 0;                          // SRT_GATHER_*: what the last srt_unpack_accum since the last pass brought (whole_for)
        void invalidate() { state = State::Invalid; gathered = 0; }
        void begin(Kind k, uint32_t streams_per_pixel = 1) { kind = k; n_streams = streams_per_pixel; state = State::Empty; gathered = 0; }      // (srt_accum_reset has zeroed the total)
        bool valid() const { return state != State::Invalid; }
        bool bound() const { return state == State::Bound; }
        bool adaptive() const { return kind == Kind::Adaptive || kind == Kind::AdaptiveFeatures || kind == Kind::AdaptiveSpectral || kind == Kind::AdaptiveSpectralFeatures; }
        bool spectral() const { return kind == Kind::Spectral || kind == Kind::SpectralFeatures || kind == Kind::AdaptiveSpectral || kind == Kind::AdaptiveSpectralFeatures; }
        bool streamed() const { return kind == Kind::Streams; }
        bool featured() const { return kind == Kind::Features || kind == Kind::AdaptiveFeatures || kind == Kind::SpectralFeatures || kind == Kind::AdaptiveSpectralFeatures; }
    } accum;
    // the buffers behind it, allocated on first use:
    DeviceBuffer d_accum;                               // progressive rendering (AccumLayout)
    DeviceBuffer d_adapt;                               // adaptive sampling (srt_accum_reset_adaptive, AdaptPlanes)
    DeviceBuffer d_adapt_queue;                         // pixel queue of the next adaptive pass (AdaptQueue)
    DeviceBuffer d_film;                                // spectral film (srt_accum_reset_spectral): kFilmStride floats per lane (adaptive + spectral + features: and the rows behind it)
    DeviceBuffer d_film_staging;                        // row-major staging block of srt_read_spectral
    DeviceBuffer d_features;                            // first-hit features (srt_accum_reset_features): kFeatureStride floats per lane
    DeviceBuffer d_features_staging;                    // row-major staging block of srt_read_features
    DeviceBuffer d_denoise;                             // the denoiser's working images (DenoiseLayout), grown when the rectangle grows
    DeviceBuffer d_denoise_in;                          // srt_denoise_kat: the caller's sums and feature rows
    DeviceBuffer d_denoise_dev;                         // srt_denoise_developed: the payload images (DenoiseDevLayout), grown when rectangle or channels grow
    hipEvent_t denoise_ev[16] = {};                     // around the kernels of the last denoise: prepass | (estimator) | (despeckle) | (temporal) | (estimator | choice: srt_*_temporal_vg) | levels | epilogue (created on first use)
    uint32_t denoise_timed_levels = 0;                  // levels the events of the last denoise bracket
    uint32_t denoise_level_ev = 1;                      // the event level 0 starts at: 1, or 2 after a variance-guided denoise
    bool denoise_timed = false;
    bool denoise_estimated = false;                     // the last denoise ran a variance estimator (the event pair [denoise_est_ev, + 1] brackets it)
    uint32_t denoise_est_ev = 1;                        // the event the estimator starts at: 1, or behind the stage in srt_*_temporal_vg
    DeviceBuffer d_develop;                             // the developed film's working blocks (DevelopLayout), grown when the rectangle or the channels grow
    DeviceBuffer d_develop_in;                          // srt_develop_kat: the caller's film in 96-float rows
    hipEvent_t develop_ev[3] = {};                      // around the kernels of the last develop: contraction | sRGB epilogue (created on first use)
    bool develop_timed = false, develop_epilogue = false;
    DeviceBuffer d_expose;                              // metering and tone mapping: the global histogram and the counters (ExposeLayout)
    DeviceBuffer d_expose_in;                           // srt_meter_kat / srt_expose_kat: the caller's XYZ means
    DeviceBuffer d_expose_out;                          // the tone kernel's three row-major images, grown when the rectangle grows
    hipEvent_t expose_ev[4] = {};                       // around the last meter kernel [0, 1] and the last tone kernel [2, 3] (created on first use)
    bool meter_timed = false, tone_timed = false;
    DeviceBuffer d_present;                             // the presented picture: one packed word per pixel, and a developed source's XYZ mean (PresentLayout)
    PinnedBuffer h_present;                             // its pinned staging block on the host: the packed rectangle, the three tone counters behind it
    hipEvent_t present_ev[2] = {};                      // around the last present kernel (created on first use)
    bool present_timed = false;
    bool present_scalar = false;                        // test knob (env SRT_PRESENT_SCALAR under SRT_TEST_KNOBS=1): present_kernel's scalar path alone
    DeviceBuffer d_gather_unit;                         // srt_comm_gather_accum: this context's packed exchange unit (srt_internal_pack_accum_own)
    hipEvent_t gather_ev[4] = {};                       // around the last pack kernel [0, 1] and the last unpack kernel [2, 3] (created on first use)
    bool pack_timed = false, unpack_timed = false;
    bool gather_scalar = false;                         // test knob (env SRT_GATHER_SCALAR under SRT_TEST_KNOBS=1): gather_kernel's 4-byte paths alone
    DeviceBuffer d_despeckle;                           // the firefly filter: its counters and its four row-major images (DespeckleLayout)
    hipEvent_t despeckle_ev[2] = {};                    // around the last despeckle kernel (created on first use)
    bool despeckle_timed = false;
    // temporal reprojection (srt_temporal.hip): the history survives srt_set_camera and srt_accum_reset*, which is its point
    DeviceBuffer d_temporal_hist;                       // the double-buffered history of the last rectangle (TemporalHistory): 96 bytes per pixel
    DeviceBuffer d_temporal;                            // the stage's counters and its row-major output images (TemporalLayout)
    DeviceBuffer d_temporal_kat;                        // srt_temporal_kat: the caller's arrays and the history it gets back (TemporalKatLayout)
    uint32_t temporal_frames = 0;                       // calls since the history began (0: there is none)
    uint32_t temporal_cur = 0;                          // the half of d_temporal_hist the last call wrote
    uint32_t temporal_rect[4] = {0, 0, 0, 0};           // w, h, offx, offy of the history's rectangle
    srt_camera_data temporal_cam = {};                  // the camera that was current when the history was written
    hipEvent_t temporal_ev[2] = {};                     // around the last temporal kernel (created on first use)
    bool temporal_timed = false;
    // ... its moments (srt_*_temporal_vg): allocated by the first call that asks for them
    DeviceBuffer d_temporal_mom;                        // the double-buffered moments history Hm (TemporalMoments): 32 bytes per pixel, halves indexed as d_temporal_hist's
    bool temporal_moments = false;                      // the last call that advanced the history wrote Hm (it is present while temporal_frames > 0)
    DeviceBuffer d_temporal_var;                        // the choice kernel's counter; srt_temporal_variance_kat: and the caller's arrays (TemporalVarianceKatLayout)
    hipEvent_t temporal_var_ev[2] = {};                 // around the last choice kernel (created on first use)
    bool temporal_var_timed = false;
    // BVH refit (srt_refit.hip).  The topology tables are made on the host by srt_upload_scene (RefitParams states them), copied to the
    // device by the first refit after an upload; tables, scratch and staging belong to the context and are reused.
    std::vector<uint32_t> refit_tri_tab, refit_sched;   // two words per triangle; the record indices grouped by height
    std::vector<int32_t> refit_child;                   // two references per record
    std::vector<uint32_t> refit_level_first;            // height h (1 ..) owns sched[first[h - 1] .. first[h])
    bool refit_tables_ok = false;                       // the tables describe the uploaded scene
    bool refit_tables_on_device = false;                // ... and d_refit_tab holds them
    DeviceBuffer d_refit_tab;                           // RefitTables
    DeviceBuffer d_refit_scratch;                       // RefitScratch: the validation count, the leaf boxes, the records' own boxes
    DeviceBuffer d_refit_verts;                         // srt_refit_vertices: the caller's vertices
    size_t image_bytes[5] = {0, 0, 0, 0, 0};            // bytes of the uploaded scene images, by SRT_IMAGE_* (0: the plan keeps none)
    hipEvent_t refit_ev[3] = {};                        // around the last refit's triangle kernel [0, 1] and its level launches [1, 2] (created on first use)
    uint32_t refit_timed_levels = 0;
    bool refit_timed = false;
    // surface motion (srt_motion.hip; srt_c_api.h states the vertex state at "Surface motion").  Nothing below exists while tracking is off.
    bool track_motion = false;                          // srt_temporal_track_motion
    enum class Verts { Unknown, Host, Device } verts = Verts::Unknown;      // where V_cur is: nowhere, in track_verts (since an upload), in d_verts_cur
    std::vector<float> track_verts;                     // V_cur between srt_upload_scene and its first use: 9 floats per triangle
    DeviceBuffer d_verts_cur, d_verts_hist;             // V_cur and V_hist on the device
    bool verts_hist = false;                            // V_hist is not "none" (none = equal to V_cur)
    uint32_t refits_pending = 0;                        // successful refits since the history was last written
    DeviceBuffer d_motion;                              // the pass's counters and its row-major outputs (MotionLayout)
    DeviceBuffer d_motion_kat;                          // srt_surface_motion_kat: the caller's two vertex arrays
    hipEvent_t motion_ev[2] = {};                       // around the last motion kernel (created on first use)
    bool motion_timed = false;
    // batched ray queries (srt_query.hip; srt_c_api.h, "Ray queries")
    DeviceBuffer d_query;                               // the kernel's 32-bit ray counter (256 B)
    DeviceBuffer d_query_io;                            // the host entries' staging: the rays, then the answers
    hipEvent_t query_ev[2] = {};                        // around the last query kernel (created on first use)
    bool query_timed = false;
    srt_query_info query_info = {};                     // the plan of the last query launch (ms filled in by srt_query_last)
    uint32_t query_max_waves = 0;                       // srt_set_query_test_grid (0: fill the device)
    // direct lighting (srt_light.hip; srt_c_api.h, "Direct lighting").  The upload keeps what the host tables are made from; the tables
    // and their device copy are made at the first use after it.
    struct LightSource { uint32_t tri, mat; float v0[3], v1[3], v2[3], n[3]; };
    std::vector<LightSource> light_src;                 // the triangles with an EMISSIVE material, in scene order
    std::vector<srt_material> light_mats;               // the uploaded materials
    float light_bg[SRT_N_CIE_SAMPLES] = {};             // the uploaded background
    bool light_refitted = false;                        // a refit moved the vertices since the upload: the table's areas are stale
    bool light_tables_ok = false;                       // the host tables below describe the uploaded scene
    bool light_tables_on_device = false;                // ... and d_light_tab holds them
    std::vector<uint32_t> light_thresholds;             // [lights + 1]
    std::vector<float> light_records;                   // [lights][16]
    std::vector<float> light_t_light, light_t_sky, light_t_emit;      // [mats][slots][3], [mats][3], [mats][3]
    float light_t_bg[3] = {0.f, 0.f, 0.f};
    uint32_t light_slots = 0;
    bool light_bg_nonzero = false;
    DeviceBuffer d_light_tab;                           // LightTables
    DeviceBuffer d_light_work;                          // LightWork: the round's rows, records and occlusion bytes
    DeviceBuffer d_light_out;                           // LightOut: the counters, sum and m2 of the call's rectangle
    hipEvent_t light_ev[6] = {};                        // around the kernels of a round (created on first use)
    srt_light_info light_info = {};
    bool light_timed = false;
    uint32_t light_max_rows = 0;                        // srt_set_light_test_batch (0: the budget)
    DeviceBuffer d_streams;                            // sample-parallel pixels (srt_accum_reset_streams, StreamPlanes)
    uint32_t streams_seeded = 0;                        // the K whose RNG streams d_streams holds, seeded since the last srt_init_device_params (0: none)
};

namespace {

// Optional roctx ranges around the phases of srt_render_chunk (cost probe, queue build, render launch): they show up in
// rocprofv3 --marker-trace timelines next to the kernels.  libroctx64 is looked up once with dlopen; absent library = no ranges.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char *n : {"libroctx64.so.4", "libroctx64.so", "/opt/rocm/lib/libroctx64.so.4"}) {
            if (void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL)) {
                push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
                pop = (int (*)())dlsym(h, "roctxRangePop");
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
struct RoctxRange {
    static Roctx &api() { static Roctx r; return r; }
    explicit RoctxRange(const char *name) { if (api().push) api().push(name); }
    ~RoctxRange() { if (api().pop) api().pop(); }
};

int fail(srt_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    set_global_error(msg);
    return code;
}
int hip_fail(srt_ctx *ctx, hipError_t e, const char *what) {
    return fail(ctx, SRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY_AS(ctx, what, expr) do { if (hipError_t _e = (expr)) return hip_fail(ctx, _e, what); } while (0)
#define HIP_TRY(ctx, expr) HIP_TRY_AS(ctx, #expr, expr)

// ---- the order of a context's calls (srt_c_api.h): they take effect in the order they were made, whichever streams they name --------
// Passes, srt_copy_tile_buffer and srt_scatter_tiles run on the caller's stream, everything else on the null stream, and a blocking
// copy orders against the null stream only -- which serialises with the caller's blocking streams, not with a hipStreamNonBlocking one.
// So every entry point that enqueues selects the device through set_device(c, its stream): when the context's last work went to ANOTHER
// stream and may still be in flight, the new stream first waits for an event recorded behind that work.  A caller that stays on one
// stream never gets here: no HIP call is added.  The remembered stream is not touched again after the context's next device-wide wait
// (device_synchronize), so the caller may destroy it then.
hipError_t set_device(srt_ctx *c, hipStream_t st = nullptr) {
    if (const hipError_t e = hipSetDevice(c->device)) return e;
    if (c->order_pending && c->order_stream != st) {
        if (!c->order_ev)
            if (const hipError_t e = hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming)) return e;
        if (const hipError_t e = hipEventRecord(c->order_ev, c->order_stream)) return e;
        if (const hipError_t e = hipStreamWaitEvent(st, c->order_ev, 0)) return e;
    }
    c->order_stream = st; c->order_pending = true;
    return hipSuccess;
}
// every device-wide wait of a context: nothing of it is in flight afterwards, on any stream
hipError_t device_synchronize(srt_ctx *c) {
    const hipError_t e = hipDeviceSynchronize();
    c->order_stream = nullptr; c->order_pending = false;
    return e;
}

int upload(srt_ctx *ctx, DeviceBuffer &dst, const std::vector<float> &src) {
    HIP_TRY(ctx, dst.reserve(src.size() * sizeof(float)));
    HIP_TRY(ctx, hipMemcpy(dst.ptr, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
    return SRT_OK;
}

// ---- the layouts of the composite buffers: each is taken apart here and nowhere else ------------------------------------------

// The refit's topology tables on the device: [tri_tab: 2 words per triangle | child: 2 per record | sched: 1 per record]
struct RefitTables {
    uint32_t *tri_tab, *sched;
    int32_t *child;
    static size_t bytes(size_t n_tris, size_t n_records) { return (2 * n_tris + 3 * n_records) * sizeof(uint32_t); }
    RefitTables(const DeviceBuffer &d, size_t n_tris, size_t n_records)
        : tri_tab(d.as<uint32_t>()), sched(tri_tab + 2 * n_tris + 2 * n_records), child(reinterpret_cast<int32_t *>(tri_tab + 2 * n_tris)) {}
};
// The refit's scratch: [count: the validation kernel's word, 256 B | leaf boxes: 6 floats per triangle | own boxes: 6 per record]
struct RefitScratch {
    static constexpr size_t kCountBytes = 256;
    uint32_t *count;
    float *leaf_box, *rec_box;
    static size_t bytes(size_t n_tris, size_t n_records) { return kCountBytes + 6 * (n_tris + n_records) * sizeof(float); }
    RefitScratch(const DeviceBuffer &d, size_t n_tris)
        : count(d.as<uint32_t>()), leaf_box(reinterpret_cast<float *>(d.as<char>() + kCountBytes)), rec_box(leaf_box + 6 * n_tris) {}
};

// The refit's tables (refit_topology, srt_host.cpp) into the context; host only
void build_refit_tables(srt_ctx *c, const FlatScene &f, const srt_scene &s) {
    static_assert(kRefitNoSlot == kRefitTopologyNoSlot, "the kernel's and the host's marker of a triangle without a FRINGE block");
    RefitTopology t;
    refit_topology(f, s, t);
    c->refit_tri_tab.swap(t.tri_tab); c->refit_child.swap(t.child); c->refit_sched.swap(t.sched); c->refit_level_first.swap(t.level_first);
    c->refit_tables_ok = t.ok;
}

// What the direct-light tables are made from (srt_c_api.h, "Direct lighting"), copied out of the scene; host only
void keep_light_sources(srt_ctx *c, const srt_scene &s) {
    c->light_tables_ok = false; c->light_tables_on_device = false; c->light_refitted = false;
    c->light_mats = s.mats;
    memcpy(c->light_bg, s.background, sizeof(c->light_bg));
    c->light_src.clear();
    for (size_t k = 0; k < s.raw.size(); k++) {
        const uint32_t m = s.raw[k].mat_index;
        if (m >= s.mats.size() || s.mats[m].material_type != (uint32_t)SRT_MAT_EMISSIVE) continue;
        srt_ctx::LightSource l;
        l.tri = (uint32_t)k; l.mat = m;
        memcpy(l.v0, s.raw[k].v0, sizeof(l.v0)); memcpy(l.v1, s.raw[k].v1, sizeof(l.v1)); memcpy(l.v2, s.raw[k].v2, sizeof(l.v2));
        memcpy(l.n, s.rec[k].n, sizeof(l.n));
        c->light_src.push_back(l);
    }
}

// The cost probe's schedule.  d_tile_order: [rows: up to 64 per tile][sorted tile ids][queue_info 4 words]; d_tile_cost: per local tile
// its cost, then the cost of its most expensive pixel.
struct TileSchedule {
    uint32_t *rows = nullptr, *sorted = nullptr, *info = nullptr, *cost = nullptr;
    static size_t order_bytes(size_t tiles) { return (tiles * 65 + 4) * sizeof(uint32_t); }
    static size_t cost_bytes(size_t tiles) { return 2 * tiles * sizeof(uint32_t); }
    explicit TileSchedule(const srt_ctx *c) : cost(c->d_tile_cost.as<uint32_t>()) {
        if (!c->d_tile_order) return;
        const size_t tiles = (c->d_tile_order.bytes / sizeof(uint32_t) - 4) / 65;      // the tiles the buffer was reserved for
        rows = c->d_tile_order.as<uint32_t>(); sorted = rows + tiles * 64; info = sorted + tiles;
    }
};

// Pixel queue of the next adaptive pass: [queue_info 4 words | counts: 1 x u64 + pad | rows | flags], as many flags as rows.
// counts: the pixels that rendered in the pass that just ended in the low half, those still active in the high half (adapt_flag_kernel).
struct AdaptQueue {
    uint32_t *info, *rows, *flags;
    unsigned long long *counts;
    static size_t bytes(size_t n_rows) { return (8 + 2 * n_rows) * sizeof(uint32_t); }
    explicit AdaptQueue(const DeviceBuffer &d_adapt_queue)      // (an allocated one)
        : info(d_adapt_queue.as<uint32_t>()), rows(info + 8), flags(rows + (d_adapt_queue.bytes / sizeof(uint32_t) - 8) / 2),
          counts(reinterpret_cast<unsigned long long *>(info + 4)) {}
};
int read_adapt_counts(srt_ctx *c, uint64_t *rendered, uint64_t *active) {      // (either may be null)
    unsigned long long counts = 0;
    HIP_TRY(c, hipMemcpy(&counts, AdaptQueue(c->d_adapt_queue).counts, sizeof(counts), hipMemcpyDeviceToHost));
    if (rendered) *rendered = counts & 0xffffffffull;
    if (active) *active = counts >> 32;
    return SRT_OK;
}

// Progressive rendering: [AccumHeader | pad to 256 B | X Y Z planes of n_lanes floats]
struct AccumLayout {
    static constexpr size_t kAccumHeaderBytes = 256;      // the sum planes start behind the header, 256-byte aligned
    AccumHeader *header;
    float *sums, *y;
    static size_t sums_bytes(size_t lanes) { return 3 * lanes * sizeof(float); }
    static size_t bytes(size_t lanes) { return kAccumHeaderBytes + sums_bytes(lanes); }
    explicit AccumLayout(const srt_ctx *c)
        : header(c->d_accum.as<AccumHeader>()), sums(reinterpret_cast<float *>(c->d_accum.as<char>() + kAccumHeaderBytes)), y(sums + c->n_lanes) {}
};
// MODE 3 / 4 / 5 read their AccumHeader where the instrumented build keeps its debug words (srt_internal.h, AccumHeader)
void set_accum_header(RenderParams &p, AccumHeader *h) { p.wave_debug = reinterpret_cast<uint32_t *>(h); }

// Adaptive sampling: [S2 plane | state plane] of n_lanes words
struct AdaptPlanes {
    float *sum2;
    uint32_t *state;
    static size_t bytes(size_t lanes) { return 2 * lanes * sizeof(float); }
    explicit AdaptPlanes(const srt_ctx *c) : sum2(c->d_adapt.as<float>()), state(c->d_adapt.as<uint32_t>() + c->n_lanes) {}
};

// Sample-parallel pixels (AccumHeader::stream_planes): [RNG state: 6 planes | XYZ sums: 3 planes] of K * n_lanes words, stream k of lane
// idx at k * n_lanes + idx
struct StreamPlanes {
    uint32_t *rng;
    float *sums;
    static size_t sums_bytes(size_t lanes, size_t k) { return 3 * k * lanes * sizeof(float); }
    static size_t bytes(size_t lanes, size_t k) { return kStreamSumPlane * k * lanes * sizeof(uint32_t) + sums_bytes(lanes, k); }
    StreamPlanes(const DeviceBuffer &d_streams, size_t lanes, size_t k) : rng(d_streams.as<uint32_t>()), sums(d_streams.as<float>() + kStreamSumPlane * k * lanes) {}
};

// The last chunk clipped to the reference grid, and its rectangle clipped to an image as well: w x h pixels whose first one has index
// `first` in the row-major image (w = h = 0: the chunk lies outside the image).
uint32_t clipped_w(const srt_ctx *c) { return std::min<uint32_t>(c->last_w, c->tx * c->bx); }
uint32_t clipped_h(const srt_ctx *c) { return std::min<uint32_t>(c->last_h, c->ty * c->by); }
struct ChunkRect { uint32_t w, h; size_t first; };
ChunkRect chunk_rect(const srt_ctx *c, uint32_t image_width, uint32_t image_height) {
    if (c->last_offx >= image_width || c->last_offy >= image_height) return {0, 0, 0};
    return {std::min<uint32_t>(clipped_w(c), image_width - c->last_offx), std::min<uint32_t>(clipped_h(c), image_height - c->last_offy),
            (size_t)c->last_offy * image_width + c->last_offx};
}

// Instrumented launches: the waves d_wave_debug has words for behind its OrderProfile header
size_t wave_debug_bytes(size_t n_waves) { return sizeof(OrderProfile) + n_waves * 4 * sizeof(uint32_t); }
uint32_t wave_debug_waves(const srt_ctx *c) { return c->d_wave_debug ? (uint32_t)((c->d_wave_debug.bytes - sizeof(OrderProfile)) / (4 * sizeof(uint32_t))) : 0u; }

float *fb_plane(const srt_ctx *c, int k) { return c->d_fb.as<float>() + (size_t)k * c->n_lanes; }      // 0 .. 8: r g b | lin r g b | X Y Z

// what launch_render will do for the uploaded scene
LaunchPlan plan_of(const srt_ctx *c) { LaunchPlan lp; render_launch_plan(c->stack_depth, c->n_records, c->n_inner, c->knobs, lp); return lp; }

void fill_params(const srt_ctx *c, RenderParams &p) {
    memset(&p, 0, sizeof(p));
    p.nodes = c->d_nodes.as<const float4>(); p.nodes_sw = c->d_nodes_sw.as<const float>(); p.fringe = c->d_fringe.as<const float4>(); p.tris = c->d_tris.as<const float4>();
    p.mat_sd = c->d_mat_sd.as<const float2>(); p.mat_par = c->d_mat_par.as<const float4>();
    p.shade = c->d_shade.as<const float4>(); p.cmf = c->d_cmf.as<const float4>();
    p.root_ref = c->root_ref; p.stack_depth = c->stack_depth; p.n_materials = c->n_materials;
    p.n_inner = c->n_inner; p.n_cached = 0;   // n_cached is set by the launcher
    p.n_tris = c->n_tris; p.n_records = c->n_records; p.fringe_stride = c->fringe_stride;
    p.paired = c->paired ? 1u : 0u;
    for (int k = 0; k < 3; k++) {
        p.du[k] = c->cam.pixel_delta_u[k]; p.dv[k] = c->cam.pixel_delta_v[k]; p.p00[k] = c->cam.pixel00_loc[k];
        p.center[k] = c->cam.camera_center[k]; p.disk_u[k] = c->cam.defocus_disk_u[k]; p.disk_v[k] = c->cam.defocus_disk_v[k];
    }
    p.defocus_angle = c->cam.defocus_angle;
    p.tx = c->tx; p.ty = c->ty; p.bx = c->bx; p.by = c->by;
    p.spp = c->spp; p.bounce_limit = c->bounce;
    p.rank = c->rank; p.world = c->world;
    p.rng = c->d_rng.as<uint32_t>(); p.n_lanes = c->n_lanes;
    p.tile_out = c->d_tiles.as<float>(); p.counters = c->d_counters.as<unsigned long long>();
    p.tile_group_stride = c->tiles_padded * (uint32_t)(kGroupPlanes * kTileLanes);
    p.write_parity = c->gather_planes == (uint32_t)kTilePlanes ? 1u : 0u;
}

// ---- srt_render_chunk's body, in phases.  Each takes the context, what the phases share (Pass) and the RenderParams under construction.

struct Pass {
    uint32_t spp_add;          // 0: a plain launch of c->spp samples; > 0: an accumulating pass of spp_add samples
    hipStream_t st;
    RenderMode mode;           // of the render launch
    bool later;                // a pass of a Bound accumulation: not its first
    LaunchPlan plan;
    bool ordered;              // the launch runs the cost probe's queue, fresh or reused (choose_queue)
    uint32_t adapt_bound;      // adaptive passes: host-side bound of the rows of their queues (choose_queue)
    uint32_t streams;          // streamed passes: K, the copies of every queue row (one per stream); 1 otherwise
};

// MODE 4, 8, 10 and 11 share everything around the launch
bool adaptive_mode(RenderMode m) { return m == Adaptive || m == AdaptiveFeatures || m == AdaptiveSpectral || m == AdaptiveSpectralFeatures; }
uint32_t split_rows_bound(const srt_ctx *c) { return (uint32_t)std::min<uint64_t>((uint64_t)c->tiles_local * 64, 0x7fffffffull); }
// The queue head is a 32-bit pixel-slot counter, and a streamed pass runs K copies of every row: its tiles are split only where even
// the finest split of every tile stays below 2^32 slots; srt_render_chunk_accum refuses a pass whose UNsplit rows do not.
constexpr uint64_t kQueueSlots = 1ull << 32;
bool queue_may_split(const srt_ctx *c, uint32_t streams) { return c->split_load_pct && (streams == 1 || (uint64_t)split_rows_bound(c) * streams * 64 < kQueueSlots); }

// Tile geometry and the compact tile buffer.
// (the geometry: a function of the grid and the partition alone: a pass can be refused on it before anything is enqueued)
void tile_geometry(srt_ctx *c) {
    // Tiles cover every pixel the reference grid can address, whatever the size of THIS chunk: the tile number of a lane
    // idx -- and with it the rank that owns the lane's persistent RNG stream (Q13) -- must not move when a ragged edge
    // chunk is narrower than the one before.  Tiles (partly) outside the chunk just skip those pixels (rendering.cu:205).
    const uint32_t cover_w = c->tx * c->bx, cover_h = c->ty * c->by;
    c->tiles_x = (cover_w + 7) / 8; c->tiles_y = (cover_h + 7) / 8;
    c->n_tiles = c->tiles_x * c->tiles_y;
    c->tiles_padded = (c->n_tiles + c->world - 1) / c->world;
    c->tiles_local = c->n_tiles > c->rank ? (c->n_tiles - c->rank + c->world - 1) / c->world : 0;
}

int prepare_tiles(srt_ctx *c, const Pass &ps) {
    tile_geometry(c);
    const size_t tile_floats = (size_t)std::max<uint32_t>(c->tiles_padded, 1) * kTileLanes;      // per plane
    HIP_TRY(c, c->d_tiles.reserve(tile_floats * kTilePlanes * sizeof(float)));
    // (only the plane groups this launch writes: group 0, or all three when the parity planes were asked for.  Not on the later passes
    // of an adaptive accumulation: their converged pixels keep the slots they wrote last)
    if (!(adaptive_mode(ps.mode) && ps.later)) HIP_TRY(c, hipMemsetAsync(c->d_tiles.ptr, 0, tile_floats * c->gather_planes * sizeof(float), ps.st));
    HIP_TRY(c, hipMemsetAsync(c->d_counters.ptr, 0, (kCounters + 1) * sizeof(unsigned long long), ps.st));
    return SRT_OK;
}

// The launch's parameters up to the pixel queue, which starts as the identity order.
void chunk_params(const srt_ctx *c, const Pass &ps, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy, RenderParams &p) {
    fill_params(c, p);
    if (ps.spp_add) p.spp = ps.spp_add / ps.streams;      // the samples this pass adds, per stream (the running total is in the header)
    p.width = width; p.height = height; p.offx = offx; p.offy = offy;
    p.tiles_x = c->tiles_x; p.tiles_y = c->tiles_y; p.n_tiles = c->n_tiles;
    p.tiles_local = c->tiles_local;
    p.pixel_counter = reinterpret_cast<uint32_t *>(c->d_counters.as<unsigned long long>() + kCounters);
    p.waves_per_cu_override = c->waves_per_cu;
    const bool all_cached = ps.plan.all_cached;
    // (inner records that come from L2 make an INNER visit ~2x as expensive, so shading and FRINGE visits weigh more:
    // plateau 280-400 / 560-1100 on cfg 5's scene, 60-85 / 280-340 on cfg 2 / 3 / 4, profiles/r02/knob_sweeps.txt)
    p.score_shade = c->score_shade ? c->score_shade : (all_cached ? 70u : kScoreShadeL2);
    // (the PAIRED variant's FRINGE visit is a fifth cheaper: plateau 340-480 on cfg 3, profiles/r05/experiments/weights_paired.txt)
    const bool paired = render_paired_variant(c->paired, render_narrow_refs(c->n_records, c->knobs), all_cached);
    p.score_fringe = c->score_fringe ? c->score_fringe : (all_cached ? (paired ? 400u : 280u) : kScoreFringeL2);
    p.tile_order = nullptr; p.tile_cost = nullptr; p.queue_rows = nullptr; p.queue_rows_bound = c->tiles_local;
    p.debug_lane_limit = c->debug_lane_limit;
}

// The cost probe: probe_spp samples per pixel from a copy of the RNG state, nothing written, then the queue built on the device.
// `p`: the launch's parameters with the identity queue.
int run_cost_probe(srt_ctx *c, const Pass &ps, const RenderParams &p) {
    HIP_TRY(c, c->d_tile_cost.reserve(TileSchedule::cost_bytes(c->tiles_local)));
    HIP_TRY(c, c->d_tile_order.reserve(TileSchedule::order_bytes(c->tiles_local)));
    const TileSchedule sched(c);
    HIP_TRY(c, hipMemsetAsync(sched.cost, 0, TileSchedule::cost_bytes(c->tiles_local), ps.st));
    RenderParams pp = p;
    pp.spp = c->probe_spp; pp.tile_cost = sched.cost;
    RoctxRange range_probe("srt cost probe + pixel queue");
    HIP_TRY(c, launch_render(pp, c->knobs, (uint32_t)c->n_cu, Probe, ps.st));
    // (a streamed pass runs K copies of every row, each a chain of 1/K of the pixel's samples: the split policy's latency and capacity
    // constraints, with T the makespan of the UNsplit streams, are those of a machine of n_waves / K waves -- order_tiles_kernel)
    const uint32_t n_waves_plan = std::max<uint32_t>((uint32_t)c->n_cu * (uint32_t)ps.plan.waves_per_cu / ps.streams, 1u);
    const uint32_t order_pct = c->order_max_pct >= 0 ? (uint32_t)c->order_max_pct : ((!ps.plan.all_cached && (uint64_t)c->tiles_local < 6ull * n_waves_plan) ? 100u : 0u);
    const uint32_t split_pct = queue_may_split(c, ps.streams) ? c->split_load_pct : 0u;
    HIP_TRY(c, launch_order_tiles(sched.cost, sched.sorted, sched.rows, c->tiles_local, n_waves_plan, split_pct, sched.info, order_pct, ps.st));   // device-side, no host sync
    c->sched_note = {};
    c->sched_note.tiles_local = c->tiles_local; c->sched_note.n_waves_plan = n_waves_plan; c->sched_note.split_load_pct = split_pct;
    c->sched_note.order_max_pct = order_pct; c->sched_note.streams = ps.streams;
    HIP_TRY(c, hipMemsetAsync(c->d_counters.as<unsigned long long>() + kCounters, 0, sizeof(unsigned long long), ps.st));   // rewind the queue head
    return SRT_OK;
}

// ---- cost-ordered pixel queue --------------------------------------------------------------------------------
// A pixel is one sequential RNG stream, so the launch cannot finish before its most expensive pixel does.  A short
// probe (probe_spp samples per pixel from a copy of the RNG state, nothing written) measures the traversal cost of
// every tile; order_tiles_kernel then builds the queue on the device: tiles in descending cost order
// (longest-processing-time-first), the most expensive ones split over several waves when the launch is chain-bound.
enum class QueueSource { Identity, FreshProbe, ReusedProbe, Compacted };

QueueSource queue_source(const srt_ctx *c, const Pass &ps) {
    // (adaptive passes after the first: the queue the previous pass compacted -- the probe's rows, or the identity order, whose tiles
    // still hold an active pixel.  A queue row has a 22-bit tile field: beyond that the pass runs the plain identity queue, and its
    // converged pixels are only skipped at the fetch)
    if (adaptive_mode(ps.mode) && ps.later && c->tiles_local <= kQueueTileMask) return QueueSource::Compacted;
    if (!ps.ordered) return QueueSource::Identity;
    // (accumulating passes: the probe runs on the FIRST pass whatever its sample count -- short passes would otherwise run an unordered
    // queue -- and the later passes of the accumulation reuse its queue: a tile's cost depends on its geometry, not on the sample index,
    // and nothing else writes the schedule buffers before the accumulation is invalidated)
    return ps.later ? QueueSource::ReusedProbe : QueueSource::FreshProbe;
}

int choose_queue(srt_ctx *c, Pass &ps, RenderParams &p) {
    const bool schedulable = c->probe_spp > 0 && c->tiles_local > 1 && c->tiles_local <= kQueueTileMask;   // the tile field of a queue row
    ps.ordered = schedulable && (ps.spp_add || c->spp > 4 * c->probe_spp);
    ps.adapt_bound = ps.ordered && c->split_load_pct ? split_rows_bound(c) : c->tiles_local;      // (adaptive passes are never streamed)
    if (adaptive_mode(ps.mode)) HIP_TRY(c, c->d_adapt_queue.reserve(AdaptQueue::bytes(std::max<uint32_t>(ps.adapt_bound, 1u))));
    const QueueSource src = queue_source(c, ps);
    c->sched_probe_queue = false; c->sched_compacted_queue = false;      // (srt_read_tile_schedule: set again below and by compact_adaptive_queue)
    if (src == QueueSource::Compacted) {
        const AdaptQueue q(c->d_adapt_queue);
        p.tile_order = q.rows;
        p.queue_rows = q.info;
        p.prio_cost = ps.ordered ? c->d_tile_cost.as<uint32_t>() : nullptr;
        p.queue_rows_bound = ps.adapt_bound;
    } else if (src != QueueSource::Identity) {      // (the identity queue: chunk_params)
        if (src == QueueSource::FreshProbe)
            if (const int rc = run_cost_probe(c, ps, p)) return rc;
        const TileSchedule sched(c);
        p.tile_order = sched.rows;
        p.queue_rows = sched.info;
        p.prio_cost = sched.cost;      // wave priorities of the render launch (render_kernel, LDS-resident trees)
        if (queue_may_split(c, ps.streams)) p.queue_rows_bound = split_rows_bound(c);
    }
    c->sched_probe_queue = ps.ordered && src != QueueSource::Identity;      // (a compacted queue of an ordered accumulation: the probe's is its source)
    p.queue_rows_bound *= ps.streams;      // (after the probe, which walks the tiles themselves)
    return SRT_OK;
}

// The instrumented launch's debug buffer.
int bind_wave_debug(srt_ctx *c, const Pass &ps, RenderParams &p) {
    if (!c->count_traversal) return SRT_OK;
    // layout of the debug buffer: [OrderProfile header][4 words per wave]: the header sits at a FIXED place, so the kernel finds it
    // whatever number of waves the launcher ends up starting.  Sized from the launcher's own grid arithmetic WITHOUT the clamp to the
    // queue's rows (every CU filled, rounded up to whole workgroups): no queue of this plan can start more waves
    const uint32_t most_waves = render_launch_grid(ps.plan, (uint32_t)c->n_cu, p.waves_per_cu_override, UINT32_MAX).waves;
    HIP_TRY(c, c->d_wave_debug.reserve(wave_debug_bytes(most_waves)));
    HIP_TRY(c, hipMemsetAsync(c->d_wave_debug.ptr, 0, c->d_wave_debug.bytes, ps.st));
    p.wave_debug = c->d_wave_debug.as<uint32_t>();
    if (c->order_profile.magic == kOrderProfileMagic || c->order_profile.seg != nullptr)
        HIP_TRY(c, hipMemcpyAsync(c->d_wave_debug.ptr, &c->order_profile, sizeof(OrderProfile), hipMemcpyHostToDevice, ps.st));
    return SRT_OK;
}

int launch_pass(srt_ctx *c, const Pass &ps, RenderParams &p) {
    // (nothing is enqueued for a launch whose waves the debug buffer cannot hold: the kernel writes 4 words per wave it starts)
    if (c->count_traversal && render_launch_grid(ps.plan, (uint32_t)c->n_cu, p.waves_per_cu_override, p.queue_rows_bound).waves > wave_debug_waves(c))
        return fail(c, SRT_ERR_HIP, "srt_render_chunk: the launch started more waves than the debug buffer holds (launch plan and launcher disagree)");
    HIP_TRY(c, hipEventRecord(c->ev0, ps.st));     // ev0..ev1 bracket the render kernel alone (roofline.achieved)
    if (ps.spp_add) set_accum_header(p, AccumLayout(c).header);
    HIP_TRY(c, launch_render(p, c->knobs, (uint32_t)c->n_cu, ps.mode, ps.st));
    HIP_TRY(c, hipEventRecord(c->ev1, ps.st));
    return SRT_OK;
}

// After an adaptive pass: the next pass's queue, from the probe's queue (kept intact for the whole accumulation) or the identity order;
// the same kernels count the pixels that rendered in this pass and those still active (srt_get_stats, srt_accum_active)
int compact_adaptive_queue(srt_ctx *c, const Pass &ps, const RenderParams &p) {
    const TileSchedule sched(c);
    const AdaptQueue dst(c->d_adapt_queue);
    AdaptQueueParams q = {};
    q.src_rows = ps.ordered ? sched.rows : nullptr; q.src_info = ps.ordered ? sched.info : nullptr; q.n_identity = c->tiles_local;
    q.dst_info = dst.info; q.dst_rows = dst.rows; q.flags = dst.flags; q.counts = dst.counts;
    q.state = AdaptPlanes(c).state;
    q.spp_total = c->accum.total + ps.spp_add;
    q.width = p.width; q.height = p.height; q.tx = c->tx; q.ty = c->ty; q.bx = c->bx; q.by = c->by;
    q.tiles_x = c->tiles_x; q.n_tiles = c->n_tiles; q.rank = c->rank; q.world = c->world;
    q.lane_limit = c->debug_lane_limit ? c->debug_lane_limit : 64u;
    HIP_TRY(c, hipMemsetAsync(q.counts, 0, sizeof(unsigned long long), ps.st));
    HIP_TRY(c, launch_adapt_queue(q, ps.adapt_bound, ps.st));
    c->sched_compacted_queue = true;
    return SRT_OK;
}

// After a streamed pass: the K sums of every pixel added in stream order, and the tile buffer written from the result
int combine_streams(srt_ctx *c, const Pass &ps, const RenderParams &p) {
    StreamCombineParams q = {};
    q.stream_sums = StreamPlanes(c->d_streams, c->n_lanes, ps.streams).sums; q.sums = AccumLayout(c).sums; q.tile_out = p.tile_out;
    q.streams = ps.streams; q.spp_total = c->accum.total + ps.spp_add; q.n_lanes = c->n_lanes;
    q.tile_group_stride = p.tile_group_stride; q.write_parity = p.write_parity; q.tiles_local = c->tiles_local;
    q.width = p.width; q.height = p.height; q.tx = c->tx; q.ty = c->ty; q.bx = c->bx; q.by = c->by;
    q.tiles_x = c->tiles_x; q.n_tiles = c->n_tiles; q.rank = c->rank; q.world = c->world;
    q.lane_limit = c->debug_lane_limit ? c->debug_lane_limit : 64u;
    HIP_TRY(c, launch_stream_combine(q, ps.st));
    return SRT_OK;
}

// spp_add == 0: a plain launch of c->spp samples (Plain, or Counting when instrumented); spp_add > 0: an accumulating pass of spp_add
// samples (Accum / Adaptive / Spectral / Streams / Features / AdaptiveFeatures / SpectralFeatures / AdaptiveSpectral / AdaptiveSpectralFeatures) whose caller has checked the accumulation and enqueued its header.
// width .. offy are already narrowed to 16 bit.
int render_chunk_impl(srt_ctx *c, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy, uint32_t spp_add, hipStream_t st) {
    Pass ps = {};
    ps.spp_add = spp_add; ps.st = st;
    ps.mode = !spp_add ? (c->count_traversal ? Counting : Plain) : c->accum.adaptive() ? (c->accum.spectral() ? (c->accum.featured() ? AdaptiveSpectralFeatures : AdaptiveSpectral) : c->accum.featured() ? AdaptiveFeatures : Adaptive) : c->accum.spectral() ? (c->accum.featured() ? SpectralFeatures : Spectral) : c->accum.streamed() ? Streams : c->accum.featured() ? Features : Accum;
    ps.later = spp_add && c->accum.bound(); ps.plan = plan_of(c);
    ps.streams = ps.mode == Streams ? c->accum.n_streams : 1u;
    c->last_w = width; c->last_h = height; c->last_offx = offx; c->last_offy = offy;
    RenderParams p;
    if (const int rc = prepare_tiles(c, ps)) return rc;
    chunk_params(c, ps, width, height, offx, offy, p);
    if (const int rc = choose_queue(c, ps, p)) return rc;
    if (const int rc = bind_wave_debug(c, ps, p)) return rc;
    RoctxRange range_render("srt render_kernel");
    if (const int rc = launch_pass(c, ps, p)) return rc;
    if (adaptive_mode(ps.mode))
        if (const int rc = compact_adaptive_queue(c, ps, p)) return rc;
    if (ps.mode == Streams)
        if (const int rc = combine_streams(c, ps, p)) return rc;
    c->timed = true;
    c->stats_spp = spp_add;
    c->stats_adaptive = adaptive_mode(ps.mode);
    return SRT_OK;
}

int read_planes(srt_ctx *c, int first_plane, float *p0, float *p1, float *p2) {
    if (!c || !c->d_fb) return fail(c, SRT_ERR_INVALID, "read: device parameters not initialised");
    if (const int rc = srt_synchronize(c)) return rc;
    float *dst[3] = {p0, p1, p2};
    for (int k = 0; k < 3; k++)
        if (dst[k]) HIP_TRY(c, hipMemcpy(dst[k], fb_plane(c, first_plane + k), (size_t)c->n_lanes * sizeof(float), hipMemcpyDeviceToHost));
    return SRT_OK;
}

// Three block-linear planes of n_lanes words (bits copied as they are) -> the last chunk's rectangle of three row-major host images.
// A null host plane is not copied (its source plane may be any valid one).
int read_rowmajor(srt_ctx *c, const float *const src[3], float *const host[3], uint32_t image_width, uint32_t image_height) {
    HIP_TRY(c, set_device(c));
    const size_t n = (size_t)image_width * image_height;
    // context-owned row-major staging image: the un-swizzle writes the chunk's pixels into it on the device and only the
    // chunk's rectangle travels to the caller's planes (update_fb touches nothing else either, render_manager.cuh:68-142)
    if (c->rowmajor_w != image_width || c->rowmajor_h != image_height || !c->d_rowmajor) {
        HIP_TRY(c, c->d_rowmajor.reserve(3 * n * sizeof(float)));
        HIP_TRY(c, hipMemset(c->d_rowmajor.ptr, 0, 3 * n * sizeof(float)));
        c->rowmajor_w = image_width; c->rowmajor_h = image_height;
    }
    float *dst[3] = {c->d_rowmajor.as<float>(), c->d_rowmajor.as<float>() + n, c->d_rowmajor.as<float>() + 2 * n};
    HIP_TRY(c, launch_unswizzle(src, dst, c->tx, c->ty, c->bx, c->by, c->last_w, c->last_h, c->last_offx, c->last_offy, image_width, image_height, nullptr));
    const ChunkRect rect = chunk_rect(c, image_width, image_height);
    const size_t pitch = (size_t)image_width * sizeof(float);
    for (int k = 0; k < 3 && rect.w && rect.h; k++)
        if (host[k]) HIP_TRY(c, hipMemcpy2D(host[k] + rect.first, pitch, dst[k] + rect.first, pitch, (size_t)rect.w * sizeof(float), rect.h, hipMemcpyDeviceToHost));
    HIP_TRY(c, device_synchronize(c));
    return SRT_OK;
}

}  // namespace

extern "C" {

int srt_create(int device, srt_ctx **out) {
    if (!out) return fail(nullptr, SRT_ERR_INVALID, "srt_create: null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, SRT_ERR_NO_DEVICE, std::string("srt_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") +
                                                    "); this library has no CPU fallback");
    if (device < 0 || device >= n) return fail(nullptr, SRT_ERR_NO_DEVICE, "srt_create: device index out of range");
    e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipSetDevice");
    srt_ctx *c = new srt_ctx();
    c->device = device;
    if (const char *ev = getenv("SRT_WAVES_PER_CU")) c->waves_per_cu = (uint32_t)std::max(0, atoi(ev));
    if (const char *ev = getenv("SRT_PROBE_SPP")) c->probe_spp = (uint32_t)std::max(0, atoi(ev));
    if (const char *ev = getenv("SRT_SCORE_SHADE")) c->score_shade = (uint32_t)std::max(1, atoi(ev));
    if (const char *ev = getenv("SRT_SCORE_FRINGE")) c->score_fringe = (uint32_t)std::max(1, atoi(ev));   // 0 would starve fringe lanes
    if (const char *tk = getenv("SRT_TEST_KNOBS")) if (atoi(tk) == 1) {
        if (const char *ev = getenv("SRT_DEBUG_LANE_LIMIT")) { c->debug_lane_limit = (uint32_t)std::max(0, atoi(ev)); c->knobs_from_env = true; }
        if (const char *ev = getenv("SRT_PRESENT_SCALAR")) c->present_scalar = atoi(ev) != 0;      // (no render kernel depends on it: not a plan knob)
        if (const char *ev = getenv("SRT_GATHER_SCALAR")) c->gather_scalar = atoi(ev) != 0;        // (likewise)
        if (const char *ev = getenv("SRT_WIDE_REFS")) { c->knobs.wide_refs = atoi(ev) != 0; c->knobs_from_env = true; }
        if (const char *ev = getenv("SRT_LDS_CACHE_MAX")) { c->knobs.lds_cache_max = std::max(0, atoi(ev)); c->knobs_from_env = true; }
    }
    if (const char *ev = getenv("SRT_SPLIT_LOAD")) c->split_load_pct = (uint32_t)std::max(0, atoi(ev));
    if (const char *ev = getenv("SRT_ORDER_MAX_PCT")) c->order_max_pct = std::min(400, std::max(-1, atoi(ev)));
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    }
    std::vector<float> rows(96 * 4);
    cmf_rows(rows.data());
    int rc = upload(c, c->d_cmf, rows);
    if (rc != SRT_OK) { delete c; return rc; }
    if ((e = c->d_counters.reserve((kCounters + 1) * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(c->d_counters.ptr, 0, (kCounters + 1) * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) {
        int r = hip_fail(nullptr, e, "srt_create");
        srt_destroy(c);
        return r;
    }
    *out = c;
    return SRT_OK;
}

void srt_destroy(srt_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    for (hipEvent_t e : c->denoise_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->develop_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->expose_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->present_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->gather_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->despeckle_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->temporal_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->temporal_var_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->refit_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->query_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->light_ev) if (e) (void)hipEventDestroy(e);
    delete c;      // (every DeviceBuffer, and the pinned staging block, frees itself, on the device selected above)
}

int srt_ctx_device(const srt_ctx *ctx) { return ctx ? ctx->device : -1; }
int srt_ctx_cu_count(const srt_ctx *ctx) { return ctx ? ctx->n_cu : -1; }

const char *srt_last_error(const srt_ctx *ctx) { return ctx ? ctx->err.c_str() : global_error(); }

int srt_upload_scene(srt_ctx *c, const srt_scene *s) {
    if (!c || !s) return fail(c, SRT_ERR_INVALID, "srt_upload_scene: null argument");
    c->accum.invalidate();
    c->temporal_frames = 0;      // (the temporal history shows another scene)
    c->sched_probe_queue = false; c->sched_compacted_queue = false;      // (the queues of the last launch belong to the old set-up)
    c->refit_tables_ok = false; c->refit_tables_on_device = false;      // (the refit's tables describe the old tree)
    HIP_TRY(c, set_device(c));
    FlatScene f;
    int rc = flatten_scene(*s, f);
    if (rc != SRT_OK) return fail(c, rc, global_error());
    if (render_lds_bytes(f.stack_depth, 1, 0, f.n_records, c->knobs) > 64 * 1024) return fail(c, SRT_ERR_BVH, "srt_upload_scene: BVH too deep for the LDS traversal stack");
    if ((rc = upload(c, c->d_nodes, f.nodes)) != SRT_OK) return rc;
    {
        // FRINGE records are 96 B.  Packed, every second one straddles two 128-byte cache lines; when the tree is too large for
        // LDS every visit is an L2 round trip and a record that lies in ONE line halves the lines a FRINGE visit pulls through the
        // CU's small L1: SRT_FRINGE_STRIDE=128 pads such trees' records to a 128-byte stride (measured -1.4 % on cfg 5's scene, kept as a knob).
        LaunchPlan plan;
        render_launch_plan(f.stack_depth, f.n_records, f.n_inner, c->knobs, plan);
        uint32_t stride = plan.all_cached ? 96u : kFringeStrideL2;
        if (const char *ev = getenv("SRT_FRINGE_STRIDE")) stride = (atoi(ev) == 128 && !plan.all_cached) ? 128u : 96u;
        if ((uint64_t)(f.n_records - f.n_inner + 1) * stride >= (1ull << 31)) stride = 96u;
        std::vector<float> padded;
        if (stride != 96u) {
            const size_t n_fr = f.fringe.size() / 24;
            padded.assign(n_fr * 32, 0.f);
            for (size_t k = 0; k < n_fr; k++) memcpy(&padded[32 * k], &f.fringe[24 * k], 24 * sizeof(float));
        }
        if ((rc = upload(c, c->d_fringe, stride == 96u ? f.fringe : padded)) != SRT_OK) return rc;
        c->fringe_stride = stride;
        c->image_bytes[SRT_IMAGE_FRINGE] = (stride == 96u ? f.fringe.size() : padded.size()) * sizeof(float);
        c->image_bytes[SRT_IMAGE_NODES_SW] = plan.all_cached ? 0 : f.nodes_sw.size() * sizeof(float);
        // (the pre-swizzled copy of the INNER records: only trees whose INNER visits read memory need it)
        c->d_nodes_sw.release();
        if (!plan.all_cached && (rc = upload(c, c->d_nodes_sw, f.nodes_sw)) != SRT_OK) return rc;
    }
    if ((rc = upload(c, c->d_tris, f.tris)) != SRT_OK) return rc;
    if ((rc = upload(c, c->d_mat_sd, f.mat_sd)) != SRT_OK) return rc;
    if ((rc = upload(c, c->d_mat_par, f.mat_par)) != SRT_OK) return rc;
    if ((rc = upload(c, c->d_shade, f.shade)) != SRT_OK) return rc;
    {
        std::vector<float> col(4 * s->mats.size(), 0.f);
        for (size_t m = 0; m < s->mats.size(); m++)
            for (int k = 0; k < 3; k++) col[4 * m + k] = s->mats[m].col[k];
        if ((rc = upload(c, c->d_mat_col, col)) != SRT_OK) return rc;
    }
    c->root_ref = f.root_ref; c->stack_depth = f.stack_depth; c->n_materials = (uint32_t)s->mats.size();
    c->n_inner = f.n_inner; c->n_records = f.n_records; c->n_tris = (uint32_t)s->raw.size();
    c->paired = tree_is_paired(*s);
    c->image_bytes[SRT_IMAGE_NODES] = f.nodes.size() * sizeof(float);
    c->image_bytes[SRT_IMAGE_TRIS] = f.tris.size() * sizeof(float);
    c->image_bytes[SRT_IMAGE_SHADE] = f.shade.size() * sizeof(float);
    build_refit_tables(c, f, *s);      // (host only: nothing is enqueued or allocated on the device for a caller who never refits)
    keep_light_sources(c, *s);         // (host only as well: the direct-light tables are made at their first use)
    if (c->track_motion) {      // V_cur = the scene's vertices, on the host until first use; V_hist = none
        c->track_verts.resize(9 * s->raw.size());
        for (size_t k = 0; k < s->raw.size(); k++) {
            memcpy(&c->track_verts[9 * k], s->raw[k].v0, 3 * sizeof(float));
            memcpy(&c->track_verts[9 * k + 3], s->raw[k].v1, 3 * sizeof(float));
            memcpy(&c->track_verts[9 * k + 6], s->raw[k].v2, 3 * sizeof(float));
        }
        c->verts = srt_ctx::Verts::Host; c->verts_hist = false; c->refits_pending = 0;
    }
    c->scene_ready = true;
    return SRT_OK;
}

// ---- BVH refit (srt_refit.hip; srt_c_api.h states it at srt_refit_vertices) ---------------------------------------------------------
namespace {

int develop_reserve(srt_ctx *c, const char *who, DeviceBuffer &d, size_t bytes);      // (below, with the stages' working blocks)

// the refit: the device copy of the tables is made now if this is the first refit since the upload, then one triangle kernel and one
// level launch per height, bottom up, on the NULL stream; d_verts holds 9 * n_tris validated floats on the device
// V_cur of a tracking context on the device (it waits on the host from an upload until its first use); the vertices are known
int track_verts_to_device(srt_ctx *c, const char *who) {
    if (c->verts != srt_ctx::Verts::Host) return SRT_OK;
    const size_t bytes = c->track_verts.size() * sizeof(float);
    if (const int rc = develop_reserve(c, who, c->d_verts_cur, bytes)) return rc;
    HIP_TRY_AS(c, who, hipMemcpy(c->d_verts_cur.ptr, c->track_verts.data(), bytes, hipMemcpyHostToDevice));
    c->track_verts.clear(); c->track_verts.shrink_to_fit();
    c->verts = srt_ctx::Verts::Device;
    return SRT_OK;
}

// (h_verts: the caller's host array when the vertices came through the host entry, else null; a tracking context copies V_cur from it)
int refit_run(srt_ctx *c, const char *who, const float *d_verts, const float *h_verts) {
    const size_t n_tris = c->n_tris, n_rec = (size_t)c->n_records;
    const bool keep_history = c->track_motion && c->verts != srt_ctx::Verts::Unknown && c->temporal_frames > 0;
    if (c->track_motion) {
        if (keep_history && !c->verts_hist) {      // V_hist = the old V_cur: the blocks change places
            if (const int rc = track_verts_to_device(c, who)) return rc;
            if (const int rc = develop_reserve(c, who, c->d_verts_hist, 9 * n_tris * sizeof(float))) return rc;
        }
        if (c->verts != srt_ctx::Verts::Device) if (const int rc = develop_reserve(c, who, c->d_verts_cur, 9 * n_tris * sizeof(float))) return rc;
    }
    if (const int rc = develop_reserve(c, who, c->d_refit_tab, RefitTables::bytes(n_tris, n_rec))) return rc;
    if (const int rc = develop_reserve(c, who, c->d_refit_scratch, RefitScratch::bytes(n_tris, n_rec))) return rc;
    for (hipEvent_t &e : c->refit_ev)
        if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    const RefitTables T(c->d_refit_tab, n_tris, n_rec);
    const RefitScratch S(c->d_refit_scratch, n_tris);
    if (!c->refit_tables_on_device) {
        HIP_TRY_AS(c, who, hipMemcpy(T.tri_tab, c->refit_tri_tab.data(), c->refit_tri_tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (n_rec) {
            HIP_TRY_AS(c, who, hipMemcpy(T.child, c->refit_child.data(), c->refit_child.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY_AS(c, who, hipMemcpy(T.sched, c->refit_sched.data(), c->refit_sched.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        c->refit_tables_on_device = true;
    }
    RefitParams p = {};
    p.verts = d_verts; p.tri_tab = T.tri_tab; p.child = T.child; p.sched = T.sched;
    p.tris = c->d_tris.as<float>(); p.shade = c->d_shade.as<float>(); p.fringe = c->d_fringe.as<float>(); p.nodes = c->d_nodes.as<float>();
    p.nodes_sw = c->image_bytes[SRT_IMAGE_NODES_SW] ? c->d_nodes_sw.as<float>() : nullptr;
    p.leaf_box = S.leaf_box; p.rec_box = S.rec_box;
    p.n_tris = c->n_tris; p.n_inner = (uint32_t)c->n_inner; p.fringe_stride = c->fringe_stride / (uint32_t)sizeof(float);
    // from here on the images change: what shows the old geometry goes, as at srt_upload_scene
    c->accum.invalidate();
    if (!keep_history) c->temporal_frames = 0;      // (a tracking context keeps it: the *_moving calls reproject across the refit)
    c->sched_probe_queue = false; c->sched_compacted_queue = false;
    c->refit_timed = false;
    c->light_refitted = true;      // (the light table's areas describe the uploaded vertices)
    if (c->track_motion) {
        if (keep_history && !c->verts_hist) { c->d_verts_cur.swap(c->d_verts_hist); c->verts_hist = true; }
        if (!keep_history) c->verts_hist = false;
        if (h_verts) HIP_TRY_AS(c, who, hipMemcpyAsync(c->d_verts_cur.ptr, h_verts, 9 * n_tris * sizeof(float), hipMemcpyHostToDevice, nullptr));
        else HIP_TRY_AS(c, who, hipMemcpyAsync(c->d_verts_cur.ptr, d_verts, 9 * n_tris * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        c->track_verts.clear();
        c->verts = srt_ctx::Verts::Device;
        c->refits_pending = keep_history ? c->refits_pending + 1u : 0u;
    }
    HIP_TRY_AS(c, who, hipEventRecord(c->refit_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_refit_triangles(p, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->refit_ev[1], nullptr));
    const uint32_t n_levels = c->refit_level_first.empty() ? 0u : (uint32_t)c->refit_level_first.size() - 1u;
    for (uint32_t h = 0; h < n_levels; h++)
        HIP_TRY_AS(c, who, launch_refit_level(p, c->refit_level_first[h], c->refit_level_first[h + 1] - c->refit_level_first[h], nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->refit_ev[2], nullptr));
    HIP_TRY_AS(c, who, device_synchronize(c));
    c->refit_timed = true; c->refit_timed_levels = n_levels;
    return SRT_OK;
}

const char *refit_refusal(const srt_ctx *c, const void *verts, size_t n_tris) {
    if (!c->scene_ready) return "no scene uploaded";
    if (!c->refit_tables_ok) return "the uploaded records do not form a tree the refit can schedule (internal error)";
    if (!verts) return "null vertices";
    if (n_tris != c->n_tris) return "n_tris is not the uploaded scene's triangle count";
    return nullptr;
}

}  // namespace

int srt_refit_vertices(srt_ctx *c, const float *verts, size_t n_tris) { return srt_internal_refit_vertices(c, verts, n_tris, 0); }

int srt_internal_refit_vertices(srt_ctx *c, const float *verts, size_t n_tris, int scanned) {
    const char *who = "srt_refit_vertices";
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_refit_vertices: null ctx");
    if (const char *why = refit_refusal(c, verts, n_tris)) return fail(c, SRT_ERR_INVALID, std::string("srt_refit_vertices: ") + why);
    for (size_t k = 0; !scanned && k < 9 * n_tris; k++)
        if (!std::isfinite(verts[k])) return fail(c, SRT_ERR_INVALID, "srt_refit_vertices: a coordinate is not finite");
    HIP_TRY(c, set_device(c));
    if (const int rc = develop_reserve(c, who, c->d_refit_verts, 9 * n_tris * sizeof(float))) return rc;
    HIP_TRY_AS(c, who, hipMemcpy(c->d_refit_verts.ptr, verts, 9 * n_tris * sizeof(float), hipMemcpyHostToDevice));
    return refit_run(c, who, c->d_refit_verts.as<float>(), verts);
}

int srt_refit_vertices_dev(srt_ctx *c, const float *verts_dev, size_t n_tris) {
    const char *who = "srt_refit_vertices_dev";
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_refit_vertices_dev: null ctx");
    if (const char *why = refit_refusal(c, verts_dev, n_tris)) return fail(c, SRT_ERR_INVALID, std::string("srt_refit_vertices_dev: ") + why);
    HIP_TRY(c, set_device(c));
    if (const int rc = develop_reserve(c, who, c->d_refit_scratch, RefitScratch::bytes(n_tris, (size_t)c->n_records))) return rc;
    // the validation: the count of coordinates that are not finite comes back, 4 bytes, before anything is written
    const RefitScratch S(c->d_refit_scratch, n_tris);
    uint32_t bad = 0;
    HIP_TRY_AS(c, who, hipMemsetAsync(S.count, 0, sizeof(uint32_t), nullptr));
    HIP_TRY_AS(c, who, launch_refit_validate(verts_dev, 9 * n_tris, S.count, nullptr));
    HIP_TRY_AS(c, who, hipMemcpy(&bad, S.count, sizeof(bad), hipMemcpyDeviceToHost));
    if (bad) {
        HIP_TRY_AS(c, who, device_synchronize(c));
        return fail(c, SRT_ERR_INVALID, "srt_refit_vertices_dev: a coordinate is not finite");
    }
    return refit_run(c, who, verts_dev, nullptr);
}

int srt_refit_last_ms(srt_ctx *c, float *tri_ms, float *levels_ms, uint32_t *n_levels) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_refit_last_ms: null ctx");
    if (!c->refit_timed) return fail(c, SRT_ERR_INVALID, "srt_refit_last_ms: no refit has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->refit_ev[2]));
    if (tri_ms) HIP_TRY(c, hipEventElapsedTime(tri_ms, c->refit_ev[0], c->refit_ev[1]));
    if (levels_ms) HIP_TRY(c, hipEventElapsedTime(levels_ms, c->refit_ev[1], c->refit_ev[2]));
    if (n_levels) *n_levels = c->refit_timed_levels;
    return SRT_OK;
}

int srt_read_scene_image(srt_ctx *c, int which, void *out, size_t cap_bytes, size_t *n_bytes) {
    if (!c || !n_bytes) return fail(c, SRT_ERR_INVALID, "srt_read_scene_image: null argument");
    if (!c->scene_ready) return fail(c, SRT_ERR_INVALID, "srt_read_scene_image: no scene uploaded");
    const DeviceBuffer *src = nullptr;
    switch (which) {
    case SRT_IMAGE_NODES: src = &c->d_nodes; break;
    case SRT_IMAGE_NODES_SW: src = &c->d_nodes_sw; break;
    case SRT_IMAGE_FRINGE: src = &c->d_fringe; break;
    case SRT_IMAGE_TRIS: src = &c->d_tris; break;
    case SRT_IMAGE_SHADE: src = &c->d_shade; break;
    default: return fail(c, SRT_ERR_INVALID, "srt_read_scene_image: unknown image");
    }
    const size_t n = c->image_bytes[which];
    if (out && cap_bytes < n) return fail(c, SRT_ERR_INVALID, "srt_read_scene_image: the image does not fit cap_bytes");
    HIP_TRY(c, set_device(c));
    HIP_TRY(c, device_synchronize(c));
    if (out && n) HIP_TRY(c, hipMemcpy(out, src->ptr, n, hipMemcpyDeviceToHost));
    *n_bytes = n;
    return SRT_OK;
}

int srt_set_camera(srt_ctx *c, const srt_camera_data *cam) {
    if (!c || !cam) return fail(c, SRT_ERR_INVALID, "srt_set_camera: null argument");
    c->accum.invalidate();
    c->cam = *cam;
    c->camera_ready = true;
    return SRT_OK;
}

int srt_launch_plan(const srt_ctx *c, int *waves_per_cu, int *n_cached, int *all_cached, int *narrow_refs) {
    if (!c || !c->scene_ready) return fail(nullptr, SRT_ERR_INVALID, "srt_launch_plan: no scene uploaded");
    const LaunchPlan plan = plan_of(c);
    if (waves_per_cu) *waves_per_cu = plan.waves_per_cu;
    if (n_cached) *n_cached = plan.n_cached;
    if (all_cached) *all_cached = plan.all_cached ? 1 : 0;
    if (narrow_refs) *narrow_refs = render_narrow_refs(c->n_records, c->knobs) ? 1 : 0;
    return SRT_OK;
}

int srt_launch_paired(const srt_ctx *c, int *paired) {
    if (!c || !c->scene_ready || !paired) return fail(nullptr, SRT_ERR_INVALID, "srt_launch_paired: no scene uploaded / null argument");
    const LaunchPlan plan = plan_of(c);
    *paired = render_paired_variant(c->paired, render_narrow_refs(c->n_records, c->knobs), plan.all_cached) ? 1 : 0;
    return SRT_OK;
}

int srt_launch_lds_bytes(const srt_ctx *c, size_t *bytes) {
    if (!c || !c->scene_ready || !bytes) return fail(nullptr, SRT_ERR_INVALID, "srt_launch_lds_bytes: no scene uploaded / null argument");
    const LaunchPlan plan = plan_of(c);
    *bytes = render_lds_bytes(c->stack_depth, plan.waves_per_block, plan.n_cached, c->n_records, c->knobs);
    return SRT_OK;
}

// Test knobs of a context: wide_refs != 0 sends small trees through the 32-bit-reference kernel variants, lds_cache_max >= 0 caps the
// inner records kept in LDS (0 = every inner record from L2), lane_limit > 0 renders only the first lane_limit pixels of every tile.
// -1 / 0 / 0 restores the defaults.  A scene uploaded before the call must be uploaded again (the FRINGE stride follows the plan).
int srt_set_test_knobs(srt_ctx *c, int wide_refs, int lds_cache_max, uint32_t lane_limit) {
    if (!c || lds_cache_max < -1 || lane_limit > 64) return fail(c, SRT_ERR_INVALID, "srt_set_test_knobs: bad argument");
    c->knobs.wide_refs = wide_refs != 0; c->knobs.lds_cache_max = lds_cache_max; c->debug_lane_limit = lane_limit;
    c->scene_ready = false;      // the upload's FRINGE stride and the plan must be made with the same knobs
    return SRT_OK;
}
int srt_get_test_knobs(const srt_ctx *c, int *wide_refs, int *lds_cache_max, uint32_t *lane_limit, int *from_env) {
    if (!c) return fail(nullptr, SRT_ERR_INVALID, "srt_get_test_knobs: null ctx");
    if (wide_refs) *wide_refs = c->knobs.wide_refs ? 1 : 0;
    if (lds_cache_max) *lds_cache_max = c->knobs.lds_cache_max;
    if (lane_limit) *lane_limit = c->debug_lane_limit;
    if (from_env) *from_env = c->knobs_from_env ? 1 : 0;
    return SRT_OK;
}

// srt_init_device_params without the final device-wide wait: a communicator that drives several GPUs from one process enqueues
// the re-seeding on all of them before it waits for any (srt_comm_init_device_params)
int srt_internal_init_device_params(srt_ctx *c, uint32_t tx, uint32_t ty, uint32_t bx, uint32_t by, uint32_t chunk_w, uint32_t chunk_h,
                                    uint32_t spp, uint32_t bounce_limit, uint64_t seed, int wait) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_init_device_params: null ctx");
    if (tx == 0 || ty == 0 || bx == 0 || by == 0 || chunk_w == 0 || chunk_h == 0)
        return fail(c, SRT_ERR_INVALID, "srt_init_device_params: zero dimension");
    c->accum.invalidate();
    c->temporal_frames = 0;      // (the temporal history belongs to the old grid)
    c->verts_hist = false; c->refits_pending = 0;
    c->sched_probe_queue = false; c->sched_compacted_queue = false;      // (the queues of the last launch belong to the old set-up)
    const uint64_t lanes = (uint64_t)tx * ty * bx * by;
    if (lanes > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, "srt_init_device_params: grid too large");
    HIP_TRY(c, set_device(c));
    c->tx = tx; c->ty = ty; c->bx = bx; c->by = by; c->chunk_w = chunk_w; c->chunk_h = chunk_h;
    c->spp = (uint16_t)spp; c->bounce = (uint16_t)bounce_limit;     // short_uint, rendering.cu:154 (Q17)
    c->seed = seed; c->n_lanes = (uint32_t)lanes;
    c->streams_seeded = 0;      // streams 1 .. K-1 start from this seed again at the next srt_accum_reset_streams
    // (a new frame of the same grid -- or of a smaller one -- re-seeds in place)
    HIP_TRY(c, c->d_rng.reserve(6 * lanes * sizeof(uint32_t)));
    HIP_TRY(c, c->d_fb.reserve(kTilePlanes * lanes * sizeof(float)));
    HIP_TRY(c, hipMemset(c->d_fb.ptr, 0, kTilePlanes * lanes * sizeof(float)));
    HIP_TRY(c, launch_init_rng(c->d_rng.as<uint32_t>(), c->n_lanes, seed, nullptr));   // init_random_states, rendering.cu:330
    if (wait) HIP_TRY(c, device_synchronize(c));
    c->fb_groups_valid = (uint32_t)kTileGroups;      // all nine planes are zero
    c->params_ready = true;
    return SRT_OK;
}

int srt_init_device_params(srt_ctx *c, uint32_t tx, uint32_t ty, uint32_t bx, uint32_t by, uint32_t chunk_w, uint32_t chunk_h,
                           uint32_t spp, uint32_t bounce_limit, uint64_t seed) {
    return srt_internal_init_device_params(c, tx, ty, bx, by, chunk_w, chunk_h, spp, bounce_limit, seed, 1);
}

int srt_set_partition(srt_ctx *c, uint32_t rank, uint32_t world) {
    if (!c || world == 0 || rank >= world) return fail(c, SRT_ERR_INVALID, "srt_set_partition: need rank < world");
    c->accum.invalidate();
    c->temporal_frames = 0;      // (the temporal history belongs to the old partition)
    c->verts_hist = false; c->refits_pending = 0;
    c->sched_probe_queue = false; c->sched_compacted_queue = false;      // (the queues of the last launch belong to the old set-up)
    c->rank = rank; c->world = world;
    return SRT_OK;
}

uint32_t srt_internal_gather_planes(const srt_ctx *c) { return c ? c->gather_planes : 0u; }

int srt_set_gather_planes(srt_ctx *c, uint32_t planes) {
    if (!c || (planes != 3 && planes != 9)) return fail(c, SRT_ERR_INVALID, "srt_set_gather_planes: planes must be 3 or 9");
    // (an adaptive pass writes only the slots of its active pixels: the converged ones would keep planes of another set)
    if (c->accum.adaptive()) c->accum.invalidate();
    c->gather_planes = planes;
    return SRT_OK;
}

int srt_render_chunk(srt_ctx *c, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy, void *stream) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_render_chunk: null ctx");
    // reference: "Device parameters were not initialized, render aborted" (rendering.cu:247-250)
    if (!c->scene_ready || !c->camera_ready || !c->params_ready)
        return fail(c, SRT_ERR_INVALID, "srt_render_chunk: scene, camera and device parameters must be set first");
    c->accum.invalidate();      // its launch moves the RNG streams (and may rewrite the pixel queue) behind the sums
    HIP_TRY(c, set_device(c, (hipStream_t)stream));
    width = (uint16_t)width; height = (uint16_t)height; offx = (uint16_t)offx; offy = (uint16_t)offy;   // rendering.cu:245 (Q17)
    return render_chunk_impl(c, width, height, offx, offy, 0u, (hipStream_t)stream);
}

int srt_accum_reset(srt_ctx *c) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_accum_reset: null ctx");
    if (!c->params_ready) return fail(c, SRT_ERR_INVALID, "srt_accum_reset: device parameters must be set first (srt_init_device_params)");
    HIP_TRY(c, set_device(c));
    c->accum.invalidate();
    HIP_TRY(c, c->d_accum.reserve(AccumLayout::bytes(c->n_lanes)));
    // (null stream, then a wait: a pass on any stream of the caller's finds the sums zeroed)
    HIP_TRY(c, hipMemset(AccumLayout(c).sums, 0, AccumLayout::sums_bytes(c->n_lanes)));
    HIP_TRY(c, device_synchronize(c));
    c->accum.total = 0;
    c->accum.begin(srt_ctx::Accumulation::Kind::Plain);
    return SRT_OK;
}

int srt_accum_reset_spectral(srt_ctx *c) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_spectral: null ctx");
    // refusals first: a refused call leaves the context's accumulation as it was
    if (c->count_traversal)
        return fail(c, SRT_ERR_UNSUPPORTED, "srt_accum_reset_spectral: no instrumented accumulating kernel (srt_set_count_traversal(ctx, 0) first)");
    if (!c->params_ready) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_spectral: device parameters must be set first (srt_init_device_params)");
    HIP_TRY(c, set_device(c));
    const size_t film_bytes = (size_t)c->n_lanes * kFilmStride * sizeof(float);
    if (c->d_film.bytes < film_bytes) {
        // (the new film is allocated before the old one goes: a failed allocation changes nothing)
        DeviceBuffer film;
        HIP_TRY(c, film.reserve(film_bytes));
        c->d_film = std::move(film);
    }
    int rc = srt_accum_reset(c);
    if (rc != SRT_OK) return rc;
    c->accum.invalidate();      // (until the film is in place)
    HIP_TRY(c, hipMemset(c->d_film.ptr, 0, film_bytes));
    // the film's slot of the header (the per-pass kernel rewrites only sums and spp_total)
    float *film = c->d_film.as<float>();
    HIP_TRY(c, hipMemcpy(&AccumLayout(c).header->film, &film, sizeof(film), hipMemcpyHostToDevice));
    HIP_TRY(c, device_synchronize(c));
    c->accum.begin(srt_ctx::Accumulation::Kind::Spectral);
    return SRT_OK;
}

int srt_accum_reset_features(srt_ctx *c) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_features: null ctx");
    // refusals first: a refused call leaves the context's accumulation as it was
    if (c->count_traversal)
        return fail(c, SRT_ERR_UNSUPPORTED, "srt_accum_reset_features: no instrumented accumulating kernel (srt_set_count_traversal(ctx, 0) first)");
    if (!c->params_ready) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_features: device parameters must be set first (srt_init_device_params)");
    HIP_TRY(c, set_device(c));
    const size_t bytes = (size_t)c->n_lanes * kFeatureStride * sizeof(float);
    if (c->d_features.bytes < bytes) {
        // (the new rows are allocated before the old ones go: a failed allocation changes nothing)
        DeviceBuffer rows;
        HIP_TRY(c, rows.reserve(bytes));
        c->d_features = std::move(rows);
    }
    int rc = srt_accum_reset(c);
    if (rc != SRT_OK) return rc;
    c->accum.invalidate();      // (until the rows are in place)
    HIP_TRY(c, hipMemset(c->d_features.ptr, 0, bytes));
    // the featured part of the header (the per-pass kernel rewrites only sums and spp_total)
    AccumHeader h = {};
    h.features = c->d_features.as<float>(); h.mat_col = c->d_mat_col.as<const float>();
    const size_t tail = offsetof(AccumHeader, features);
    HIP_TRY(c, hipMemcpy(&AccumLayout(c).header->features, reinterpret_cast<const char *>(&h) + tail, sizeof(h) - tail, hipMemcpyHostToDevice));
    HIP_TRY(c, device_synchronize(c));
    c->accum.begin(srt_ctx::Accumulation::Kind::Features);
    return SRT_OK;
}

int srt_accum_reset_spectral_features(srt_ctx *c) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_spectral_features: null ctx");
    // refusals first: a refused call leaves the context's accumulation as it was
    if (c->count_traversal)
        return fail(c, SRT_ERR_UNSUPPORTED, "srt_accum_reset_spectral_features: no instrumented accumulating kernel (srt_set_count_traversal(ctx, 0) first)");
    if (!c->params_ready) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_spectral_features: device parameters must be set first (srt_init_device_params)");
    HIP_TRY(c, set_device(c));
    // srt_accum_reset_spectral's rule for the film and srt_accum_reset_features' rule for the rows.  Both new blocks are allocated before
    // either old one goes: a failed allocation changes nothing, and leaves no error behind for the next launch's hipGetLastError
    const char *who = "srt_accum_reset_spectral_features";
    const size_t film_bytes = (size_t)c->n_lanes * kFilmStride * sizeof(float), row_bytes = (size_t)c->n_lanes * kFeatureStride * sizeof(float);
    DeviceBuffer film, rows;
    if (c->d_film.bytes < film_bytes)
        if (const hipError_t e = film.reserve(film_bytes)) { (void)hipGetLastError(); return hip_fail(c, e, who); }
    if (c->d_features.bytes < row_bytes)
        if (const hipError_t e = rows.reserve(row_bytes)) { (void)hipGetLastError(); return hip_fail(c, e, who); }
    if (film) c->d_film = std::move(film);
    if (rows) c->d_features = std::move(rows);
    int rc = srt_accum_reset(c);
    if (rc != SRT_OK) return rc;
    c->accum.invalidate();      // (until film and rows are in place)
    HIP_TRY(c, hipMemset(c->d_film.ptr, 0, film_bytes));
    HIP_TRY(c, hipMemset(c->d_features.ptr, 0, row_bytes));
    // the film's slot of the header and the featured part behind it (the per-pass kernel rewrites only sums and spp_total)
    float *film_ptr = c->d_film.as<float>();
    HIP_TRY(c, hipMemcpy(&AccumLayout(c).header->film, &film_ptr, sizeof(film_ptr), hipMemcpyHostToDevice));
    AccumHeader h = {};
    h.features = c->d_features.as<float>(); h.mat_col = c->d_mat_col.as<const float>();
    const size_t tail = offsetof(AccumHeader, features);
    HIP_TRY(c, hipMemcpy(&AccumLayout(c).header->features, reinterpret_cast<const char *>(&h) + tail, sizeof(h) - tail, hipMemcpyHostToDevice));
    HIP_TRY(c, device_synchronize(c));
    c->accum.begin(srt_ctx::Accumulation::Kind::SpectralFeatures);
    return SRT_OK;
}

int srt_accum_reset_streams(srt_ctx *c, uint32_t streams) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_streams: null ctx");
    // refusals first: a refused call leaves the context's accumulation as it was
    if (streams == 0 || streams > kMaxStreams) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_streams: streams must be in 1 .. SRT_MAX_STREAMS (16)");
    if (c->count_traversal)
        return fail(c, SRT_ERR_UNSUPPORTED, "srt_accum_reset_streams: no instrumented accumulating kernel (srt_set_count_traversal(ctx, 0) first)");
    if (!c->params_ready) return fail(c, SRT_ERR_INVALID, "srt_accum_reset_streams: device parameters must be set first (srt_init_device_params)");
    if ((uint64_t)streams * c->n_lanes > 0x7fffffffull)
        return fail(c, SRT_ERR_INVALID, "srt_accum_reset_streams: streams x lanes of the grid must stay below 2^31 (the stream planes have 32-bit indices)");
    HIP_TRY(c, set_device(c));
    const size_t bytes = StreamPlanes::bytes(c->n_lanes, streams);
    const bool seeded = c->streams_seeded == streams && c->d_streams.bytes >= bytes;
    if (c->d_streams.bytes < bytes) {
        // (the new planes are allocated before the old ones go: a failed allocation changes nothing)
        DeviceBuffer planes;
        HIP_TRY(c, planes.reserve(bytes));
        c->d_streams = std::move(planes);
        c->streams_seeded = 0;
    }
    int rc = srt_accum_reset(c);
    if (rc != SRT_OK) return rc;
    c->accum.invalidate();      // (until the stream planes are in place)
    const StreamPlanes sp(c->d_streams, c->n_lanes, streams);
    // streams 1 .. K-1 of lane idx: XORWOW(seed + k * n_lanes + idx), the state that lane has in a context initialised with seed + k * n_lanes.
    // Once per srt_init_device_params and K: like stream 0, they continue across resets.  (The planes of another K are laid out
    // differently: a reset with another K seeds them afresh.)
    if (!seeded) {
        c->streams_seeded = 0;
        HIP_TRY(c, launch_init_rng(sp.rng, streams * c->n_lanes, c->seed, nullptr));
    }
    HIP_TRY(c, hipMemset(sp.sums, 0, StreamPlanes::sums_bytes(c->n_lanes, streams)));
    // the streamed part of the header (the per-pass kernel rewrites only sums and spp_total)
    AccumHeader h = {};
    h.stream_planes = sp.rng; h.streams = streams;
    const size_t tail = offsetof(AccumHeader, stream_planes);
    HIP_TRY(c, hipMemcpy(&AccumLayout(c).header->stream_planes, reinterpret_cast<const char *>(&h) + tail, sizeof(h) - tail, hipMemcpyHostToDevice));
    HIP_TRY(c, device_synchronize(c));
    c->streams_seeded = streams;
    c->accum.begin(srt_ctx::Accumulation::Kind::Streams, streams);
    return SRT_OK;
}

int srt_accum_streams(const srt_ctx *c, uint32_t *streams) {
    if (!c || !streams) return fail(nullptr, SRT_ERR_INVALID, "srt_accum_streams: null argument");
    *streams = c->accum.valid() && c->accum.streamed() ? c->accum.n_streams : 0u;
    return SRT_OK;
}

// srt_accum_reset_adaptive, srt_accum_reset_adaptive_features (`features`), srt_accum_reset_adaptive_spectral (`spectral`) and
// srt_accum_reset_adaptive_spectral_features (both): one body, so that validation, refusals and invalidation of the others are those of the
// first by construction; the featured one adds srt_accum_reset_features' allocation rule and rows, the spectral ones
// srt_accum_reset_spectral's rule and film.  With both, the rows lie behind the film in d_film (feature_rows): MODE 11 finds them there.
static int accum_reset_adaptive(srt_ctx *c, const srt_adaptive *cfg, bool features, bool spectral, const char *who) {
    const std::string w_(who);
    if (!c) return fail(c, SRT_ERR_INVALID, w_ + ": null ctx");
    // refusals first: a refused call leaves the context's accumulation as it was
    if (!cfg) return fail(c, SRT_ERR_INVALID, w_ + ": null cfg");
    if (!std::isfinite(cfg->rel_tol) || !std::isfinite(cfg->abs_tol) || cfg->rel_tol < 0.f || cfg->abs_tol < 0.f || !(cfg->rel_tol + cfg->abs_tol > 0.f))
        return fail(c, SRT_ERR_INVALID, w_ + ": rel_tol and abs_tol must be finite and >= 0, and not both 0");
    if (cfg->min_spp < 2) return fail(c, SRT_ERR_INVALID, w_ + ": min_spp must be >= 2 (the variance of the mean needs two samples)");
    if (cfg->reserved != 0) return fail(c, SRT_ERR_INVALID, w_ + ": reserved must be 0");
    if (c->count_traversal)
        return fail(c, SRT_ERR_UNSUPPORTED, w_ + ": no instrumented accumulating kernel (srt_set_count_traversal(ctx, 0) first)");
    if (!c->params_ready) return fail(c, SRT_ERR_INVALID, w_ + ": device parameters must be set first (srt_init_device_params)");
    const size_t row_bytes = (size_t)c->n_lanes * kFeatureStride * sizeof(float), film_bytes = (size_t)c->n_lanes * kFilmStride * sizeof(float);
    if (spectral) {
        // (film, and rows behind it: one block, allocated before the old one goes -- a failed allocation changes nothing, and leaves no
        // error behind for the next launch's hipGetLastError)
        const size_t bytes = film_bytes + (features ? row_bytes : 0);
        if (c->d_film.bytes < bytes) {
            HIP_TRY(c, hipSetDevice(c->device));
            DeviceBuffer film;
            if (const hipError_t e = film.reserve(bytes)) { (void)hipGetLastError(); return hip_fail(c, e, who); }
            c->d_film = std::move(film);
        }
    } else if (features && c->d_features.bytes < row_bytes) {
        // (the new rows are allocated before the old ones go: a failed allocation changes nothing)
        HIP_TRY(c, hipSetDevice(c->device));
        DeviceBuffer rows;
        HIP_TRY(c, rows.reserve(row_bytes));
        c->d_features = std::move(rows);
    }
    int rc = srt_accum_reset(c);
    if (rc != SRT_OK) return rc;
    c->accum.invalidate();      // (until the adaptive planes are in place)
    HIP_TRY(c, c->d_adapt.reserve(AdaptPlanes::bytes(c->n_lanes)));
    HIP_TRY(c, hipMemset(c->d_adapt.ptr, 0, AdaptPlanes::bytes(c->n_lanes)));
    float *const rows = !features ? nullptr : spectral ? c->d_film.as<float>() + (size_t)c->n_lanes * kFilmStride : c->d_features.as<float>();
    if (spectral) HIP_TRY(c, hipMemset(c->d_film.ptr, 0, film_bytes));
    if (features) HIP_TRY(c, hipMemset(rows, 0, row_bytes));
    // the adaptive half of the header, and the film and the featured part behind it (the per-pass kernel rewrites only sums and spp_total)
    AccumHeader h = {};
    h.sum2 = AdaptPlanes(c).sum2; h.state = AdaptPlanes(c).state;
    h.rel_tol = cfg->rel_tol; h.abs_tol = cfg->abs_tol; h.min_spp = cfg->min_spp;
    if (spectral) h.film = c->d_film.as<float>();
    if (features) { h.features = rows; h.mat_col = c->d_mat_col.as<const float>(); }
    const size_t tail = offsetof(AccumHeader, sum2);
    HIP_TRY(c, hipMemcpy(&AccumLayout(c).header->sum2, reinterpret_cast<const char *>(&h) + tail, sizeof(h) - tail, hipMemcpyHostToDevice));
    HIP_TRY(c, device_synchronize(c));
    using Kind = srt_ctx::Accumulation::Kind;
    c->accum.begin(spectral ? (features ? Kind::AdaptiveSpectralFeatures : Kind::AdaptiveSpectral) : features ? Kind::AdaptiveFeatures : Kind::Adaptive);
    return SRT_OK;
}

// the feature rows of the context's featured accumulation: d_features, except that an adaptive spectral featured accumulation keeps them
// behind its film (accum_reset_adaptive)
static float *feature_rows(const srt_ctx *c) {
    return c->accum.kind == srt_ctx::Accumulation::Kind::AdaptiveSpectralFeatures ? c->d_film.as<float>() + (size_t)c->n_lanes * kFilmStride : c->d_features.as<float>();
}

// ---- a gathered accumulation (srt_gather.hip; srt_c_api.h at srt_pack_accum) ---------------------------------------------------------
// the parts the accumulation's kind holds
static uint32_t gather_parts_held(const srt_ctx *c) {
    return SRT_GATHER_SUMS | (c->accum.adaptive() ? SRT_GATHER_COUNTS : 0u) | (c->accum.featured() ? SRT_GATHER_FEATURES : 0u) | (c->accum.spectral() ? SRT_GATHER_FILM : 0u);
}
// Is the context whole for a stage that reads the sums (and the counts of an adaptive accumulation), the rows when `features`, the film
// when `film`?  Partition (0, 1), or the last unpack since the last pass brought all of that.
static bool whole_for(const srt_ctx *c, bool features, bool film) {
    if (c->rank == 0 && c->world == 1) return true;
    const uint32_t need = (gather_parts_held(c) & (SRT_GATHER_SUMS | SRT_GATHER_COUNTS)) | (features ? SRT_GATHER_FEATURES : 0u) | (film ? SRT_GATHER_FILM : 0u);
    return c->accum.bound() && (c->accum.gathered & need) == need;
}
static const char *const kNotWhole = "needs the whole chunk on this context (partition (0, 1)): pixels of other ranks read +0 (or srt_comm_gather_accum first)";
// whose pixels the per-rank counters of the meter, tone and present kernels count: this rank's, or everybody's on a whole context
static uint32_t counted_rank(const srt_ctx *c) { return whole_for(c, false, false) ? 0u : c->rank; }
static uint32_t counted_world(const srt_ctx *c) { return whole_for(c, false, false) ? 1u : c->world; }

int srt_accum_reset_adaptive(srt_ctx *c, const srt_adaptive *cfg) { return accum_reset_adaptive(c, cfg, false, false, "srt_accum_reset_adaptive"); }

int srt_accum_reset_adaptive_features(srt_ctx *c, const srt_adaptive *cfg) { return accum_reset_adaptive(c, cfg, true, false, "srt_accum_reset_adaptive_features"); }

int srt_accum_reset_adaptive_spectral(srt_ctx *c, const srt_adaptive *cfg) { return accum_reset_adaptive(c, cfg, false, true, "srt_accum_reset_adaptive_spectral"); }

int srt_accum_reset_adaptive_spectral_features(srt_ctx *c, const srt_adaptive *cfg) {
    return accum_reset_adaptive(c, cfg, true, true, "srt_accum_reset_adaptive_spectral_features");
}

int srt_accum_active(srt_ctx *c, uint64_t *active) {
    if (!c || !active) return fail(c, SRT_ERR_INVALID, "srt_accum_active: null argument");
    if (!c->accum.adaptive() || !c->accum.valid())
        return fail(c, SRT_ERR_INVALID, "srt_accum_active: no adaptive accumulation (srt_accum_reset_adaptive first)");
    *active = 0;
    if (!c->accum.bound()) return SRT_OK;      // (the first pass binds the chunk)
    if (const int rc = srt_synchronize(c)) return rc;
    return read_adapt_counts(c, nullptr, active);
}

int srt_accum_samples(const srt_ctx *c, uint32_t *spp_total) {
    if (!c || !spp_total) return fail(nullptr, SRT_ERR_INVALID, "srt_accum_samples: null argument");
    *spp_total = c->accum.valid() ? c->accum.total : 0u;
    return SRT_OK;
}

int srt_render_chunk_accum(srt_ctx *c, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy, uint32_t spp_add, void *stream) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: null ctx");
    // every refusal comes before anything is enqueued: a refused pass leaves sums, RNG state and framebuffer as they were
    if (!c->scene_ready || !c->camera_ready || !c->params_ready)
        return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: scene, camera and device parameters must be set first");
    if (c->count_traversal)
        return fail(c, SRT_ERR_UNSUPPORTED, "srt_render_chunk_accum: no instrumented accumulating kernel (srt_set_count_traversal(ctx, 0) first)");
    if (!c->accum.valid())
        return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: no accumulation (srt_accum_reset first; scene, camera, device parameters, partition "
                                        "and a plain srt_render_chunk invalidate it)");
    if (spp_add == 0) return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: spp_add must be > 0");
    if ((uint64_t)c->accum.total + spp_add > 0xffffu)
        return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: the total would exceed 65535 samples per pixel (16-bit spp, Q17)");
    if (c->accum.streamed()) {
        const uint32_t k = c->accum.n_streams;
        if (spp_add % k != 0)
            return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: spp_add must be a multiple of the accumulation's streams (every stream draws spp_add / K samples)");
        tile_geometry(c);
        if ((uint64_t)c->tiles_local * k * 64 >= kQueueSlots)
            return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: tiles x streams x 64 must stay below 2^32 (the pixel queue's 32-bit slot counter)");
    }
    width = (uint16_t)width; height = (uint16_t)height; offx = (uint16_t)offx; offy = (uint16_t)offy;   // rendering.cu:245 (Q17)
    if (c->accum.bound() && (width != c->accum.w || height != c->accum.h || offx != c->accum.offx || offy != c->accum.offy))
        return fail(c, SRT_ERR_INVALID, "srt_render_chunk_accum: the accumulation belongs to another chunk (one accumulation per context)");
    HIP_TRY(c, set_device(c, (hipStream_t)stream));
    hipStream_t st = (hipStream_t)stream;
    c->accum.gathered = 0;      // (the pass moves this rank's records on: what an unpack brought of the others is stale from here)
    // (the header travels by value in the arguments of a one-lane kernel on the pass's stream: stream-ordered, no host buffer to keep alive)
    HIP_TRY(c, launch_accum_header(AccumLayout(c).header, AccumLayout(c).sums, c->accum.total + spp_add, st));
    const int rc = render_chunk_impl(c, width, height, offx, offy, spp_add, st);
    if (rc != SRT_OK) { c->accum.invalidate(); return rc; }      // (a launch that failed half-way leaves the sums undefined)
    c->accum.total += spp_add;
    c->accum.w = width; c->accum.h = height; c->accum.offx = offx; c->accum.offy = offy;
    c->accum.state = srt_ctx::Accumulation::State::Bound;
    return SRT_OK;
}

int srt_synchronize(srt_ctx *c) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_synchronize: null ctx");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, device_synchronize(c));
    return SRT_OK;
}

int srt_tile_buffer(srt_ctx *c, void **dev_ptr, size_t *n_floats, uint32_t *tiles_local, uint32_t *tiles_padded) {
    if (!c || !c->d_tiles) return fail(c, SRT_ERR_INVALID, "srt_tile_buffer: nothing rendered yet");
    if (dev_ptr) *dev_ptr = c->d_tiles.ptr;
    if (n_floats) *n_floats = (size_t)c->tiles_padded * c->gather_planes * kTileLanes;      // the exchange unit: the first 1 or 3 plane groups
    if (tiles_local) *tiles_local = c->tiles_local;
    if (tiles_padded) *tiles_padded = c->tiles_padded;
    return SRT_OK;
}

int srt_copy_tile_buffer(srt_ctx *c, void *dst_dev, void *stream) {
    if (!c || !c->d_tiles || !dst_dev) return fail(c, SRT_ERR_INVALID, "srt_copy_tile_buffer: nothing rendered yet / null destination");
    HIP_TRY(c, set_device(c, (hipStream_t)stream));
    HIP_TRY(c, hipMemcpyAsync(dst_dev, c->d_tiles.ptr, (size_t)c->tiles_padded * c->gather_planes * kTileLanes * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SRT_OK;
}

int srt_scatter_tiles(srt_ctx *c, const void *dev_gathered, void *stream) {
    if (!c || !c->d_fb || !c->d_tiles) return fail(c, SRT_ERR_INVALID, "srt_scatter_tiles: nothing rendered yet");
    uint32_t groups = c->gather_planes / (uint32_t)kGroupPlanes;
    if (!dev_gathered) {
        if (c->world != 1) return fail(c, SRT_ERR_INVALID, "srt_scatter_tiles: a gathered buffer is required when world > 1");
        dev_gathered = c->d_tiles.ptr;      // the context's own tile buffer: group 0, and the parity groups when they were asked for
    }
    HIP_TRY(c, set_device(c, (hipStream_t)stream));
    ScatterParams sp = {};
    sp.gathered = (const float *)dev_gathered;
    sp.groups = groups;
    for (int p = 0; p < kTilePlanes; p++) sp.fb[p] = fb_plane(c, p);
    sp.width = c->last_w; sp.height = c->last_h;
    sp.tx = c->tx; sp.ty = c->ty; sp.bx = c->bx; sp.by = c->by;
    sp.tiles_x = c->tiles_x; sp.n_tiles = c->n_tiles; sp.world = c->world; sp.tiles_padded = c->tiles_padded;
    HIP_TRY(c, launch_scatter(sp, (hipStream_t)stream));
    c->fb_groups_valid = groups;      // with a 3-plane exchange unit the parity planes of d_fb are NOT those of this frame
    return SRT_OK;
}

// What a pack / unpack of `parts` needs of the context: the refusal (null: none) and, in *resolved, the parts that travel.  Host only.
static const char *gather_refusal(const srt_ctx *c, uint32_t parts, uint32_t *resolved, int *code) {
    *code = SRT_ERR_INVALID;
    if (!c->accum.bound()) return "no accumulation with a pass (srt_accum_reset* and srt_render_chunk_accum first)";
    if (c->count_traversal) { *code = SRT_ERR_UNSUPPORTED; return "not on an instrumented context (srt_set_count_traversal(ctx, 0) first)"; }
    const uint32_t held = gather_parts_held(c);
    if (parts & ~(SRT_GATHER_SUMS | SRT_GATHER_COUNTS | SRT_GATHER_FEATURES | SRT_GATHER_FILM)) return "unknown part (SRT_GATHER_SUMS .. SRT_GATHER_FILM)";
    if (parts & ~held) return "the accumulation's kind does not hold that part (COUNTS: adaptive; FEATURES: featured; FILM: spectral)";
    *resolved = parts ? (parts | SRT_GATHER_SUMS) : (held & ~SRT_GATHER_FILM);
    return nullptr;
}
static GatherParams gather_params(const srt_ctx *c, uint32_t resolved, void *unit) {
    GatherParams p = {};
    p.unit = static_cast<uint32_t *>(unit);
    p.sums = reinterpret_cast<uint32_t *>(AccumLayout(c).sums);
    p.n_planes = 3;
    if (resolved & SRT_GATHER_COUNTS) { p.state = AdaptPlanes(c).state; p.sum2 = reinterpret_cast<uint32_t *>(AdaptPlanes(c).sum2); p.n_planes = 5; }
    if (resolved & SRT_GATHER_FEATURES) p.features = reinterpret_cast<uint32_t *>(feature_rows(c));
    if (resolved & SRT_GATHER_FILM) p.film = c->d_film.as<uint32_t>();
    p.tile_words = gather_tile_words(p.n_planes, p.features != nullptr, p.film != nullptr);
    p.n_lanes = c->n_lanes;
    p.width = c->accum.w; p.height = c->accum.h;      // (the bound chunk: the last pass's)
    p.tx = c->tx; p.ty = c->ty; p.bx = c->bx; p.by = c->by;
    p.tiles_x = c->tiles_x; p.n_tiles = c->n_tiles; p.rank = c->rank; p.world = c->world; p.tiles_padded = c->tiles_padded;
    return p;
}
static size_t gather_unit_floats(const srt_ctx *c, uint32_t resolved) {
    return (size_t)c->tiles_padded * gather_tile_words((resolved & SRT_GATHER_COUNTS) ? 5u : 3u, (resolved & SRT_GATHER_FEATURES) != 0, (resolved & SRT_GATHER_FILM) != 0);
}

int srt_accum_exchange_size(srt_ctx *c, uint32_t parts, size_t *n_floats) {
    if (!c || !n_floats) return fail(c, SRT_ERR_INVALID, "srt_accum_exchange_size: null argument");
    uint32_t resolved = 0; int code = 0;
    if (const char *why = gather_refusal(c, parts, &resolved, &code)) return fail(c, code, std::string("srt_accum_exchange_size: ") + why);
    *n_floats = gather_unit_floats(c, resolved);
    return SRT_OK;
}

int srt_pack_accum(srt_ctx *c, uint32_t parts, void *dst_dev, void *stream) {
    if (!c || !dst_dev) return fail(c, SRT_ERR_INVALID, "srt_pack_accum: null argument");
    uint32_t resolved = 0; int code = 0;
    if (const char *why = gather_refusal(c, parts, &resolved, &code)) return fail(c, code, std::string("srt_pack_accum: ") + why);
    HIP_TRY(c, set_device(c, (hipStream_t)stream));
    c->pack_timed = false;
    for (int k = 0; k < 2; k++) if (!c->gather_ev[k]) HIP_TRY(c, hipEventCreate(&c->gather_ev[k]));
    HIP_TRY(c, hipEventRecord(c->gather_ev[0], (hipStream_t)stream));
    HIP_TRY(c, launch_gather(gather_params(c, resolved, dst_dev), false, !c->gather_scalar, (hipStream_t)stream));
    HIP_TRY(c, hipEventRecord(c->gather_ev[1], (hipStream_t)stream));
    c->pack_timed = true;
    return SRT_OK;
}

int srt_internal_gather_reserve(srt_ctx *c, size_t n_floats) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_pack_accum: null argument");
    if (n_floats * sizeof(float) > c->d_gather_unit.bytes) {      // (growing frees the old block: a transport may still be reading it)
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, device_synchronize(c));
        HIP_TRY(c, c->d_gather_unit.reserve(std::max<size_t>(n_floats, 1) * sizeof(float)));
    }
    for (hipEvent_t &e : c->gather_ev) if (!e) { HIP_TRY(c, hipSetDevice(c->device)); HIP_TRY(c, hipEventCreate(&e)); }
    return SRT_OK;
}

int srt_internal_pack_accum_own(srt_ctx *c, uint32_t parts, void *stream, void **unit_dev, size_t *n_floats) {
    if (!c || !unit_dev || !n_floats) return fail(c, SRT_ERR_INVALID, "srt_pack_accum: null argument");
    uint32_t resolved = 0; int code = 0;
    if (const char *why = gather_refusal(c, parts, &resolved, &code)) return fail(c, code, std::string("srt_pack_accum: ") + why);
    const size_t n = gather_unit_floats(c, resolved);
    if (const int rc = srt_internal_gather_reserve(c, n)) return rc;
    *unit_dev = c->d_gather_unit.ptr; *n_floats = n;
    return srt_pack_accum(c, parts, c->d_gather_unit.ptr, stream);
}

int srt_unpack_accum(srt_ctx *c, uint32_t parts, const void *dev_gathered, void *stream) {
    if (!c || !dev_gathered) return fail(c, SRT_ERR_INVALID, "srt_unpack_accum: null argument");
    uint32_t resolved = 0; int code = 0;
    if (const char *why = gather_refusal(c, parts, &resolved, &code)) return fail(c, code, std::string("srt_unpack_accum: ") + why);
    if (c->world > 1) {
        HIP_TRY(c, set_device(c, (hipStream_t)stream));
        c->unpack_timed = false;
        for (int k = 2; k < 4; k++) if (!c->gather_ev[k]) HIP_TRY(c, hipEventCreate(&c->gather_ev[k]));
        HIP_TRY(c, hipEventRecord(c->gather_ev[2], (hipStream_t)stream));
        HIP_TRY(c, launch_gather(gather_params(c, resolved, const_cast<void *>(dev_gathered)), true, !c->gather_scalar, (hipStream_t)stream));
        HIP_TRY(c, hipEventRecord(c->gather_ev[3], (hipStream_t)stream));
        c->unpack_timed = true;
    }
    c->accum.gathered = resolved;
    return SRT_OK;
}

int srt_accum_gathered(const srt_ctx *c, uint32_t *parts) {
    if (!c || !parts) return fail(nullptr, SRT_ERR_INVALID, "srt_accum_gathered: null argument");
    *parts = c->accum.bound() ? c->accum.gathered : 0u;
    return SRT_OK;
}

int srt_accum_whole(const srt_ctx *c, uint32_t parts, int *whole) {
    if (!c || !whole) return fail(nullptr, SRT_ERR_INVALID, "srt_accum_whole: null argument");
    if (parts & ~(SRT_GATHER_SUMS | SRT_GATHER_COUNTS | SRT_GATHER_FEATURES | SRT_GATHER_FILM)) return fail(nullptr, SRT_ERR_INVALID, "srt_accum_whole: unknown part (SRT_GATHER_SUMS .. SRT_GATHER_FILM)");
    *whole = whole_for(c, (parts & SRT_GATHER_FEATURES) != 0, (parts & SRT_GATHER_FILM) != 0) ? 1 : 0;
    return SRT_OK;
}

int srt_gather_last_ms(srt_ctx *c, float *pack_ms, float *unpack_ms) {
    if (!c || (!pack_ms && !unpack_ms)) return fail(c, SRT_ERR_INVALID, "srt_gather_last_ms: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (pack_ms) {
        *pack_ms = 0.f;
        if (c->pack_timed) { HIP_TRY(c, hipEventSynchronize(c->gather_ev[1])); HIP_TRY(c, hipEventElapsedTime(pack_ms, c->gather_ev[0], c->gather_ev[1])); }
    }
    if (unpack_ms) {
        *unpack_ms = 0.f;
        if (c->unpack_timed) { HIP_TRY(c, hipEventSynchronize(c->gather_ev[3])); HIP_TRY(c, hipEventElapsedTime(unpack_ms, c->gather_ev[2], c->gather_ev[3])); }
    }
    return SRT_OK;
}

void srt_internal_gather_descriptor(const srt_ctx *c, uint32_t parts, uint32_t out[kGatherDescriptorWords]) {
    uint32_t resolved = 0; int code = 0;
    const bool ok = c && !gather_refusal(c, parts, &resolved, &code);
    memset(out, 0, kGatherDescriptorWords * sizeof(uint32_t));
    if (!c) return;
    out[0] = ok ? 1u : 0u; out[1] = (uint32_t)c->accum.kind; out[2] = c->accum.total; out[3] = c->accum.n_streams;
    out[4] = c->accum.w; out[5] = c->accum.h; out[6] = c->accum.offx; out[7] = c->accum.offy;
    const uint64_t unit = ok ? (uint64_t)gather_unit_floats(c, resolved) : 0u;
    out[8] = ok ? resolved : parts; out[9] = (uint32_t)unit; out[10] = (uint32_t)(unit >> 32);
}

int srt_dev_fb(srt_ctx *c, void **r, void **g, void **b, size_t *n_floats) {
    if (!c || !c->d_fb) return fail(c, SRT_ERR_INVALID, "srt_dev_fb: device parameters not initialised");
    if (r) *r = fb_plane(c, 0);
    if (g) *g = fb_plane(c, 1);
    if (b) *b = fb_plane(c, 2);
    if (n_floats) *n_floats = c->n_lanes;
    return SRT_OK;
}

int srt_read_fb(srt_ctx *c, float *r, float *g, float *b) { return read_planes(c, 0, r, g, b); }

int srt_read_fb_aux(srt_ctx *c, int which, float *p0, float *p1, float *p2) {
    if (which != 1 && which != 2) return fail(c, SRT_ERR_INVALID, "srt_read_fb_aux: which must be 1 (sRGB) or 2 (XYZ)");
    if (c && (uint32_t)which >= c->fb_groups_valid)
        return fail(c, SRT_ERR_UNSUPPORTED, "srt_read_fb_aux: the parity planes of the last frame were not gathered (the exchange unit was the 3 quantised "
                                            "planes; srt_set_gather_planes / srt_comm_set_gather_planes(.., 9) before rendering moves all nine)");
    return read_planes(c, 3 * which, p0, p1, p2);
}

int srt_read_fb_rowmajor(srt_ctx *c, float *r, float *g, float *b, uint32_t image_width, uint32_t image_height) {
    if (!c || !c->d_fb || !r || !g || !b || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_read_fb_rowmajor: bad argument");
    const float *src[3] = {fb_plane(c, 0), fb_plane(c, 1), fb_plane(c, 2)};
    float *const host[3] = {r, g, b};
    return read_rowmajor(c, src, host, image_width, image_height);
}

int srt_read_accum_stats(srt_ctx *c, uint32_t *samples, float *sum_y, float *sum_y2, uint32_t image_width, uint32_t image_height) {
    if (!c || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_read_accum_stats: bad argument");
    if (!c->accum.bound())
        return fail(c, SRT_ERR_INVALID, "srt_read_accum_stats: no accumulation with a pass (srt_accum_reset[_adaptive] and srt_render_chunk_accum first)");
    if ((samples || sum_y2) && !c->accum.adaptive())
        return fail(c, SRT_ERR_INVALID, "srt_read_accum_stats: sample counts and S2 belong to an adaptive accumulation (srt_accum_reset_adaptive)");
    const float *y = AccumLayout(c).y;
    const float *s2 = c->accum.adaptive() ? AdaptPlanes(c).sum2 : y;
    const float *st = c->accum.adaptive() ? reinterpret_cast<const float *>(AdaptPlanes(c).state) : y;
    const float *src[3] = {st, y, s2};
    float *const host[3] = {reinterpret_cast<float *>(samples), sum_y, sum_y2};
    const int rc = read_rowmajor(c, src, host, image_width, image_height);
    if (rc != SRT_OK || !samples) return rc;
    // the state words carry the converged flag in bit 31: the map holds the sample counts alone
    const ChunkRect rect = chunk_rect(c, image_width, image_height);
    for (uint32_t j = 0; j < rect.h; j++)
        for (uint32_t i = 0; i < rect.w; i++) samples[rect.first + (size_t)j * image_width + i] &= ~kAdaptConverged;
    return SRT_OK;
}

int srt_read_spectral(srt_ctx *c, uint32_t first, uint32_t count, float *out, uint32_t image_width, uint32_t image_height) {
    if (!c || !out || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_read_spectral: bad argument");
    if (count == 0 || (uint64_t)first + count > kFilmSamples)
        return fail(c, SRT_ERR_INVALID, "srt_read_spectral: the range [first, first + count) must be a non-empty part of the 95 grid samples");
    if (!c->accum.spectral() || !c->accum.bound())
        return fail(c, SRT_ERR_INVALID, "srt_read_spectral: no spectral accumulation with a pass (srt_accum_reset_spectral and srt_render_chunk_accum first)");
    HIP_TRY(c, set_device(c));
    // the chunk's rectangle, clipped to the reference grid and the image (srt_read_fb_rowmajor's placement): un-swizzled on the device
    // into a [h][w][count] staging block, then one 2-D copy into the caller's [image_height][image_width][count] array
    const ChunkRect rect = chunk_rect(c, image_width, image_height);
    if (const size_t n = (size_t)rect.w * rect.h * count) {
        HIP_TRY(c, c->d_film_staging.reserve(n * sizeof(float)));
        HIP_TRY(c, launch_film_unswizzle(c->d_film.as<float>(), c->d_film_staging.as<float>(), first, count, rect.w, rect.h, c->tx, c->ty, c->bx, nullptr));
        const size_t row = (size_t)rect.w * count * sizeof(float), pitch = (size_t)image_width * count * sizeof(float);
        HIP_TRY(c, hipMemcpy2D(out + rect.first * count, pitch, c->d_film_staging.ptr, row, row, rect.h, hipMemcpyDeviceToHost));
    }
    HIP_TRY(c, device_synchronize(c));
    return SRT_OK;
}

int srt_read_features(srt_ctx *c, float *out, uint32_t image_width, uint32_t image_height) {
    if (!c || !out || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_read_features: bad argument");
    if (!c->accum.featured() || !c->accum.bound())
        return fail(c, SRT_ERR_INVALID, "srt_read_features: no featured accumulation with a pass (srt_accum_reset_features and srt_render_chunk_accum first)");
    HIP_TRY(c, set_device(c));
    // the chunk's rectangle, clipped to the reference grid and the image (srt_read_fb_rowmajor's placement): un-swizzled on the device
    // into a [h][w][8] staging block, then one 2-D copy into the caller's [image_height][image_width][8] array
    const ChunkRect rect = chunk_rect(c, image_width, image_height);
    if (const size_t n = (size_t)rect.w * rect.h * kFeatureStride) {
        HIP_TRY(c, c->d_features_staging.reserve(n * sizeof(float)));
        HIP_TRY(c, launch_features_unswizzle(feature_rows(c), c->d_features_staging.as<float>(), rect.w, rect.h, c->tx, c->ty, c->bx, nullptr));
        const size_t row = (size_t)rect.w * kFeatureStride * sizeof(float), pitch = (size_t)image_width * kFeatureStride * sizeof(float);
        HIP_TRY(c, hipMemcpy2D(out + rect.first * kFeatureStride, pitch, c->d_features_staging.ptr, row, row, rect.h, hipMemcpyDeviceToHost));
    }
    HIP_TRY(c, device_synchronize(c));
    return SRT_OK;
}

// ---- the developed film (srt_develop.hip) -----------------------------------------------------------------------------------------
namespace {

// d_develop: [the curves, transposed and padded: kFilmSamples x kMaxDevelopChannels floats | developed planes: `channels` floats per pixel
//             | sRGB variant only: out_lin | out_q: 3 floats per pixel each]
struct DevelopLayout {
    float *resp, *out, *lin, *q;
    static constexpr size_t kRespFloats = (size_t)kFilmSamples * kMaxDevelopChannels;
    static size_t bytes(size_t pixels, uint32_t channels, bool srgb) { return (kRespFloats + pixels * (channels + (srgb ? 6u : 0u))) * sizeof(float); }
    DevelopLayout(const DeviceBuffer &d, size_t pixels, uint32_t channels)
        : resp(d.as<float>()), out(resp + kRespFloats), lin(out + pixels * channels), q(lin + 3 * pixels) {}      // (lin, q: inside the buffer only when reserved with srgb)
};

const char *develop_args_error(const float *response, uint32_t channels, float scale) {
    if (channels == 0 || channels > kMaxDevelopChannels) return "channels must be in 1 .. SRT_MAX_DEVELOP_CHANNELS (16)";
    if (!std::isfinite(scale)) return "scale must be finite";
    for (size_t i = 0; i < (size_t)channels * kFilmSamples; i++)
        if (!std::isfinite(response[i])) return "every response must be finite";
    return nullptr;
}

// the colour-matching rows x, y, z of srt_color_tables as three response curves [3][kFilmSamples]
void cie_response_rows(float cie[3 * kFilmSamples]) {
    float rows[96 * 4];
    cmf_rows(rows);
    for (uint32_t k = 0; k < 3; k++)
        for (uint32_t j = 0; j < kFilmSamples; j++) cie[k * kFilmSamples + j] = rows[4 * j + k];
}

// grows a working block; a refused allocation is SRT_ERR_HIP and leaves no error behind for the next launch's hipGetLastError
int develop_reserve(srt_ctx *c, const char *who, DeviceBuffer &d, size_t bytes) {
    if (const hipError_t e = d.reserve(bytes)) {
        (void)hipGetLastError();
        return hip_fail(c, e, who);
    }
    return SRT_OK;
}

// The contraction of the film rows `film` (the lanes of a tx x ty x bx grid, n_lanes of them) over the w x h rectangle into
// DevelopLayout::out, then (samples > 0) the sRGB epilogue into lin / q.  d_develop is reserved by the caller.  Enqueues on the default
// stream; the caller synchronises.  Events: [0] contraction [1] epilogue [2].
// counts (with samples > 0): the state words of an adaptive accumulation, by lane -- the epilogue normalises each pixel by its own count.
int run_develop(srt_ctx *c, const char *who, const float *film, uint32_t n_lanes, uint32_t tx, uint32_t ty, uint32_t bx, uint32_t w, uint32_t h,
                const float *response, uint32_t channels, float scale, uint32_t samples, const uint32_t *counts = nullptr) {
    const size_t pixels = (size_t)w * h;
    const DevelopLayout L(c->d_develop, pixels, channels);
    // the curves as the kernel reads them: [j][kc], the padding +0
    const uint32_t kc = develop_padded_channels(channels);
    std::vector<float> table((size_t)kFilmSamples * kc, 0.0f);
    for (uint32_t k = 0; k < channels; k++)
        for (uint32_t j = 0; j < kFilmSamples; j++) table[(size_t)j * kc + k] = response[(size_t)k * kFilmSamples + j];
    HIP_TRY_AS(c, who, hipMemcpy(L.resp, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    c->develop_timed = false;
    for (hipEvent_t &e : c->develop_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    DevelopParams p = {};
    p.film = film; p.response = L.resp; p.out = L.out; p.scale = scale; p.channels = channels;
    p.n_lanes = n_lanes; p.tx = tx; p.ty = ty; p.bx = bx; p.w = w; p.h = h;
    HIP_TRY_AS(c, who, hipEventRecord(c->develop_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_develop(p, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->develop_ev[1], nullptr));
    if (samples) {
        if (counts) {
            DevelopSrgbCountsParams sp = {};
            sp.xyz = L.out; sp.out_lin = L.lin; sp.out_q = L.q; sp.counts = counts; sp.tx = tx; sp.ty = ty; sp.bx = bx; sp.w = w; sp.h = h;
            HIP_TRY_AS(c, who, launch_develop_srgb_counts(sp, nullptr));
        } else HIP_TRY_AS(c, who, launch_develop_srgb(L.out, L.lin, L.q, samples, pixels, nullptr));
        HIP_TRY_AS(c, who, hipEventRecord(c->develop_ev[2], nullptr));
    }
    c->develop_epilogue = samples != 0; c->develop_timed = true;
    return SRT_OK;
}

// srt_develop_spectral / srt_develop_spectral_srgb behind their argument checks: host[0] the developed planes, host[1 .. 2] the sRGB
// variant's outputs (srgb: the accumulation's sample total normalises them -- each pixel's own count when the accumulation is adaptive)
int develop_accumulation(srt_ctx *c, const char *who, const float *response, uint32_t channels, float scale, bool srgb, float *const host[3],
                         uint32_t image_width, uint32_t image_height) {
    if (!c->accum.spectral() || !c->accum.bound())
        return fail(c, SRT_ERR_INVALID, std::string(who) + ": no spectral accumulation with a pass (srt_accum_reset_spectral and srt_render_chunk_accum first)");
    HIP_TRY(c, set_device(c));
    // the kernel runs on the chunk's rectangle (clipped to the reference grid); the image clips only what is copied out
    const uint32_t w = clipped_w(c), h = clipped_h(c);
    const size_t pixels = (size_t)w * h;
    if (pixels) {
        if (const int rc = develop_reserve(c, who, c->d_develop, DevelopLayout::bytes(pixels, channels, srgb))) return rc;
        if (const int rc = run_develop(c, who, c->d_film.as<float>(), c->n_lanes, c->tx, c->ty, c->bx, w, h, response, channels, scale, srgb ? c->accum.total : 0u,
                                       srgb && c->accum.adaptive() ? AdaptPlanes(c).state : nullptr)) return rc;
        const ChunkRect rect = chunk_rect(c, image_width, image_height);
        const DevelopLayout L(c->d_develop, pixels, channels);
        const float *src[3] = {L.out, L.lin, L.q};
        for (int k = 0; k < (srgb ? 3 : 1); k++) {
            const size_t row = (size_t)rect.w * channels * sizeof(float), src_pitch = (size_t)w * channels * sizeof(float), pitch = (size_t)image_width * channels * sizeof(float);
            if (host[k] && rect.w && rect.h) HIP_TRY(c, hipMemcpy2D(host[k] + rect.first * channels, pitch, src[k], src_pitch, row, rect.h, hipMemcpyDeviceToHost));
        }
    }
    HIP_TRY(c, device_synchronize(c));
    return SRT_OK;
}

}  // namespace

int srt_develop_spectral(srt_ctx *c, const float *response, uint32_t channels, float scale, float *out, uint32_t image_width, uint32_t image_height) {
    if (!c || !response || !out) return fail(c, SRT_ERR_INVALID, "srt_develop_spectral: null argument");
    if (image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_develop_spectral: empty image");
    if (const char *why = develop_args_error(response, channels, scale)) return fail(c, SRT_ERR_INVALID, std::string("srt_develop_spectral: ") + why);
    float *const host[3] = {out, nullptr, nullptr};
    return develop_accumulation(c, "srt_develop_spectral", response, channels, scale, false, host, image_width, image_height);
}

int srt_develop_spectral_srgb(srt_ctx *c, const float *response3, float scale, float *out_xyz, float *out_lin, float *out_q, uint32_t image_width, uint32_t image_height) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_develop_spectral_srgb: null ctx");
    if ((!out_xyz && !out_lin && !out_q) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_develop_spectral_srgb: no output / empty image");
    // response3 == NULL: the colour-matching rows x, y, z of srt_color_tables
    float cie[3 * kFilmSamples];
    if (!response3) {
        cie_response_rows(cie);
        response3 = cie;
    }
    if (const char *why = develop_args_error(response3, 3, scale)) return fail(c, SRT_ERR_INVALID, std::string("srt_develop_spectral_srgb: ") + why);
    float *const host[3] = {out_xyz, out_lin, out_q};
    return develop_accumulation(c, "srt_develop_spectral_srgb", response3, 3, scale, true, host, image_width, image_height);
}

int srt_develop_kat(srt_ctx *c, const float *film, uint32_t n_pixels, const float *response, uint32_t channels, float scale, float *out) {
    if (!c || !film || !response || !out) return fail(c, SRT_ERR_INVALID, "srt_develop_kat: null argument");
    if (n_pixels == 0 || n_pixels > 0x7fffffffu) return fail(c, SRT_ERR_INVALID, "srt_develop_kat: n_pixels must be in 1 .. 2^31 - 1");
    if (const char *why = develop_args_error(response, channels, scale)) return fail(c, SRT_ERR_INVALID, std::string("srt_develop_kat: ") + why);
    HIP_TRY(c, set_device(c));
    const char *who = "srt_develop_kat";
    if (const int rc = develop_reserve(c, who, c->d_develop_in, (size_t)n_pixels * kFilmStride * sizeof(float))) return rc;      // (the larger block first)
    if (const int rc = develop_reserve(c, who, c->d_develop, DevelopLayout::bytes(n_pixels, channels, false))) return rc;
    // 96-float rows; the unused word is a NaN, which no result may show
    std::vector<float> rows((size_t)n_pixels * kFilmStride);
    for (size_t p = 0; p < n_pixels; p++) {
        memcpy(&rows[p * kFilmStride], film + p * kFilmSamples, kFilmSamples * sizeof(float));
        for (uint32_t j = kFilmSamples; j < kFilmStride; j++) rows[p * kFilmStride + j] = NAN;
    }
    HIP_TRY_AS(c, who, hipMemcpy(c->d_develop_in.ptr, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
    // a grid of one n x 1 block makes the block-linear lane the pixel
    if (const int rc = run_develop(c, who, c->d_develop_in.as<float>(), n_pixels, n_pixels, 1, 1, n_pixels, 1, response, channels, scale, 0)) return rc;
    HIP_TRY_AS(c, who, hipMemcpy(out, DevelopLayout(c->d_develop, n_pixels, channels).out, (size_t)n_pixels * channels * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY_AS(c, who, device_synchronize(c));
    return SRT_OK;
}

int srt_develop_last_ms(srt_ctx *c, float *contract_ms, float *epilogue_ms) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_develop_last_ms: null ctx");
    if (!c->develop_timed) return fail(c, SRT_ERR_INVALID, "srt_develop_last_ms: no develop has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->develop_ev[c->develop_epilogue ? 2 : 1]));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->develop_ev[0], c->develop_ev[1]));
    if (contract_ms) *contract_ms = ms;
    ms = 0.0f;
    if (c->develop_epilogue) HIP_TRY(c, hipEventElapsedTime(&ms, c->develop_ev[1], c->develop_ev[2]));
    if (epilogue_ms) *epilogue_ms = ms;
    return SRT_OK;
}

// ---- exposure metering and tone mapping (srt_expose.hip) --------------------------------------------------------------------------
namespace {

// d_expose: [histogram: kMeterBins words | meter counters: metered, dark, non-finite | tone counters: blown, crushed, non-finite (u64 each)]
struct ExposeLayout {
    uint32_t *hist;
    unsigned long long *meter_counts, *tone_counts;
    static constexpr size_t kBytes = kMeterBins * sizeof(uint32_t) + 6 * sizeof(unsigned long long);
    explicit ExposeLayout(const DeviceBuffer &d) : hist(d.as<uint32_t>()), meter_counts(reinterpret_cast<unsigned long long *>(hist + kMeterBins)), tone_counts(meter_counts + 3) {}
};
// d_expose_out: [out_xyz | out_lin | out_q], three floats per pixel each
struct ExposeImages {
    float *img[3];
    static size_t bytes(size_t pixels) { return 9 * pixels * sizeof(float); }
    ExposeImages(const DeviceBuffer &d, size_t pixels) : img{d.as<float>(), d.as<float>() + 3 * pixels, d.as<float>() + 6 * pixels} {}
};

// everything of a srt_meter but where its rectangle lies (the chunk decides that)
const char *meter_cfg_error(const srt_meter *m) {
    if (m->percentile_ppm < 1 || m->percentile_ppm > 1000000u) return "percentile_ppm must be in 1 .. 1000000";
    if (!std::isfinite(m->key) || !(m->key > 0.0f)) return "key must be finite and > 0";
    if (!std::isfinite(m->gain_min) || !std::isfinite(m->gain_max) || !(m->gain_min > 0.0f) || !(m->gain_min <= m->gain_max)) return "needs 0 < gain_min <= gain_max, both finite";
    for (const uint32_t r : m->reserved) if (r) return "the reserved words must be 0";
    const bool whole = !m->x0 && !m->y0 && !m->w && !m->h;
    if (!whole && (m->w == 0 || m->h == 0)) return "the rectangle must be all zero (the whole chunk) or non-empty";
    return nullptr;
}
// ... and the rectangle against a chunk of chunk_w x chunk_h pixels; rect receives the rectangle to meter
const char *meter_rect_error(const srt_meter *m, uint32_t chunk_w, uint32_t chunk_h, uint32_t rect[4]) {
    if (!m->x0 && !m->y0 && !m->w && !m->h) { rect[0] = 0; rect[1] = 0; rect[2] = chunk_w; rect[3] = chunk_h; return nullptr; }
    if ((uint64_t)m->x0 + m->w > chunk_w || (uint64_t)m->y0 + m->h > chunk_h) return "the rectangle must lie inside the chunk";
    rect[0] = m->x0; rect[1] = m->y0; rect[2] = m->w; rect[3] = m->h;
    return nullptr;
}
const char *tone_cfg_error(const srt_tone *t) {
    if (t->curve > 1u) return "curve must be 0 (linear) or 1 (extended Reinhard)";
    if (!std::isfinite(t->gain) || !(t->gain > 0.0f)) return "gain must be finite and > 0";
    if (!(t->white > 0.0f)) return "white must be > 0 (+inf allowed)";
    for (const uint32_t r : t->reserved) if (r) return "the reserved words must be 0";
    return nullptr;
}

// the decision of srt_meter_decide on a validated cfg; dark and nonfinite of *out are not touched
void meter_decide(const uint32_t *hist, const srt_meter *m, srt_meter_result *out) {
    uint64_t n = 0;
    for (uint32_t b = 16; b < 4080; b++) n += hist[b];
    uint32_t bin_ref = 0;
    float y_ref = 0.0f, g = 1.0f;
    if (n) {
        const uint64_t target = std::max<uint64_t>(1, (n * m->percentile_ppm + 999999u) / 1000000u);
        uint64_t run = 0;
        for (uint32_t b = 16; b < 4080; b++) {
            run += hist[b];
            if (run >= target) { bin_ref = b; break; }
        }
        const uint32_t word = (bin_ref << 19) | (1u << 18);
        memcpy(&y_ref, &word, sizeof(y_ref));
        g = m->key / y_ref;
    }
    g = g < m->gain_min ? m->gain_min : g;
    g = g > m->gain_max ? m->gain_max : g;
    out->metered = n; out->bin_ref = bin_ref; out->y_ref = y_ref; out->gain = g; out->reserved = 0;
}

// The meter kernel over the lanes described by p (hist and counts are filled in here), the copy of histogram and counters to the
// host, the decision.  Synchronises.
int run_meter(srt_ctx *c, const char *who, MeterParams p, const srt_meter *cfg, uint32_t *hist_out, srt_meter_result *result) {
    if (const int rc = develop_reserve(c, who, c->d_expose, ExposeLayout::kBytes)) return rc;
    const ExposeLayout L(c->d_expose);
    c->meter_timed = false;
    for (int k = 0; k < 2; k++) if (!c->expose_ev[k]) HIP_TRY_AS(c, who, hipEventCreate(&c->expose_ev[k]));
    HIP_TRY_AS(c, who, hipMemsetAsync(L.hist, 0, kMeterBins * sizeof(uint32_t) + 3 * sizeof(unsigned long long), nullptr));
    p.hist = L.hist; p.counts = L.meter_counts;
    HIP_TRY_AS(c, who, hipEventRecord(c->expose_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_meter(p, (uint32_t)c->n_cu, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->expose_ev[1], nullptr));
    c->meter_timed = true;
    std::vector<uint32_t> host(kMeterBins + 6);      // the histogram and the three 64-bit counters behind it
    HIP_TRY_AS(c, who, hipMemcpy(host.data(), L.hist, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY_AS(c, who, device_synchronize(c));
    unsigned long long counts[3];
    memcpy(counts, host.data() + kMeterBins, sizeof(counts));
    meter_decide(host.data(), cfg, result);
    result->metered = counts[0]; result->dark = counts[1]; result->nonfinite = counts[2];      // (the device's own count: the tests hold it to the histogram's sum)
    if (hist_out) memcpy(hist_out, host.data(), kMeterBins * sizeof(uint32_t));
    return SRT_OK;
}

// The tone kernel over the w x h rectangle described by p (outputs and counts are filled in here) into d_expose_out.  The caller copies
// the images out and synchronises; counts are read here.
int run_tone(srt_ctx *c, const char *who, ToneParams p, const srt_tone *tone, const bool want[3]) {
    const size_t pixels = (size_t)p.w * p.h;
    const ExposeLayout L(c->d_expose);
    const ExposeImages I(c->d_expose_out, pixels);
    c->tone_timed = false;
    for (int k = 2; k < 4; k++) if (!c->expose_ev[k]) HIP_TRY_AS(c, who, hipEventCreate(&c->expose_ev[k]));
    HIP_TRY_AS(c, who, hipMemsetAsync(L.tone_counts, 0, 3 * sizeof(unsigned long long), nullptr));
    p.curve = tone->curve; p.gain = tone->gain; p.kw = tone->white * tone->white;
    p.out_xyz = want[0] ? I.img[0] : nullptr; p.out_lin = want[1] ? I.img[1] : nullptr; p.out_q = want[2] ? I.img[2] : nullptr;
    p.counts = L.tone_counts;
    HIP_TRY_AS(c, who, hipEventRecord(c->expose_ev[2], nullptr));
    HIP_TRY_AS(c, who, launch_tone(p, (uint32_t)c->n_cu, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->expose_ev[3], nullptr));
    c->tone_timed = true;
    return SRT_OK;
}
int read_tone_counts(srt_ctx *c, const char *who, srt_tone_result *result) {
    unsigned long long counts[3] = {0, 0, 0};
    HIP_TRY_AS(c, who, hipMemcpy(counts, ExposeLayout(c->d_expose).tone_counts, sizeof(counts), hipMemcpyDeviceToHost));
    result->blown = counts[0]; result->crushed = counts[1]; result->nonfinite = counts[2];
    return SRT_OK;
}

// a caller's [h][w][3] array on the device (d_expose_in)
int upload_kat_xyz(srt_ctx *c, const char *who, const float *xyz_mean, uint32_t w, uint32_t h) {
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    if (const int rc = develop_reserve(c, who, c->d_expose_in, bytes)) return rc;
    HIP_TRY_AS(c, who, hipMemcpy(c->d_expose_in.ptr, xyz_mean, bytes, hipMemcpyHostToDevice));
    return SRT_OK;
}

}  // namespace

int srt_meter_decide(const uint32_t *hist, const srt_meter *cfg, srt_meter_result *result) {
    if (!hist || !cfg || !result) return fail(nullptr, SRT_ERR_INVALID, "srt_meter_decide: null argument");
    if (const char *why = meter_cfg_error(cfg)) return fail(nullptr, SRT_ERR_INVALID, std::string("srt_meter_decide: ") + why);
    meter_decide(hist, cfg, result);
    return SRT_OK;
}

int srt_meter_accum(srt_ctx *c, const srt_meter *cfg, uint32_t *hist, srt_meter_result *result) {
    const char *who = "srt_meter_accum";
    if (!c || !cfg || !result) return fail(c, SRT_ERR_INVALID, "srt_meter_accum: null argument");
    if (const char *why = meter_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_meter_accum: ") + why);
    if (!c->accum.bound()) return fail(c, SRT_ERR_INVALID, "srt_meter_accum: no accumulation with a pass (srt_accum_reset* and srt_render_chunk_accum first)");
    uint32_t rect[4];
    if (const char *why = meter_rect_error(cfg, clipped_w(c), clipped_h(c), rect)) return fail(c, SRT_ERR_INVALID, std::string("srt_meter_accum: ") + why);
    HIP_TRY(c, set_device(c));
    MeterParams p = {};
    p.y = AccumLayout(c).y; p.y_stride = 1; p.state = c->accum.adaptive() ? AdaptPlanes(c).state : nullptr;
    p.samples = c->accum.total; p.normalise = 1;
    p.n_lanes = c->n_lanes; p.tx = c->tx; p.ty = c->ty; p.bx = c->bx;
    p.x0 = rect[0]; p.y0 = rect[1]; p.w = rect[2]; p.h = rect[3];
    p.tiles_x = c->tiles_x; p.rank = counted_rank(c); p.world = counted_world(c);
    srt_meter_result res = *result;
    if (const int rc = run_meter(c, who, p, cfg, hist, &res)) return rc;
    *result = res;
    return SRT_OK;
}

int srt_meter_kat(srt_ctx *c, const srt_meter *cfg, const float *xyz_mean, uint32_t w, uint32_t h, uint32_t *hist, srt_meter_result *result) {
    const char *who = "srt_meter_kat";
    if (!c || !cfg || !xyz_mean || !result) return fail(c, SRT_ERR_INVALID, "srt_meter_kat: null argument");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, "srt_meter_kat: w x h must be in 1 .. 2^31 - 1");
    if (const char *why = meter_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_meter_kat: ") + why);
    uint32_t rect[4];
    if (const char *why = meter_rect_error(cfg, w, h, rect)) return fail(c, SRT_ERR_INVALID, std::string("srt_meter_kat: ") + why);
    HIP_TRY(c, set_device(c));
    if (const int rc = upload_kat_xyz(c, who, xyz_mean, w, h)) return rc;
    // a grid of one w x h block makes the block-linear lane the row-major pixel
    MeterParams p = {};
    p.y = c->d_expose_in.as<float>() + 1; p.y_stride = 3; p.state = nullptr; p.samples = 1; p.normalise = 0;
    p.n_lanes = w * h; p.tx = w; p.ty = h; p.bx = 1;
    p.x0 = rect[0]; p.y0 = rect[1]; p.w = rect[2]; p.h = rect[3];
    p.tiles_x = (w + 7u) / 8u; p.rank = 0; p.world = 1;
    srt_meter_result res = *result;
    if (const int rc = run_meter(c, who, p, cfg, hist, &res)) return rc;
    *result = res;
    return SRT_OK;
}

int srt_expose_accum(srt_ctx *c, const srt_tone *tone, float *out_xyz, float *out_lin, float *out_q, srt_tone_result *result,
                     uint32_t image_width, uint32_t image_height) {
    const char *who = "srt_expose_accum";
    if (!c || !tone) return fail(c, SRT_ERR_INVALID, "srt_expose_accum: null argument");
    if ((!out_xyz && !out_lin && !out_q) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_expose_accum: no output / empty image");
    if (const char *why = tone_cfg_error(tone)) return fail(c, SRT_ERR_INVALID, std::string("srt_expose_accum: ") + why);
    if (!c->accum.bound()) return fail(c, SRT_ERR_INVALID, "srt_expose_accum: no accumulation with a pass (srt_accum_reset* and srt_render_chunk_accum first)");
    HIP_TRY(c, set_device(c));
    // the kernel runs on the chunk's rectangle (clipped to the reference grid); the image clips only what is copied out
    const uint32_t w = clipped_w(c), h = clipped_h(c);
    const size_t pixels = (size_t)w * h;
    srt_tone_result res = {};
    if (pixels) {
        if (const int rc = develop_reserve(c, who, c->d_expose, ExposeLayout::kBytes)) return rc;
        if (const int rc = develop_reserve(c, who, c->d_expose_out, ExposeImages::bytes(pixels))) return rc;
        ToneParams p = {};
        p.sums = AccumLayout(c).sums; p.comp_stride = c->n_lanes; p.state = c->accum.adaptive() ? AdaptPlanes(c).state : nullptr;
        p.samples = c->accum.total; p.tx = c->tx; p.ty = c->ty; p.bx = c->bx; p.w = w; p.h = h;
        p.tiles_x = c->tiles_x; p.rank = counted_rank(c); p.world = counted_world(c);
        float *const host[3] = {out_xyz, out_lin, out_q};
        const bool want[3] = {out_xyz != nullptr, out_lin != nullptr, out_q != nullptr};
        if (const int rc = run_tone(c, who, p, tone, want)) return rc;
        const ChunkRect rect = chunk_rect(c, image_width, image_height);
        const ExposeImages I(c->d_expose_out, pixels);
        for (int k = 0; k < 3; k++) {
            const size_t row = (size_t)rect.w * 3 * sizeof(float), src_pitch = (size_t)w * 3 * sizeof(float), pitch = (size_t)image_width * 3 * sizeof(float);
            if (host[k] && rect.w && rect.h) HIP_TRY(c, hipMemcpy2D(host[k] + rect.first * 3, pitch, I.img[k], src_pitch, row, rect.h, hipMemcpyDeviceToHost));
        }
        if (const int rc = read_tone_counts(c, who, &res)) return rc;
    }
    HIP_TRY(c, device_synchronize(c));
    if (result) *result = res;
    return SRT_OK;
}

int srt_expose_kat(srt_ctx *c, const srt_tone *tone, const float *xyz_mean, uint32_t w, uint32_t h, float *out_xyz, float *out_lin, float *out_q,
                   srt_tone_result *result) {
    const char *who = "srt_expose_kat";
    if (!c || !tone || !xyz_mean) return fail(c, SRT_ERR_INVALID, "srt_expose_kat: null argument");
    if (!out_xyz && !out_lin && !out_q) return fail(c, SRT_ERR_INVALID, "srt_expose_kat: no output");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, "srt_expose_kat: w x h must be in 1 .. 2^31 - 1");
    if (const char *why = tone_cfg_error(tone)) return fail(c, SRT_ERR_INVALID, std::string("srt_expose_kat: ") + why);
    HIP_TRY(c, set_device(c));
    const size_t pixels = (size_t)w * h;
    if (const int rc = develop_reserve(c, who, c->d_expose_out, ExposeImages::bytes(pixels))) return rc;      // (the larger block first)
    if (const int rc = develop_reserve(c, who, c->d_expose, ExposeLayout::kBytes)) return rc;
    if (const int rc = upload_kat_xyz(c, who, xyz_mean, w, h)) return rc;
    ToneParams p = {};
    p.xyz = c->d_expose_in.as<float>(); p.w = w; p.h = h; p.tiles_x = (w + 7u) / 8u; p.rank = 0; p.world = 1;
    float *const host[3] = {out_xyz, out_lin, out_q};
    const bool want[3] = {out_xyz != nullptr, out_lin != nullptr, out_q != nullptr};
    if (const int rc = run_tone(c, who, p, tone, want)) return rc;
    const ExposeImages I(c->d_expose_out, pixels);
    for (int k = 0; k < 3; k++)
        if (host[k]) HIP_TRY_AS(c, who, hipMemcpy(host[k], I.img[k], pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    srt_tone_result res = {};
    if (const int rc = read_tone_counts(c, who, &res)) return rc;
    HIP_TRY_AS(c, who, device_synchronize(c));
    if (result) *result = res;
    return SRT_OK;
}

int srt_expose_last_ms(srt_ctx *c, float *meter_ms, float *tone_ms) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_expose_last_ms: null ctx");
    if (!c->meter_timed && !c->tone_timed) return fail(c, SRT_ERR_INVALID, "srt_expose_last_ms: neither a meter nor a tone kernel has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    float ms[2] = {0.0f, 0.0f};
    if (c->meter_timed) {
        HIP_TRY(c, hipEventSynchronize(c->expose_ev[1]));
        HIP_TRY(c, hipEventElapsedTime(&ms[0], c->expose_ev[0], c->expose_ev[1]));
    }
    if (c->tone_timed) {
        HIP_TRY(c, hipEventSynchronize(c->expose_ev[3]));
        HIP_TRY(c, hipEventElapsedTime(&ms[1], c->expose_ev[2], c->expose_ev[3]));
    }
    if (meter_ms) *meter_ms = ms[0];
    if (tone_ms) *tone_ms = ms[1];
    return SRT_OK;
}

// ---- the firefly filter (srt_despeckle.hip) ---------------------------------------------------------------------------------------
namespace {

// d_despeckle: [counters: clamped, non-finite, alone (u64 each), padded to 32 bytes | out_xyz | out_lin | out_q: three floats per pixel each
//               | out_scale: one float per pixel]
struct DespeckleLayout {
    unsigned long long *counts;
    float *img[3], *scale;
    static constexpr size_t kHeadBytes = 32;
    static size_t bytes(size_t pixels) { return kHeadBytes + 10 * pixels * sizeof(float); }
    DespeckleLayout(const DeviceBuffer &d, size_t pixels) : counts(d.as<unsigned long long>()) {
        img[0] = reinterpret_cast<float *>(d.as<char>() + kHeadBytes); img[1] = img[0] + 3 * pixels; img[2] = img[1] + 3 * pixels;
        scale = img[2] + 3 * pixels;      // (the images: inside the buffer only when it was reserved with pixels)
    }
};

const char *despeckle_cfg_error(const srt_despeckle *d) {
    if (d->radius != 1u && d->radius != 2u) return "despeckle: radius must be 1 or 2";
    if (d->rank_ppm > 1000000u) return "despeckle: rank_ppm must be in 0 .. 1000000";
    if (!std::isfinite(d->gain) || !(d->gain >= 0.0f)) return "despeckle: gain must be finite and >= 0";
    if (!(d->floor >= 0.0f)) return "despeckle: floor must be >= 0 (+inf switches the filter off)";
    for (const uint32_t r : d->reserved) if (r) return "despeckle: the reserved words must be 0";
    return nullptr;
}

// The despeckle kernel over the w x h rectangle described by p (its source and outputs set by the caller; cfg and counters are filled in
// here), between the context's two despeckle events.  d_despeckle is reserved by the caller.  Enqueues; the caller synchronises.
int run_despeckle(srt_ctx *c, const char *who, DespeckleParams p, const srt_despeckle *cfg) {
    const DespeckleLayout L(c->d_despeckle, 0);
    c->despeckle_timed = false;
    for (hipEvent_t &e : c->despeckle_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    HIP_TRY_AS(c, who, hipMemsetAsync(L.counts, 0, 3 * sizeof(unsigned long long), nullptr));
    p.radius = cfg->radius; p.rank_ppm = cfg->rank_ppm; p.gain = cfg->gain; p.floor = cfg->floor;
    p.counts = L.counts;
    HIP_TRY_AS(c, who, hipEventRecord(c->despeckle_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_despeckle(p, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->despeckle_ev[1], nullptr));
    c->despeckle_timed = true;
    return SRT_OK;
}
int read_despeckle_counts(srt_ctx *c, const char *who, srt_despeckle_result *result) {
    unsigned long long counts[3] = {0, 0, 0};
    HIP_TRY_AS(c, who, hipMemcpy(counts, DespeckleLayout(c->d_despeckle, 0).counts, sizeof(counts), hipMemcpyDeviceToHost));
    result->clamped = counts[0]; result->nonfinite = counts[1]; result->alone = counts[2];
    return SRT_OK;
}

// the accumulation's sum planes as the kernel's source, its chunk rectangle w x h
DespeckleParams despeckle_accum_source(const srt_ctx *c, uint32_t w, uint32_t h) {
    DespeckleParams p = {};
    p.sums = AccumLayout(c).sums; p.comp_stride = c->n_lanes; p.state = c->accum.adaptive() ? AdaptPlanes(c).state : nullptr;
    p.samples = c->accum.total; p.tx = c->tx; p.ty = c->ty; p.bx = c->bx; p.w = w; p.h = h;
    return p;
}

}  // namespace

int srt_despeckle_accum(srt_ctx *c, const srt_despeckle *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_scale, srt_despeckle_result *result,
                        uint32_t image_width, uint32_t image_height) {
    const char *who = "srt_despeckle_accum";
    if (!c || !cfg) return fail(c, SRT_ERR_INVALID, "srt_despeckle_accum: null argument");
    if ((!out_xyz && !out_lin && !out_q && !out_scale && !result) || image_width == 0 || image_height == 0)
        return fail(c, SRT_ERR_INVALID, "srt_despeckle_accum: no output / empty image");
    if (const char *why = despeckle_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_despeckle_accum: ") + why);
    if (!c->accum.bound()) return fail(c, SRT_ERR_INVALID, "srt_despeckle_accum: no accumulation with a pass (srt_accum_reset* and srt_render_chunk_accum first)");
    if (!whole_for(c, false, false))
        return fail(c, SRT_ERR_UNSUPPORTED, std::string("srt_despeckle_accum: ") + kNotWhole);
    HIP_TRY(c, set_device(c));
    // the kernel runs on the chunk's rectangle (clipped to the reference grid); the image clips only what is copied out
    const uint32_t w = clipped_w(c), h = clipped_h(c);
    const size_t pixels = (size_t)w * h;
    srt_despeckle_result res = {};
    if (pixels) {
        if (const int rc = develop_reserve(c, who, c->d_despeckle, DespeckleLayout::bytes(pixels))) return rc;
        const DespeckleLayout L(c->d_despeckle, pixels);
        DespeckleParams p = despeckle_accum_source(c, w, h);
        p.out_xyz = out_xyz ? L.img[0] : nullptr; p.out_lin = out_lin ? L.img[1] : nullptr; p.out_q = out_q ? L.img[2] : nullptr;
        p.out_scale = out_scale ? L.scale : nullptr;
        if (const int rc = run_despeckle(c, who, p, cfg)) return rc;
        const ChunkRect rect = chunk_rect(c, image_width, image_height);
        float *const host[4] = {out_xyz, out_lin, out_q, out_scale};
        const float *const src[4] = {L.img[0], L.img[1], L.img[2], L.scale};
        for (int k = 0; k < 4; k++) {
            const size_t ch = k < 3 ? 3 : 1;      // floats per pixel
            const size_t row = (size_t)rect.w * ch * sizeof(float), src_pitch = (size_t)w * ch * sizeof(float), pitch = (size_t)image_width * ch * sizeof(float);
            if (host[k] && rect.w && rect.h) HIP_TRY(c, hipMemcpy2D(host[k] + rect.first * ch, pitch, src[k], src_pitch, row, rect.h, hipMemcpyDeviceToHost));
        }
        if (const int rc = read_despeckle_counts(c, who, &res)) return rc;
    }
    HIP_TRY(c, device_synchronize(c));
    if (result) *result = res;
    return SRT_OK;
}

int srt_despeckle_kat(srt_ctx *c, const srt_despeckle *cfg, const float *xyz_mean, uint32_t w, uint32_t h, float *out_xyz, float *out_scale,
                      srt_despeckle_result *result) {
    const char *who = "srt_despeckle_kat";
    if (!c || !cfg || !xyz_mean) return fail(c, SRT_ERR_INVALID, "srt_despeckle_kat: null argument");
    if (!out_xyz && !out_scale && !result) return fail(c, SRT_ERR_INVALID, "srt_despeckle_kat: no output");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, "srt_despeckle_kat: w x h must be in 1 .. 2^31 - 1");
    if (const char *why = despeckle_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_despeckle_kat: ") + why);
    HIP_TRY(c, set_device(c));
    const size_t pixels = (size_t)w * h;
    if (const int rc = develop_reserve(c, who, c->d_despeckle, DespeckleLayout::bytes(pixels))) return rc;
    if (const int rc = upload_kat_xyz(c, who, xyz_mean, w, h)) return rc;
    const DespeckleLayout L(c->d_despeckle, pixels);
    DespeckleParams p = {};
    p.xyz = c->d_expose_in.as<float>(); p.w = w; p.h = h;
    p.out_xyz = out_xyz ? L.img[0] : nullptr; p.out_scale = out_scale ? L.scale : nullptr;
    if (const int rc = run_despeckle(c, who, p, cfg)) return rc;
    if (out_xyz) HIP_TRY_AS(c, who, hipMemcpy(out_xyz, L.img[0], pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_scale) HIP_TRY_AS(c, who, hipMemcpy(out_scale, L.scale, pixels * sizeof(float), hipMemcpyDeviceToHost));
    srt_despeckle_result res = {};
    if (const int rc = read_despeckle_counts(c, who, &res)) return rc;
    HIP_TRY_AS(c, who, device_synchronize(c));
    if (result) *result = res;
    return SRT_OK;
}

int srt_despeckle_last_ms(srt_ctx *c, float *ms) {
    if (!c || !ms) return fail(c, SRT_ERR_INVALID, "srt_despeckle_last_ms: null argument");
    if (!c->despeckle_timed) return fail(c, SRT_ERR_INVALID, "srt_despeckle_last_ms: no despeckle kernel has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->despeckle_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->despeckle_ev[0], c->despeckle_ev[1]));
    return SRT_OK;
}

// ---- temporal reprojection (srt_temporal.hip) -------------------------------------------------------------------------------------
namespace {

// d_temporal: [counters: blended, fresh, offscreen, rejected, non-finite (u64 each), padded to 64 bytes | out_xyz | out_lin | out_q: three
//              floats per pixel each | out_len: one | out_motion: two]
struct TemporalLayout {
    unsigned long long *counts;
    float *img[3], *len, *motion;
    static constexpr size_t kHeadBytes = 64;
    static size_t bytes(size_t pixels) { return kHeadBytes + 12 * pixels * sizeof(float); }
    TemporalLayout(const DeviceBuffer &d, size_t pixels) : counts(d.as<unsigned long long>()) {
        img[0] = reinterpret_cast<float *>(d.as<char>() + kHeadBytes); img[1] = img[0] + 3 * pixels; img[2] = img[1] + 3 * pixels;
        len = img[2] + 3 * pixels; motion = len + pixels;      // (the images: inside the buffer only when it was reserved with pixels)
    }
};
// d_temporal_hist: two halves of [Hc: one float4 per pixel | Hg: two]
struct TemporalHistory {
    float4 *colour[2], *guides[2];
    static size_t bytes(size_t pixels) { return 6 * pixels * sizeof(float4); }
    TemporalHistory(const DeviceBuffer &d, size_t pixels) {
        for (int k = 0; k < 2; k++) { colour[k] = d.as<float4>() + 3 * pixels * k; guides[k] = colour[k] + pixels; }
    }
};
// d_temporal_mom: two halves of [Hm: one float4 per pixel], the half k written together with half k of d_temporal_hist
struct TemporalMoments {
    float4 *m[2];
    static size_t bytes(size_t pixels) { return 2 * pixels * sizeof(float4); }
    TemporalMoments(const DeviceBuffer &d, size_t pixels) { m[0] = d.as<float4>(); m[1] = m[0] + pixels; }
};
// d_temporal_var: [the choice kernel's counter (u64), padded to 64 bytes | srt_temporal_variance_kat only: moments: 1 float4 per pixel |
//                  len | spatial | out: one float per pixel each]
struct TemporalVarianceLayout {
    unsigned long long *count;
    float4 *moments;
    float *len, *spatial, *out;
    static constexpr size_t kHeadBytes = 64;
    static size_t bytes(size_t pixels) { return kHeadBytes + pixels * (sizeof(float4) + 3 * sizeof(float)); }
    TemporalVarianceLayout(const DeviceBuffer &d, size_t pixels) : count(d.as<unsigned long long>()) {
        moments = reinterpret_cast<float4 *>(d.as<char>() + kHeadBytes); len = reinterpret_cast<float *>(moments + pixels);
        spatial = len + pixels; out = spatial + pixels;      // (inside the buffer only when it was reserved with pixels)
    }
};
// d_temporal_kat: [guides: 2 float4 per pixel | hist_c: 1 | hist_g: 2 | new_c: 1 | new_g: 2 | (moving: prev_point: 1) | (moments: hist_m: 1 |
//                  new_m: 1) | xyz: three floats per pixel]
struct TemporalKatLayout {
    float4 *guides, *hist_c, *hist_g, *new_c, *new_g;
    float *xyz;
    float4 *prev_point;      // (the moving stage only, else null)
    float4 *hist_m, *new_m;  // (srt_temporal_moments_kat only, else null)
    static size_t bytes(size_t pixels, bool moving = false, bool moments = false) {
        return pixels * ((8 + (moving ? 1 : 0) + (moments ? 2 : 0)) * sizeof(float4) + 3 * sizeof(float));
    }
    TemporalKatLayout(const DeviceBuffer &d, size_t pixels, bool moving = false, bool moments = false) : guides(d.as<float4>()) {
        hist_c = guides + 2 * pixels; hist_g = hist_c + pixels; new_c = hist_g + 2 * pixels; new_g = new_c + pixels;
        float4 *next = new_g + 2 * pixels;
        prev_point = moving ? next : nullptr;
        if (moving) next += pixels;
        hist_m = moments ? next : nullptr; new_m = moments ? next + pixels : nullptr;
        if (moments) next += 2 * pixels;
        xyz = reinterpret_cast<float *>(next);
    }
};
// d_motion: [counters: hit, miss, moved, degenerate (u64 each), padded to 64 bytes | point: one float4 per pixel | tri: one word | bary: three floats]
struct MotionLayout {
    unsigned long long *counts;
    float4 *point;
    int32_t *tri;
    float *bary;
    static constexpr size_t kHeadBytes = 64;
    static size_t bytes(size_t pixels) { return kHeadBytes + pixels * (sizeof(float4) + 4 * sizeof(float)); }
    MotionLayout(const DeviceBuffer &d, size_t pixels) : counts(d.as<unsigned long long>()) {
        point = reinterpret_cast<float4 *>(d.as<char>() + kHeadBytes); tri = reinterpret_cast<int32_t *>(point + pixels);
        bary = reinterpret_cast<float *>(tri + pixels);
    }
};

const char *motion_rect_error(uint32_t w, uint32_t h, uint32_t ox, uint32_t oy) {
    if (w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return "w x h must be in 1 .. 2^31 - 1";
    if ((uint64_t)ox + w > (1ull << 24) || (uint64_t)oy + h > (1ull << 24)) return "ox + w and oy + h must not exceed 2^24";
    return nullptr;
}
// what the bound motion pass needs of the context
const char *motion_bound_refusal(const srt_ctx *c) {
    if (!c->track_motion) return "motion tracking is off (srt_temporal_track_motion first)";
    if (!c->scene_ready || c->verts == srt_ctx::Verts::Unknown) return "the vertices are unknown (srt_upload_scene or a refit after tracking was switched)";
    if (!c->camera_ready) return "no camera set";
    return nullptr;
}
// The motion kernel over the w x h rectangle at (ox, oy) on the uploaded scene under `cam`, between the context's two motion events; the
// outputs are left in MotionLayout(c->d_motion, w * h), which is reserved here.  Enqueues; the caller synchronises.
int run_motion_kernel(srt_ctx *c, const char *who, const srt_camera_data &cam, const float *v_cur, const float *v_prev, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy) {
    const size_t pixels = (size_t)w * h;
    if (const int rc = develop_reserve(c, who, c->d_motion, MotionLayout::bytes(pixels))) return rc;
    const MotionLayout L(c->d_motion, pixels);
    c->motion_timed = false;
    for (hipEvent_t &e : c->motion_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    MotionParams p = {};
    p.nodes = c->d_nodes.as<const float4>(); p.fringe = c->d_fringe.as<const float4>(); p.tris = c->d_tris.as<const float4>();
    p.root_ref = c->root_ref; p.stack_depth = c->stack_depth; p.n_inner = c->n_inner; p.n_records = c->n_records;
    p.fringe_stride = c->fringe_stride; p.n_tris = c->n_tris;
    p.v_cur = v_cur; p.v_prev = v_prev;
    p.w = w; p.h = h; p.ox = ox; p.oy = oy;
    for (int k = 0; k < 3; k++) { p.du[k] = cam.pixel_delta_u[k]; p.dv[k] = cam.pixel_delta_v[k]; p.p00[k] = cam.pixel00_loc[k]; p.center[k] = cam.camera_center[k]; }
    p.out_point = L.point; p.out_tri = L.tri; p.out_bary = L.bary; p.counts = L.counts;
    HIP_TRY_AS(c, who, hipMemsetAsync(L.counts, 0, 4 * sizeof(unsigned long long), nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->motion_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_motion(p, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->motion_ev[1], nullptr));
    c->motion_timed = true;
    return SRT_OK;
}
// the pass on the context's own camera and vertex state: V_prev = V_hist, or V_cur when V_hist is none
int run_motion_bound(srt_ctx *c, const char *who, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy) {
    if (const int rc = track_verts_to_device(c, who)) return rc;
    return run_motion_kernel(c, who, c->cam, c->d_verts_cur.as<float>(), c->verts_hist ? c->d_verts_hist.as<float>() : nullptr, w, h, ox, oy);
}
int read_motion_counts(srt_ctx *c, const char *who, srt_motion_result *result) {
    unsigned long long counts[4] = {0, 0, 0, 0};
    HIP_TRY_AS(c, who, hipMemcpy(counts, MotionLayout(c->d_motion, 0).counts, sizeof(counts), hipMemcpyDeviceToHost));
    result->hit = counts[0]; result->miss = counts[1]; result->moved = counts[2]; result->degenerate = counts[3];
    return SRT_OK;
}
int read_motion_outputs(srt_ctx *c, const char *who, size_t pixels, float *out_point, int32_t *out_tri, float *out_bary, srt_motion_result *result) {
    const MotionLayout L(c->d_motion, pixels);
    if (out_point) HIP_TRY_AS(c, who, hipMemcpy(out_point, L.point, pixels * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_tri) HIP_TRY_AS(c, who, hipMemcpy(out_tri, L.tri, pixels * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_bary) HIP_TRY_AS(c, who, hipMemcpy(out_bary, L.bary, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    srt_motion_result res = {};
    if (const int rc = read_motion_counts(c, who, &res)) return rc;
    HIP_TRY_AS(c, who, device_synchronize(c));
    if (result) *result = res;
    return SRT_OK;
}

const char *temporal_cfg_error(const srt_temporal *t) {
    if (!(t->alpha_min > 0.0f && t->alpha_min <= 1.0f)) return "temporal: alpha_min must be in (0, 1]";
    if (!(t->max_len >= 1.0f) || !std::isfinite(t->max_len)) return "temporal: max_len must be finite and >= 1";
    for (const float s : {t->sigma_normal, t->sigma_albedo, t->sigma_depth})
        if (!(s > 0.0f)) return "temporal: every sigma must be greater than 0 (+inf switches its test off)";
    for (const uint32_t r : t->reserved) if (r) return "temporal: the reserved words must be 0";
    return nullptr;
}

const char *temporal_vg_cfg_error(const srt_temporal_vg *t) {
    if (t->min_len < 2u || t->min_len > (1u << 24)) return "temporal_vg: min_len must be in 2 .. 2^24";
    if (t->moving > 1u) return "temporal_vg: moving must be 0 or 1";
    if (t->reserved[0] | t->reserved[1]) return "temporal_vg: the reserved words must be 0";
    return nullptr;
}

// the host constants of srt_c_api.h, fp32, one rounding per operation (this unit is built without contraction)
struct Vec3f { float x, y, z; };
Vec3f vec3f(const float a[3]) { return {a[0], a[1], a[2]}; }
float dot3f(Vec3f a, Vec3f b) { const float s = a.x * b.x + a.y * b.y; return s + a.z * b.z; }
Vec3f cross3f(Vec3f a, Vec3f b) {
    const float x0 = a.y * b.z, x1 = a.z * b.y, y0 = a.z * b.x, y1 = a.x * b.z, z0 = a.x * b.y, z1 = a.y * b.x;
    return {x0 - x1, y0 - y1, z0 - z1};
}
void put3f(float dst[3], Vec3f v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }
void temporal_cameras(TemporalParams &p, const srt_camera_data &cur, const srt_camera_data *prev) {
    for (int k = 0; k < 3; k++) { p.du[k] = cur.pixel_delta_u[k]; p.dv[k] = cur.pixel_delta_v[k]; p.p00[k] = cur.pixel00_loc[k]; p.center[k] = cur.camera_center[k]; }
    if (!prev) return;
    const Vec3f du = vec3f(prev->pixel_delta_u), dv = vec3f(prev->pixel_delta_v), p00 = vec3f(prev->pixel00_loc), ce = vec3f(prev->camera_center);
    const Vec3f n = cross3f(du, dv);
    const Vec3f e = {p00.x - ce.x, p00.y - ce.y, p00.z - ce.z};
    const Vec3f cu = cross3f(dv, n), cv = cross3f(n, du);
    const float su = dot3f(du, cu), sv = dot3f(dv, cv);
    put3f(p.pcenter, ce); put3f(p.pn, n); put3f(p.pe, e);
    p.pk = dot3f(e, n);
    put3f(p.pbu, {cu.x / su, cu.y / su, cu.z / su});
    put3f(p.pbv, {cv.x / sv, cv.y / sv, cv.z / sv});
}

// The temporal kernel over the rectangle described by p (its sources, history, outputs and rectangle set by the caller; cfg, cameras and
// counters are filled in here), between the context's two temporal events.  d_temporal is reserved by the caller.  Enqueues; the caller
// synchronises.  prev: the camera of p's history (not read without one).
int run_temporal_kernel(srt_ctx *c, const char *who, TemporalParams p, const srt_temporal *cfg, const srt_camera_data &cur, const srt_camera_data *prev) {
    const TemporalLayout L(c->d_temporal, 0);
    c->temporal_timed = false;
    for (hipEvent_t &e : c->temporal_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    HIP_TRY_AS(c, who, hipMemsetAsync(L.counts, 0, 5 * sizeof(unsigned long long), nullptr));
    temporal_cameras(p, cur, p.hist_c ? prev : nullptr);
    p.kn = cfg->sigma_normal * cfg->sigma_normal; p.ka = cfg->sigma_albedo * cfg->sigma_albedo; p.kz = cfg->sigma_depth * cfg->sigma_depth;
    p.alpha_min = cfg->alpha_min; p.max_len = cfg->max_len;
    p.counts = L.counts;
    HIP_TRY_AS(c, who, hipEventRecord(c->temporal_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_temporal(p, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->temporal_ev[1], nullptr));
    c->temporal_timed = true;
    return SRT_OK;
}

// The stage on the context's history: p holds the sources, dst4 and outputs of the w x h rectangle of the last chunk.  A history of another
// rectangle is discarded (res->history_dropped).  The history advances when the kernel has been enqueued.  d_temporal is reserved by the caller.
// moments: the call carries Hm (srt_*_temporal_vg) -- gathered when the previous call wrote one, seeded otherwise; a call without marks it absent.
int run_temporal_history(srt_ctx *c, const char *who, TemporalParams p, const srt_temporal *cfg, srt_temporal_result *res, bool moments = false) {
    const uint32_t rect[4] = {p.w, p.h, c->last_offx, c->last_offy};
    const size_t pixels = (size_t)p.w * p.h;
    res->history_dropped = 0;
    if (!p.prev_point && c->refits_pending) c->temporal_frames = 0;      // (a tracking context's static call: the history shows geometry that has moved)
    if (c->temporal_frames && memcmp(rect, c->temporal_rect, sizeof(rect)) != 0) {
        c->temporal_frames = 0;
        res->history_dropped = 1;
    }
    if (!c->temporal_frames) {      // (only a first frame may grow the block: growing loses what it holds)
        if (const int rc = develop_reserve(c, who, c->d_temporal_hist, TemporalHistory::bytes(pixels))) return rc;
    }
    const TemporalHistory H(c->d_temporal_hist, pixels);
    const uint32_t old = c->temporal_cur, neu = old ^ 1u;
    p.hist_c = c->temporal_frames ? H.colour[old] : nullptr; p.hist_g = c->temporal_frames ? H.guides[old] : nullptr;
    p.new_c = H.colour[neu]; p.new_g = H.guides[neu];
    if (moments) {      // (allocated by the first call that asks; growing happens only where no Hm is present: a present one has this rectangle)
        if (const int rc = develop_reserve(c, who, c->d_temporal_mom, TemporalMoments::bytes(pixels))) return rc;
        const TemporalMoments M(c->d_temporal_mom, pixels);
        p.hist_m = (c->temporal_frames && c->temporal_moments) ? M.m[old] : nullptr; p.new_m = M.m[neu];
    }
    p.ox = c->last_offx; p.oy = c->last_offy;
    if (const int rc = run_temporal_kernel(c, who, p, cfg, c->cam, &c->temporal_cam)) {
        c->temporal_frames = 0;      // (a launch that failed may have left half a history)
        return rc;
    }
    c->temporal_cur = neu; c->temporal_frames++; c->temporal_cam = c->cam;
    c->temporal_moments = moments;
    c->verts_hist = false; c->refits_pending = 0;      // (the new history shows V_cur)
    memcpy(c->temporal_rect, rect, sizeof(rect));
    res->history_frames = c->temporal_frames;
    return SRT_OK;
}

int read_temporal_counts(srt_ctx *c, const char *who, srt_temporal_result *result) {
    unsigned long long counts[5] = {0, 0, 0, 0, 0};
    HIP_TRY_AS(c, who, hipMemcpy(counts, TemporalLayout(c->d_temporal, 0).counts, sizeof(counts), hipMemcpyDeviceToHost));
    result->blended = counts[0]; result->fresh = counts[1]; result->offscreen = counts[2]; result->rejected = counts[3]; result->nonfinite = counts[4];
    return SRT_OK;
}

// what a chained call asks of the stage: its configuration, whether TemporalLayout's out_xyz is filled, and the result (history_frames and
// history_dropped when the kernel is enqueued; the counters are read by the caller once the chain has run)
struct TemporalStage {
    const srt_temporal *cfg;
    bool out_xyz;
    srt_temporal_result res;
    bool moving = false;      // the *_moving calls: the motion pass on the rectangle first, then the moving stage on its points
    srt_motion_result mres = {};
    const srt_temporal_vg *tv = nullptr;      // srt_*_temporal_vg (variance-guided plans only): the moments stage, then the estimator and the choice
    unsigned long long n_temporal = 0;        // ... the pixels that took the temporal variance (read by the caller with the counters)
};

// The choice kernel on p (everything but the counter set by the caller), between the context's two events of its own.  d_temporal_var is
// reserved by the caller.  Enqueues; the caller synchronises.
int run_temporal_variance(srt_ctx *c, const char *who, TemporalVarianceParams p) {
    c->temporal_var_timed = false;
    for (hipEvent_t &e : c->temporal_var_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    p.count = TemporalVarianceLayout(c->d_temporal_var, 0).count;
    HIP_TRY_AS(c, who, hipMemsetAsync(p.count, 0, sizeof(unsigned long long), nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->temporal_var_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_temporal_variance(p, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->temporal_var_ev[1], nullptr));
    c->temporal_var_timed = true;
    return SRT_OK;
}
int read_temporal_variance_count(srt_ctx *c, const char *who, unsigned long long *n) {
    HIP_TRY_AS(c, who, hipMemcpy(n, TemporalVarianceLayout(c->d_temporal_var, 0).count, sizeof(*n), hipMemcpyDeviceToHost));
    return SRT_OK;
}

}  // namespace

int srt_temporal_reset(srt_ctx *c) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_temporal_reset: null ctx");
    c->temporal_frames = 0;
    c->verts_hist = false; c->refits_pending = 0;
    return SRT_OK;
}

// srt_temporal_kat (moving false, prev_point not read) and srt_temporal_moving_kat (moving true: prev_point[h][w][4], not null);
// srt_temporal_moments_kat (moments true: hist_moments[h][w][4], read with a history only and null for none, and out_moments[h][w][4])
static int temporal_kat(srt_ctx *c, const char *who, const srt_temporal *cfg, const srt_camera_data *cur_cam, const srt_camera_data *prev_cam, const float *xyz_mean,
                        const float *guides, const float *hist_colour, const float *hist_guides, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy,
                        float *out_colour, float *out_guides, float *out_motion, srt_temporal_result *result, bool moving, const float *prev_point,
                        bool moments = false, const float *hist_moments = nullptr, float *out_moments = nullptr) {
    const std::string w_(std::string(who) + ": ");
    if (!c || !cfg || !cur_cam || !xyz_mean || !guides || (moving && !prev_point)) return fail(c, SRT_ERR_INVALID, w_ + "null argument");
    if (!out_colour && !out_guides && !out_motion && !out_moments && !result) return fail(c, SRT_ERR_INVALID, w_ + "no output");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, w_ + "w x h must be in 1 .. 2^31 - 1");
    if ((uint64_t)ox + w > (1ull << 24) || (uint64_t)oy + h > (1ull << 24)) return fail(c, SRT_ERR_INVALID, w_ + "ox + w and oy + h must not exceed 2^24");
    if (const char *why = temporal_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    const bool history = prev_cam && hist_colour && hist_guides;
    HIP_TRY(c, set_device(c));
    const size_t pixels = (size_t)w * h;
    if (const int rc = develop_reserve(c, who, c->d_temporal, TemporalLayout::bytes(pixels))) return rc;
    if (const int rc = develop_reserve(c, who, c->d_temporal_kat, TemporalKatLayout::bytes(pixels, moving, moments))) return rc;
    const TemporalLayout L(c->d_temporal, pixels);
    const TemporalKatLayout K(c->d_temporal_kat, pixels, moving, moments);
    if (moving) HIP_TRY_AS(c, who, hipMemcpy(K.prev_point, prev_point, pixels * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, who, hipMemcpy(K.xyz, xyz_mean, pixels * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, who, hipMemcpy(K.guides, guides, pixels * 2 * sizeof(float4), hipMemcpyHostToDevice));
    if (history) {
        HIP_TRY_AS(c, who, hipMemcpy(K.hist_c, hist_colour, pixels * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY_AS(c, who, hipMemcpy(K.hist_g, hist_guides, pixels * 2 * sizeof(float4), hipMemcpyHostToDevice));
        if (moments && hist_moments) HIP_TRY_AS(c, who, hipMemcpy(K.hist_m, hist_moments, pixels * sizeof(float4), hipMemcpyHostToDevice));
    }
    TemporalParams p = {};
    p.xyz = K.xyz; p.guides = K.guides; p.hist_c = history ? K.hist_c : nullptr; p.hist_g = history ? K.hist_g : nullptr;
    p.new_c = K.new_c; p.new_g = K.new_g; p.w = w; p.h = h; p.ox = ox; p.oy = oy;
    p.out_motion = out_motion ? L.motion : nullptr;
    p.prev_point = K.prev_point;
    p.hist_m = (history && hist_moments) ? K.hist_m : nullptr; p.new_m = K.new_m;
    if (const int rc = run_temporal_kernel(c, who, p, cfg, *cur_cam, prev_cam)) return rc;
    if (out_moments) HIP_TRY_AS(c, who, hipMemcpy(out_moments, K.new_m, pixels * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_colour) HIP_TRY_AS(c, who, hipMemcpy(out_colour, K.new_c, pixels * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_guides) HIP_TRY_AS(c, who, hipMemcpy(out_guides, K.new_g, pixels * 2 * sizeof(float4), hipMemcpyDeviceToHost));
    if (out_motion) HIP_TRY_AS(c, who, hipMemcpy(out_motion, L.motion, pixels * 2 * sizeof(float), hipMemcpyDeviceToHost));
    srt_temporal_result res = {};
    if (const int rc = read_temporal_counts(c, who, &res)) return rc;
    res.history_frames = history ? 2u : 1u;
    HIP_TRY_AS(c, who, device_synchronize(c));
    if (result) *result = res;
    return SRT_OK;
}

int srt_temporal_kat(srt_ctx *c, const srt_temporal *cfg, const srt_camera_data *cur_cam, const srt_camera_data *prev_cam, const float *xyz_mean,
                     const float *guides, const float *hist_colour, const float *hist_guides, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy,
                     float *out_colour, float *out_guides, float *out_motion, srt_temporal_result *result) {
    return temporal_kat(c, "srt_temporal_kat", cfg, cur_cam, prev_cam, xyz_mean, guides, hist_colour, hist_guides, w, h, ox, oy, out_colour, out_guides, out_motion,
                        result, false, nullptr);
}

int srt_temporal_moving_kat(srt_ctx *c, const srt_temporal *cfg, const srt_camera_data *cur_cam, const srt_camera_data *prev_cam, const float *xyz_mean,
                            const float *guides, const float *hist_colour, const float *hist_guides, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy,
                            float *out_colour, float *out_guides, float *out_motion, srt_temporal_result *result, const float *prev_point) {
    return temporal_kat(c, "srt_temporal_moving_kat", cfg, cur_cam, prev_cam, xyz_mean, guides, hist_colour, hist_guides, w, h, ox, oy, out_colour, out_guides,
                        out_motion, result, true, prev_point);
}

int srt_temporal_moments_kat(srt_ctx *c, const srt_temporal *cfg, const srt_camera_data *cur_cam, const srt_camera_data *prev_cam, const float *xyz_mean,
                             const float *guides, const float *hist_colour, const float *hist_guides, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy,
                             float *out_colour, float *out_guides, float *out_motion, srt_temporal_result *result, const float *prev_point,
                             const float *hist_moments, float *out_moments) {
    return temporal_kat(c, "srt_temporal_moments_kat", cfg, cur_cam, prev_cam, xyz_mean, guides, hist_colour, hist_guides, w, h, ox, oy, out_colour, out_guides,
                        out_motion, result, prev_point != nullptr, prev_point, true, hist_moments, out_moments);
}

int srt_temporal_variance_kat(srt_ctx *c, const float *moments, const float *len, const float *spatial_var, uint32_t min_len, uint32_t w, uint32_t h,
                              float *out_var, uint64_t *n_temporal) {
    const char *who = "srt_temporal_variance_kat";
    if (!c || !moments || !len || !spatial_var) return fail(c, SRT_ERR_INVALID, "srt_temporal_variance_kat: null argument");
    if (!out_var && !n_temporal) return fail(c, SRT_ERR_INVALID, "srt_temporal_variance_kat: no output");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, "srt_temporal_variance_kat: w x h must be in 1 .. 2^31 - 1");
    if (min_len < 2u || min_len > (1u << 24)) return fail(c, SRT_ERR_INVALID, "srt_temporal_variance_kat: min_len must be in 2 .. 2^24");
    HIP_TRY(c, set_device(c));
    const size_t pixels = (size_t)w * h;
    if (const int rc = develop_reserve(c, who, c->d_temporal_var, TemporalVarianceLayout::bytes(pixels))) return rc;
    const TemporalVarianceLayout V(c->d_temporal_var, pixels);
    HIP_TRY_AS(c, who, hipMemcpy(V.moments, moments, pixels * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, who, hipMemcpy(V.len, len, pixels * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, who, hipMemcpy(V.spatial, spatial_var, pixels * sizeof(float), hipMemcpyHostToDevice));
    TemporalVarianceParams p = {};
    p.moments = V.moments; p.len = V.len; p.spatial = V.spatial; p.len_stride = 1; p.spatial_stride = 1; p.out_stride = 1;
    p.ml_min = (float)min_len; p.n = (uint32_t)pixels; p.out_var = V.out;
    if (const int rc = run_temporal_variance(c, who, p)) return rc;
    if (out_var) HIP_TRY_AS(c, who, hipMemcpy(out_var, V.out, pixels * sizeof(float), hipMemcpyDeviceToHost));
    unsigned long long n = 0;
    if (const int rc = read_temporal_variance_count(c, who, &n)) return rc;
    HIP_TRY_AS(c, who, device_synchronize(c));
    if (n_temporal) *n_temporal = n;
    return SRT_OK;
}

int srt_read_temporal_moments(srt_ctx *c, float *out, uint32_t image_width, uint32_t image_height) {
    const char *who = "srt_read_temporal_moments";
    if (!c || !out || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_read_temporal_moments: null argument / empty image");
    if (!c->temporal_frames || !c->temporal_moments) return fail(c, SRT_ERR_INVALID, "srt_read_temporal_moments: the context holds no moments history");
    HIP_TRY(c, set_device(c));
    const uint32_t w = c->temporal_rect[0], h = c->temporal_rect[1], ox = c->temporal_rect[2], oy = c->temporal_rect[3];
    if (ox < image_width && oy < image_height) {      // the history's rectangle, placed and clipped as the stage's outputs are
        const uint32_t cw = std::min<uint32_t>(w, image_width - ox), ch = std::min<uint32_t>(h, image_height - oy);
        const float4 *src = TemporalMoments(c->d_temporal_mom, (size_t)w * h).m[c->temporal_cur];
        HIP_TRY_AS(c, who, hipMemcpy2D(out + ((size_t)oy * image_width + ox) * 4, (size_t)image_width * sizeof(float4), src, (size_t)w * sizeof(float4),
                                       (size_t)cw * sizeof(float4), ch, hipMemcpyDeviceToHost));
    }
    HIP_TRY_AS(c, who, device_synchronize(c));
    return SRT_OK;
}

int srt_temporal_variance_last_ms(srt_ctx *c, float *ms) {
    if (!c || !ms) return fail(c, SRT_ERR_INVALID, "srt_temporal_variance_last_ms: null argument");
    if (!c->temporal_var_timed) return fail(c, SRT_ERR_INVALID, "srt_temporal_variance_last_ms: no choice kernel has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->temporal_var_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->temporal_var_ev[0], c->temporal_var_ev[1]));
    return SRT_OK;
}

// ---- surface motion (srt_motion.hip) ---------------------------------------------------------------------------------------------
int srt_temporal_track_motion(srt_ctx *c, int on) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_temporal_track_motion: null ctx");
    if ((on != 0) == c->track_motion) return SRT_OK;
    c->track_motion = on != 0;
    c->temporal_frames = 0;      // (the history was written under the other rule)
    c->verts = srt_ctx::Verts::Unknown; c->verts_hist = false; c->refits_pending = 0;
    c->track_verts.clear();
    if (!c->track_motion) {      // with tracking off none of this state exists
        HIP_TRY(c, set_device(c));
        c->d_verts_cur.release(); c->d_verts_hist.release();
    }
    return SRT_OK;
}

int srt_temporal_tracking(const srt_ctx *c, int *on, uint32_t *refits_pending) {
    if (!c) return fail(nullptr, SRT_ERR_INVALID, "srt_temporal_tracking: null ctx");
    if (on) *on = c->track_motion ? 1 : 0;
    if (refits_pending) *refits_pending = c->refits_pending;
    return SRT_OK;
}

int srt_surface_motion(srt_ctx *c, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, float *out_point, int32_t *out_tri, float *out_bary, srt_motion_result *result) {
    const char *who = "srt_surface_motion";
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_surface_motion: null ctx");
    if (!out_point && !out_tri && !out_bary && !result) return fail(c, SRT_ERR_INVALID, "srt_surface_motion: no output");
    if (const char *why = motion_rect_error(w, h, ox, oy)) return fail(c, SRT_ERR_INVALID, std::string("srt_surface_motion: ") + why);
    if (const char *why = motion_bound_refusal(c)) return fail(c, SRT_ERR_INVALID, std::string("srt_surface_motion: ") + why);
    HIP_TRY(c, set_device(c));
    if (const int rc = run_motion_bound(c, who, w, h, ox, oy)) return rc;
    return read_motion_outputs(c, who, (size_t)w * h, out_point, out_tri, out_bary, result);
}

int srt_surface_motion_kat(srt_ctx *c, const srt_camera_data *cam, const float *prev_verts, const float *cur_verts, size_t n_tris, uint32_t w, uint32_t h, uint32_t ox,
                           uint32_t oy, float *out_point, int32_t *out_tri, float *out_bary, srt_motion_result *result) {
    const char *who = "srt_surface_motion_kat";
    if (!c || !cam || !cur_verts) return fail(c, SRT_ERR_INVALID, "srt_surface_motion_kat: null argument");
    if (!c->scene_ready) return fail(c, SRT_ERR_INVALID, "srt_surface_motion_kat: no scene uploaded");
    if (n_tris != c->n_tris) return fail(c, SRT_ERR_INVALID, "srt_surface_motion_kat: n_tris is not the uploaded scene's triangle count");
    if (!out_point && !out_tri && !out_bary && !result) return fail(c, SRT_ERR_INVALID, "srt_surface_motion_kat: no output");
    if (const char *why = motion_rect_error(w, h, ox, oy)) return fail(c, SRT_ERR_INVALID, std::string("srt_surface_motion_kat: ") + why);
    for (const float *v : {cur_verts, prev_verts})
        for (size_t k = 0; v && k < 9 * n_tris; k++)
            if (!std::isfinite(v[k])) return fail(c, SRT_ERR_INVALID, "srt_surface_motion_kat: a coordinate is not finite");
    HIP_TRY(c, set_device(c));
    const size_t block = 9 * n_tris * sizeof(float);
    if (const int rc = develop_reserve(c, who, c->d_motion_kat, 2 * block)) return rc;
    float *d_cur = c->d_motion_kat.as<float>(), *d_prev = d_cur + 9 * n_tris;
    HIP_TRY_AS(c, who, hipMemcpy(d_cur, cur_verts, block, hipMemcpyHostToDevice));
    if (prev_verts) HIP_TRY_AS(c, who, hipMemcpy(d_prev, prev_verts, block, hipMemcpyHostToDevice));
    if (const int rc = run_motion_kernel(c, who, *cam, d_cur, prev_verts ? d_prev : nullptr, w, h, ox, oy)) return rc;
    return read_motion_outputs(c, who, (size_t)w * h, out_point, out_tri, out_bary, result);
}

int srt_motion_last_ms(srt_ctx *c, float *ms) {
    if (!c || !ms) return fail(c, SRT_ERR_INVALID, "srt_motion_last_ms: null argument");
    if (!c->motion_timed) return fail(c, SRT_ERR_INVALID, "srt_motion_last_ms: no motion kernel has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->motion_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->motion_ev[0], c->motion_ev[1]));
    return SRT_OK;
}

int srt_temporal_last_ms(srt_ctx *c, float *ms) {
    if (!c || !ms) return fail(c, SRT_ERR_INVALID, "srt_temporal_last_ms: null argument");
    if (!c->temporal_timed) return fail(c, SRT_ERR_INVALID, "srt_temporal_last_ms: no temporal kernel has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->temporal_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->temporal_ev[0], c->temporal_ev[1]));
    return SRT_OK;
}

// ---- the denoiser (srt_denoise.hip) ---------------------------------------------------------------------------------------------
namespace {

// d_denoise: [guides: 2 float4 per pixel | colour A | colour B: 1 float4 per pixel each | out_xyz | out_lin | out_q: 3 floats per pixel each
//             | variance-guided only: out_var: 2 floats per pixel]
struct DenoiseLayout {
    float4 *guides, *colour[2];
    float *out[3], *var;
    static size_t bytes(size_t pixels, bool vg) { return pixels * (4 * sizeof(float4) + 9 * sizeof(float) + (vg ? 2 * sizeof(float) : 0)); }
    DenoiseLayout(const DeviceBuffer &d, size_t pixels) : guides(d.as<float4>()) {
        colour[0] = guides + 2 * pixels; colour[1] = colour[0] + pixels;
        out[0] = reinterpret_cast<float *>(colour[1] + pixels); out[1] = out[0] + 3 * pixels; out[2] = out[1] + 3 * pixels;
        var = out[2] + 3 * pixels;      // (inside the buffer only when it was reserved with vg)
    }
};

// What either configuration struct asks of the kernels: the plain filter's sigma_color, or the variance-guided filter's two constants.
struct DenoisePlan {
    bool vg;
    bool measured;          // variance-guided with the measured per-pixel estimator (srt_denoise_features_mv) in the spatial one's place
    uint32_t levels;
    float kn, ka, kz;
    float sigma_color;      // plain
    float ks, floor;        // variance-guided: sigma_variance * sigma_variance (formed once, here), variance_floor
};

const char *denoise_cfg_error(const srt_denoise *cfg) {
    if (cfg->levels > 8) return "levels must be in 0 .. 8";
    for (const float s : {cfg->sigma_color, cfg->sigma_normal, cfg->sigma_albedo, cfg->sigma_depth})
        if (!(s > 0.0f)) return "every sigma must be greater than 0 (+inf switches its term off)";
    if (cfg->reserved[0] | cfg->reserved[1] | cfg->reserved[2]) return "reserved words must be 0";
    return nullptr;
}

const char *denoise_vg_cfg_error(const srt_denoise_vg *cfg) {
    if (cfg->levels > 8) return "levels must be in 0 .. 8";
    if (!(cfg->sigma_variance > 0.0f) || std::isinf(cfg->sigma_variance)) return "sigma_variance must be greater than 0 and finite";
    for (const float s : {cfg->sigma_normal, cfg->sigma_albedo, cfg->sigma_depth})
        if (!(s > 0.0f)) return "every guide sigma must be greater than 0 (+inf switches its term off)";
    if (!(cfg->variance_floor > 0.0f)) return "variance_floor must be greater than 0 (+inf switches the luminance term off)";
    if (cfg->reserved[0] | cfg->reserved[1]) return "reserved words must be 0";
    return nullptr;
}

DenoisePlan denoise_plan(const srt_denoise *cfg) {
    DenoisePlan p = {};
    p.vg = false; p.levels = cfg->levels; p.sigma_color = cfg->sigma_color;
    p.kn = cfg->sigma_normal * cfg->sigma_normal; p.ka = cfg->sigma_albedo * cfg->sigma_albedo; p.kz = cfg->sigma_depth * cfg->sigma_depth;
    return p;
}

DenoisePlan denoise_vg_plan(const srt_denoise_vg *cfg) {
    DenoisePlan p = {};
    p.vg = true; p.levels = cfg->levels; p.ks = cfg->sigma_variance * cfg->sigma_variance; p.floor = cfg->variance_floor;
    p.kn = cfg->sigma_normal * cfg->sigma_normal; p.ka = cfg->sigma_albedo * cfg->sigma_albedo; p.kz = cfg->sigma_depth * cfg->sigma_depth;
    return p;
}

// Prepass (its sources in `pre`; the outputs are set here), variance-guided: the estimator, plan.levels level kernels ping-ponging between
// the two colour images, the epilogue (variance-guided: and the variance after the last level): the row-major results are left in
// DenoiseLayout::out / var.  Enqueues on the default stream; the caller synchronises.
// Events: [0] prepass [1] (variance-guided: estimator [2]) level 0 .. epilogue: denoise_level_ev is the event level 0 starts at.
// sum_y2: the S2 words of a measured plan (indexed like pre.counts), else unused.
// ds (plain plans only; the caller has reserved d_despeckle): the firefly filter between the prepass and level 0, colour[1] =
// Despeckle(colour[0]), between its own events; one more denoise event behind it, so that level 0 is timed alone.
// ts (plain plans only; the caller has reserved d_temporal): the temporal stage behind that, colour[cur ^ 1] = Temporal(colour[cur]) on the
// context's history, between its own events and with one more denoise event behind it.  ts_out (with ts): the stage's outputs; the run
// stops behind the stage -- no level, no epilogue: srt_temporal_accum -- and records no denoise event, so the timing of the context's
// last denoise stays what it was.
// ts->tv (variance-guided plans; the caller has reserved d_temporal_var): the stage carries the moments, the spatial estimator runs behind
// it, on its output, and the choice kernel puts the temporal variance where it holds: prepass | (despeckle) | stage | estimator | choice |
// levels | epilogue.  denoise_est_ev is the event the estimator starts at.
int run_denoise(srt_ctx *c, const char *who, const DenoisePlan &plan, DenoisePrepassParams pre, const float *sum_y2 = nullptr, const srt_despeckle *ds = nullptr,
                TemporalStage *ts = nullptr, const TemporalParams *ts_out = nullptr) {
    const size_t pixels = (size_t)pre.w * pre.h;
    const DenoiseLayout L(c->d_denoise, pixels);
    pre.guides = L.guides; pre.colour = L.colour[0];
    const bool timed = !ts_out;
    if (timed) {
        c->denoise_timed = false;
        for (hipEvent_t &e : c->denoise_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    }
    uint32_t n_ev = 0;
    const auto mark = [&]() { return timed ? hipEventRecord(c->denoise_ev[n_ev++], nullptr) : hipSuccess; };
    HIP_TRY_AS(c, who, mark());
    HIP_TRY_AS(c, who, launch_denoise_prepass(pre, nullptr));
    HIP_TRY_AS(c, who, mark());
    if (plan.vg && plan.measured) {
        DenoiseMeasuredParams mp = {};
        mp.sum_y = pre.sums + pre.sum_comp_stride; mp.sum_y2 = sum_y2; mp.counts = pre.counts; mp.sum_pixel_stride = pre.sum_pixel_stride;
        mp.tx = pre.tx; mp.ty = pre.ty; mp.bx = pre.bx; mp.w = pre.w; mp.h = pre.h;
        mp.colour = reinterpret_cast<float *>(L.colour[0]); mp.out_var = L.var;
        HIP_TRY_AS(c, who, launch_denoise_measured(mp, nullptr));
        HIP_TRY_AS(c, who, mark());
    } else if (plan.vg && !(ts && ts->tv)) {
        DenoiseVarianceParams vp = {};
        vp.guides = L.guides; vp.colour = reinterpret_cast<float *>(L.colour[0]); vp.out_var = L.var;
        vp.w = pre.w; vp.h = pre.h; vp.kn = plan.kn; vp.ka = plan.ka; vp.kz = plan.kz;
        HIP_TRY_AS(c, who, launch_denoise_variance(vp, nullptr));
        HIP_TRY_AS(c, who, mark());
    }
    uint32_t cur = 0;
    if (ds) {
        DespeckleParams dp = {};
        dp.src4 = L.colour[0]; dp.dst4 = L.colour[1]; dp.w = pre.w; dp.h = pre.h;
        if (const int rc = run_despeckle(c, who, dp, ds)) return rc;
        HIP_TRY_AS(c, who, mark());
        cur = 1;
    }
    if (ts) {
        TemporalParams tp = ts_out ? *ts_out : TemporalParams{};
        tp.src4 = L.colour[cur]; tp.guides = L.guides; tp.dst4 = L.colour[cur ^ 1u]; tp.w = pre.w; tp.h = pre.h;
        if (ts->out_xyz) tp.out_xyz = TemporalLayout(c->d_temporal, pixels).img[0];
        if (ts->moving) {
            if (const int rc = run_motion_bound(c, who, pre.w, pre.h, c->last_offx, c->last_offy)) return rc;
            tp.prev_point = MotionLayout(c->d_motion, pixels).point;
        }
        if (const int rc = run_temporal_history(c, who, tp, ts->cfg, &ts->res, ts->tv != nullptr)) return rc;
        HIP_TRY_AS(c, who, mark());
        cur ^= 1u;
        if (ts_out) return SRT_OK;      // (the stage alone)
    }
    uint32_t est_ev = 1;
    if (ts && ts->tv) {      // the spatial estimate of the stage's output, then the choice between it and the moments' variance
        est_ev = n_ev - 1;
        DenoiseVarianceParams vp = {};
        vp.guides = L.guides; vp.colour = reinterpret_cast<float *>(L.colour[cur]); vp.out_var = L.var;
        vp.w = pre.w; vp.h = pre.h; vp.kn = plan.kn; vp.ka = plan.ka; vp.kz = plan.kz;
        HIP_TRY_AS(c, who, launch_denoise_variance(vp, nullptr));
        HIP_TRY_AS(c, who, mark());
        TemporalVarianceParams cp = {};
        cp.moments = TemporalMoments(c->d_temporal_mom, pixels).m[c->temporal_cur];
        cp.len = reinterpret_cast<const float *>(TemporalHistory(c->d_temporal_hist, pixels).colour[c->temporal_cur]) + 3; cp.len_stride = 4;
        cp.spatial = vp.colour + 3; cp.spatial_stride = 4; cp.colour_w = vp.colour + 3;
        cp.out_var = L.var; cp.out_stride = 2;
        cp.ml_min = (float)ts->tv->min_len; cp.n = (uint32_t)pixels;
        if (const int rc = run_temporal_variance(c, who, cp)) return rc;
        HIP_TRY_AS(c, who, mark());
    }
    const uint32_t level_ev = n_ev - 1;
    for (uint32_t i = 0; i < plan.levels; i++) {
        if (plan.vg) {
            DenoiseLevelVgParams lp = {};
            lp.guides = L.guides; lp.src = L.colour[cur]; lp.dst = L.colour[cur ^ 1u];
            lp.w = pre.w; lp.h = pre.h; lp.step = 1u << i;
            lp.kn = plan.kn; lp.ka = plan.ka; lp.kz = plan.kz; lp.ks = plan.ks; lp.floor = plan.floor;
            HIP_TRY_AS(c, who, launch_denoise_level_vg(lp, nullptr));
        } else {
            // the level's constants, fp32 on the host: sigma_color halves with every level (an exact scaling)
            const float sc = ldexpf(plan.sigma_color, -(int)i);
            DenoiseLevelParams lp = {};
            lp.guides = L.guides; lp.src = L.colour[cur]; lp.dst = L.colour[cur ^ 1u];
            lp.w = pre.w; lp.h = pre.h; lp.step = 1u << i;
            lp.kn = plan.kn; lp.ka = plan.ka; lp.kz = plan.kz; lp.kc = sc * sc;
            HIP_TRY_AS(c, who, launch_denoise_level(lp, nullptr));
        }
        HIP_TRY_AS(c, who, mark());
        cur ^= 1u;
    }
    HIP_TRY_AS(c, who, launch_denoise_epilogue(reinterpret_cast<const float *>(L.colour[cur]), L.out[0], L.out[1], L.out[2], pixels, nullptr));
    if (plan.vg) HIP_TRY_AS(c, who, launch_denoise_var_out(reinterpret_cast<const float *>(L.colour[cur]), L.var, pixels, nullptr));
    HIP_TRY_AS(c, who, mark());
    c->denoise_timed_levels = plan.levels; c->denoise_level_ev = level_ev; c->denoise_estimated = plan.vg; c->denoise_est_ev = est_ev; c->denoise_timed = true;
    return SRT_OK;
}

// srt_denoise_features / srt_denoise_features_vg behind their argument checks: host[0 .. 2] the three colour outputs, host[3] the variance
// what a denoise of the context's accumulation needs of it and of the partition; SRT_OK or the refusal
int denoise_accumulation_refusal(srt_ctx *c, const char *who, const DenoisePlan &plan) {
    const std::string w_(who);
    if (!c->accum.featured() || !c->accum.bound())
        return fail(c, SRT_ERR_INVALID, w_ + ": no featured accumulation with a pass (srt_accum_reset_features and srt_render_chunk_accum first)");
    if (plan.measured && (!c->accum.adaptive() || c->accum.total < 2))
        return fail(c, SRT_ERR_INVALID, w_ + ": needs an adaptive featured accumulation holding at least 2 samples (srt_accum_reset_adaptive_features; the "
                                             "measured variance of the mean needs S2 and two samples)");
    if (!whole_for(c, true, false))
        return fail(c, SRT_ERR_UNSUPPORTED, w_ + ": " + kNotWhole);
    return SRT_OK;
}

// run_denoise on the accumulation's w x h rectangle (not empty): the results are left in DenoiseLayout(c->d_denoise, w * h)
// ts / ts_out: run_denoise's (ts_out: the stage alone, its outputs in TemporalLayout(c->d_temporal, w * h), which the caller has reserved)
int denoise_accumulation(srt_ctx *c, const char *who, const DenoisePlan &plan, uint32_t w, uint32_t h, const srt_despeckle *ds = nullptr,
                         TemporalStage *ts = nullptr, const TemporalParams *ts_out = nullptr) {
    HIP_TRY(c, c->d_denoise.reserve(DenoiseLayout::bytes((size_t)w * h, plan.vg)));
    if (ds) if (const int rc = develop_reserve(c, who, c->d_despeckle, DespeckleLayout::kHeadBytes)) return rc;
    if (ts && !ts_out) if (const int rc = develop_reserve(c, who, c->d_temporal, ts->out_xyz ? TemporalLayout::bytes((size_t)w * h) : TemporalLayout::kHeadBytes)) return rc;
    if (ts && ts->tv) if (const int rc = develop_reserve(c, who, c->d_temporal_var, TemporalVarianceLayout::kHeadBytes)) return rc;
    DenoisePrepassParams pre = {};
    pre.sums = AccumLayout(c).sums; pre.sum_pixel_stride = 1; pre.sum_comp_stride = c->n_lanes;
    pre.rows = reinterpret_cast<const float4 *>(feature_rows(c));
    pre.tx = c->tx; pre.ty = c->ty; pre.bx = c->bx; pre.w = w; pre.h = h; pre.samples = c->accum.total;
    // (an adaptive featured accumulation: every pixel of the chunk is normalised by its own count, the samples field of its state word)
    if (c->accum.adaptive()) pre.counts = AdaptPlanes(c).state;
    return run_denoise(c, who, plan, pre, c->accum.adaptive() ? AdaptPlanes(c).sum2 : nullptr, ds, ts, ts_out);
}

int denoise_features(srt_ctx *c, const char *who, const DenoisePlan &plan, float *const host[4], uint32_t image_width, uint32_t image_height,
                     const srt_despeckle *ds = nullptr, TemporalStage *ts = nullptr) {
    if (const int rc = denoise_accumulation_refusal(c, who, plan)) return rc;
    HIP_TRY(c, set_device(c));
    // the filter runs on the chunk's rectangle (clipped to the reference grid); the image clips only what is copied out
    const uint32_t w = clipped_w(c), h = clipped_h(c);
    const size_t pixels = (size_t)w * h;
    if (pixels) {
        if (const int rc = denoise_accumulation(c, who, plan, w, h, ds, ts)) return rc;
        const ChunkRect rect = chunk_rect(c, image_width, image_height);
        const DenoiseLayout L(c->d_denoise, pixels);
        for (int k = 0; k < 4; k++) {
            const size_t ch = k < 3 ? 3 : 2;      // floats per pixel
            const float *src = k < 3 ? L.out[k] : L.var;
            const size_t row = (size_t)rect.w * ch * sizeof(float), src_pitch = (size_t)w * ch * sizeof(float), pitch = (size_t)image_width * ch * sizeof(float);
            if (host[k] && rect.w && rect.h) HIP_TRY(c, hipMemcpy2D(host[k] + rect.first * ch, pitch, src, src_pitch, row, rect.h, hipMemcpyDeviceToHost));
        }
        if (ts) if (const int rc = read_temporal_counts(c, who, &ts->res)) return rc;
        if (ts && ts->moving) if (const int rc = read_motion_counts(c, who, &ts->mres)) return rc;
        if (ts && ts->tv) if (const int rc = read_temporal_variance_count(c, who, &ts->n_temporal)) return rc;
    }
    HIP_TRY(c, device_synchronize(c));
    return SRT_OK;
}

// srt_denoise_kat / srt_denoise_vg_kat behind their configuration checks (out_var: variance-guided only)
// (a measured plan: sample_map[h][w] and sum_y2[h][w] in the place of the scalar `samples`, which is not read)
int denoise_kat(srt_ctx *c, const char *who, const DenoisePlan &plan, const float *xyz_sums, const float *features, uint32_t samples, uint32_t w, uint32_t h,
                float *out_xyz, float *out_var, const uint32_t *sample_map = nullptr, const float *sum_y2 = nullptr) {
    if (samples == 0 || w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, std::string(who) + ": samples, w and h must be positive, w x h below 2^31");
    const size_t pixels = (size_t)w * h;
    if (sample_map)
        for (size_t k = 0; k < pixels; k++)
            if ((sample_map[k] & ~kAdaptConverged) == 0) return fail(c, SRT_ERR_INVALID, std::string(who) + ": a zero in samples (every pixel must hold at least one sample)");
    HIP_TRY(c, set_device(c));
    HIP_TRY_AS(c, who, c->d_denoise.reserve(DenoiseLayout::bytes(pixels, plan.vg)));
    HIP_TRY_AS(c, who, c->d_denoise_in.reserve(pixels * (kFeatureStride + 3 + 2) * sizeof(float)));
    float *d_rows = c->d_denoise_in.as<float>(), *d_sums = d_rows + pixels * kFeatureStride, *d_map = d_sums + pixels * 3, *d_s2 = d_map + pixels;
    HIP_TRY_AS(c, who, hipMemcpy(d_rows, features, pixels * kFeatureStride * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, who, hipMemcpy(d_sums, xyz_sums, pixels * 3 * sizeof(float), hipMemcpyHostToDevice));
    if (sample_map) {
        HIP_TRY_AS(c, who, hipMemcpy(d_map, sample_map, pixels * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY_AS(c, who, hipMemcpy(d_s2, sum_y2, pixels * sizeof(float), hipMemcpyHostToDevice));
    }
    // a grid of one w x h block makes the prepass's block-linear lane the row-major pixel
    DenoisePrepassParams pre = {};
    pre.sums = d_sums; pre.sum_pixel_stride = 3; pre.sum_comp_stride = 1;
    pre.rows = reinterpret_cast<const float4 *>(d_rows);
    pre.tx = w; pre.ty = h; pre.bx = 1; pre.w = w; pre.h = h; pre.samples = samples;
    if (sample_map) pre.counts = reinterpret_cast<const uint32_t *>(d_map);
    if (const int rc = run_denoise(c, who, plan, pre, sample_map ? d_s2 : nullptr)) return rc;
    const DenoiseLayout L(c->d_denoise, pixels);
    HIP_TRY_AS(c, who, hipMemcpy(out_xyz, L.out[0], pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_var) HIP_TRY_AS(c, who, hipMemcpy(out_var, L.var, pixels * 2 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY_AS(c, who, device_synchronize(c));
    return SRT_OK;
}

}  // namespace

int srt_denoise_features(srt_ctx *c, const srt_denoise *cfg, float *out_xyz, float *out_lin, float *out_q, uint32_t image_width, uint32_t image_height) {
    if (!c || !cfg) return fail(c, SRT_ERR_INVALID, "srt_denoise_features: null argument");
    if ((!out_xyz && !out_lin && !out_q) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_denoise_features: no output / empty image");
    if (const char *why = denoise_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_features: ") + why);
    float *const host[4] = {out_xyz, out_lin, out_q, nullptr};
    return denoise_features(c, "srt_denoise_features", denoise_plan(cfg), host, image_width, image_height);
}

int srt_denoise_features_ds(srt_ctx *c, const srt_despeckle *despeckle_cfg, const srt_denoise *denoise_cfg, float *out_xyz, float *out_lin, float *out_q,
                            uint32_t image_width, uint32_t image_height) {
    if (!c || !despeckle_cfg || !denoise_cfg) return fail(c, SRT_ERR_INVALID, "srt_denoise_features_ds: null argument");
    if ((!out_xyz && !out_lin && !out_q) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_denoise_features_ds: no output / empty image");
    if (const char *why = denoise_cfg_error(denoise_cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_features_ds: ") + why);
    if (const char *why = despeckle_cfg_error(despeckle_cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_features_ds: ") + why);
    float *const host[4] = {out_xyz, out_lin, out_q, nullptr};
    return denoise_features(c, "srt_denoise_features_ds", denoise_plan(denoise_cfg), host, image_width, image_height, despeckle_cfg);
}

static int denoise_features_temporal(srt_ctx *c, const char *who, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg, const srt_denoise *denoise_cfg,
                                     float *out_xyz, float *out_lin, float *out_q, srt_temporal_result *temporal_result, uint32_t image_width, uint32_t image_height,
                                     bool moving, srt_motion_result *motion_result) {
    const std::string w_(std::string(who) + ": ");
    if (!c || !temporal_cfg || !denoise_cfg) return fail(c, SRT_ERR_INVALID, w_ + "null argument");
    if ((!out_xyz && !out_lin && !out_q) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, w_ + "no output / empty image");
    if (const char *why = denoise_cfg_error(denoise_cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (despeckle_cfg) if (const char *why = despeckle_cfg_error(despeckle_cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (const char *why = temporal_cfg_error(temporal_cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (moving) if (const char *why = motion_bound_refusal(c)) return fail(c, SRT_ERR_INVALID, w_ + why);
    float *const host[4] = {out_xyz, out_lin, out_q, nullptr};
    TemporalStage ts = {temporal_cfg, false, {}};
    ts.moving = moving;
    if (const int rc = denoise_features(c, who, denoise_plan(denoise_cfg), host, image_width, image_height, despeckle_cfg, &ts)) return rc;
    if (temporal_result) *temporal_result = ts.res;
    if (motion_result) *motion_result = ts.mres;
    return SRT_OK;
}

int srt_denoise_features_temporal(srt_ctx *c, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg, const srt_denoise *denoise_cfg, float *out_xyz,
                                  float *out_lin, float *out_q, srt_temporal_result *temporal_result, uint32_t image_width, uint32_t image_height) {
    return denoise_features_temporal(c, "srt_denoise_features_temporal", temporal_cfg, despeckle_cfg, denoise_cfg, out_xyz, out_lin, out_q, temporal_result, image_width,
                                     image_height, false, nullptr);
}

int srt_denoise_features_temporal_moving(srt_ctx *c, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg, const srt_denoise *denoise_cfg, float *out_xyz,
                                         float *out_lin, float *out_q, srt_temporal_result *temporal_result, uint32_t image_width, uint32_t image_height,
                                         srt_motion_result *motion_result) {
    return denoise_features_temporal(c, "srt_denoise_features_temporal_moving", temporal_cfg, despeckle_cfg, denoise_cfg, out_xyz, out_lin, out_q, temporal_result,
                                     image_width, image_height, true, motion_result);
}

int srt_denoise_features_temporal_vg(srt_ctx *c, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg, const srt_denoise_vg *vg_cfg,
                                     const srt_temporal_vg *tv_cfg, float *out_xyz, float *out_lin, float *out_q, float *out_var, srt_temporal_result *temporal_result,
                                     uint64_t *n_temporal, srt_motion_result *motion_result, uint32_t image_width, uint32_t image_height) {
    const char *who = "srt_denoise_features_temporal_vg";
    const std::string w_(std::string(who) + ": ");
    if (!c || !temporal_cfg || !vg_cfg || !tv_cfg) return fail(c, SRT_ERR_INVALID, w_ + "null argument");
    if ((!out_xyz && !out_lin && !out_q && !out_var) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, w_ + "no output / empty image");
    if (const char *why = denoise_vg_cfg_error(vg_cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (despeckle_cfg) if (const char *why = despeckle_cfg_error(despeckle_cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (const char *why = temporal_cfg_error(temporal_cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (const char *why = temporal_vg_cfg_error(tv_cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (tv_cfg->moving) if (const char *why = motion_bound_refusal(c)) return fail(c, SRT_ERR_INVALID, w_ + why);
    float *const host[4] = {out_xyz, out_lin, out_q, out_var};
    TemporalStage ts = {temporal_cfg, false, {}};
    ts.moving = tv_cfg->moving != 0; ts.tv = tv_cfg;
    if (const int rc = denoise_features(c, who, denoise_vg_plan(vg_cfg), host, image_width, image_height, despeckle_cfg, &ts)) return rc;
    if (temporal_result) *temporal_result = ts.res;
    if (n_temporal) *n_temporal = ts.n_temporal;
    if (motion_result) *motion_result = ts.mres;
    return SRT_OK;
}

static int temporal_accum(srt_ctx *c, const char *who, const srt_temporal *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_len, float *out_motion,
                          srt_temporal_result *result, uint32_t image_width, uint32_t image_height, bool moving, srt_motion_result *motion_result) {
    const std::string w_(std::string(who) + ": ");
    if (!c || !cfg) return fail(c, SRT_ERR_INVALID, w_ + "null argument");
    if ((!out_xyz && !out_lin && !out_q && !out_len && !out_motion && !result) || image_width == 0 || image_height == 0)
        return fail(c, SRT_ERR_INVALID, w_ + "no output / empty image");
    if (const char *why = temporal_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
    const DenoisePlan plan = {};      // (the prepass alone: no level runs)
    if (const int rc = denoise_accumulation_refusal(c, who, plan)) return rc;
    if (moving) if (const char *why = motion_bound_refusal(c)) return fail(c, SRT_ERR_INVALID, w_ + why);
    HIP_TRY(c, set_device(c));
    // the stage runs on the chunk's rectangle (clipped to the reference grid); the image clips only what is copied out
    const uint32_t w = clipped_w(c), h = clipped_h(c);
    const size_t pixels = (size_t)w * h;
    TemporalStage ts = {cfg, false, {}};
    ts.moving = moving;
    if (pixels) {
        if (const int rc = develop_reserve(c, who, c->d_temporal, TemporalLayout::bytes(pixels))) return rc;
        const TemporalLayout L(c->d_temporal, pixels);
        TemporalParams out = {};
        out.out_xyz = out_xyz ? L.img[0] : nullptr; out.out_lin = out_lin ? L.img[1] : nullptr; out.out_q = out_q ? L.img[2] : nullptr;
        out.out_len = out_len ? L.len : nullptr; out.out_motion = out_motion ? L.motion : nullptr;
        if (const int rc = denoise_accumulation(c, who, plan, w, h, nullptr, &ts, &out)) return rc;
        const ChunkRect rect = chunk_rect(c, image_width, image_height);
        float *const host[5] = {out_xyz, out_lin, out_q, out_len, out_motion};
        const float *const src[5] = {L.img[0], L.img[1], L.img[2], L.len, L.motion};
        const size_t chans[5] = {3, 3, 3, 1, 2};      // floats per pixel
        for (int k = 0; k < 5; k++) {
            const size_t ch = chans[k];
            const size_t row = (size_t)rect.w * ch * sizeof(float), src_pitch = (size_t)w * ch * sizeof(float), pitch = (size_t)image_width * ch * sizeof(float);
            if (host[k] && rect.w && rect.h) HIP_TRY(c, hipMemcpy2D(host[k] + rect.first * ch, pitch, src[k], src_pitch, row, rect.h, hipMemcpyDeviceToHost));
        }
        if (const int rc = read_temporal_counts(c, who, &ts.res)) return rc;
        if (moving) if (const int rc = read_motion_counts(c, who, &ts.mres)) return rc;
    }
    HIP_TRY(c, device_synchronize(c));
    if (result) *result = ts.res;
    if (motion_result) *motion_result = ts.mres;
    return SRT_OK;
}

int srt_temporal_accum(srt_ctx *c, const srt_temporal *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_len, float *out_motion,
                       srt_temporal_result *result, uint32_t image_width, uint32_t image_height) {
    return temporal_accum(c, "srt_temporal_accum", cfg, out_xyz, out_lin, out_q, out_len, out_motion, result, image_width, image_height, false, nullptr);
}

int srt_temporal_accum_moving(srt_ctx *c, const srt_temporal *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_len, float *out_motion,
                              srt_temporal_result *result, uint32_t image_width, uint32_t image_height, srt_motion_result *motion_result) {
    return temporal_accum(c, "srt_temporal_accum_moving", cfg, out_xyz, out_lin, out_q, out_len, out_motion, result, image_width, image_height, true, motion_result);
}

int srt_denoise_features_vg(srt_ctx *c, const srt_denoise_vg *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_var, uint32_t image_width, uint32_t image_height) {
    if (!c || !cfg) return fail(c, SRT_ERR_INVALID, "srt_denoise_features_vg: null argument");
    if ((!out_xyz && !out_lin && !out_q && !out_var) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_denoise_features_vg: no output / empty image");
    if (const char *why = denoise_vg_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_features_vg: ") + why);
    float *const host[4] = {out_xyz, out_lin, out_q, out_var};
    return denoise_features(c, "srt_denoise_features_vg", denoise_vg_plan(cfg), host, image_width, image_height);
}

int srt_denoise_kat(srt_ctx *c, const srt_denoise *cfg, const float *xyz_sums, const float *features, uint32_t samples, uint32_t w, uint32_t h, float *out_xyz) {
    if (!c || !cfg || !xyz_sums || !features || !out_xyz) return fail(c, SRT_ERR_INVALID, "srt_denoise_kat: null argument");
    if (const char *why = denoise_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_kat: ") + why);
    return denoise_kat(c, "srt_denoise_kat", denoise_plan(cfg), xyz_sums, features, samples, w, h, out_xyz, nullptr);
}

int srt_denoise_vg_kat(srt_ctx *c, const srt_denoise_vg *cfg, const float *xyz_sums, const float *features, uint32_t samples, uint32_t w, uint32_t h,
                       float *out_xyz, float *out_var) {
    if (!c || !cfg || !xyz_sums || !features || !out_xyz || !out_var) return fail(c, SRT_ERR_INVALID, "srt_denoise_vg_kat: null argument");
    if (const char *why = denoise_vg_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_vg_kat: ") + why);
    return denoise_kat(c, "srt_denoise_vg_kat", denoise_vg_plan(cfg), xyz_sums, features, samples, w, h, out_xyz, out_var);
}

int srt_denoise_features_mv(srt_ctx *c, const srt_denoise_vg *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_var, uint32_t image_width, uint32_t image_height) {
    if (!c || !cfg) return fail(c, SRT_ERR_INVALID, "srt_denoise_features_mv: null argument");
    if ((!out_xyz && !out_lin && !out_q && !out_var) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_denoise_features_mv: no output / empty image");
    if (const char *why = denoise_vg_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_features_mv: ") + why);
    float *const host[4] = {out_xyz, out_lin, out_q, out_var};
    DenoisePlan plan = denoise_vg_plan(cfg);
    plan.measured = true;
    return denoise_features(c, "srt_denoise_features_mv", plan, host, image_width, image_height);
}

int srt_denoise_mv_kat(srt_ctx *c, const srt_denoise_vg *cfg, const float *xyz_sums, const float *features, const uint32_t *samples, const float *sum_y2,
                       uint32_t w, uint32_t h, float *out_xyz, float *out_var) {
    if (!c || !cfg || !xyz_sums || !features || !samples || !sum_y2 || !out_xyz || !out_var) return fail(c, SRT_ERR_INVALID, "srt_denoise_mv_kat: null argument");
    if (const char *why = denoise_vg_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_mv_kat: ") + why);
    DenoisePlan plan = denoise_vg_plan(cfg);
    plan.measured = true;
    return denoise_kat(c, "srt_denoise_mv_kat", plan, xyz_sums, features, 1u, w, h, out_xyz, out_var, samples, sum_y2);
}

// ---- the developed payload (srt_denoise_developed) ------------------------------------------------------------------------------
namespace {

// d_denoise_dev: [payload A | payload B: `groups` float4 per pixel each, [group][pixel] | out_dev: `channels` floats per pixel
//                 | srt_denoise_developed_kat only: the caller's developed planes, `channels` floats per pixel]
struct DenoiseDevLayout {
    float4 *payload[2];
    float *out, *in;
    static size_t bytes(size_t pixels, uint32_t channels, bool kat) {
        return pixels * (2 * (size_t)denoise_payload_groups(channels) * sizeof(float4) + (size_t)channels * (kat ? 2u : 1u) * sizeof(float));
    }
    DenoiseDevLayout(const DeviceBuffer &d, size_t pixels, uint32_t channels) {
        const size_t g = denoise_payload_groups(channels);
        payload[0] = d.as<float4>(); payload[1] = payload[0] + g * pixels;
        out = reinterpret_cast<float *>(payload[1] + g * pixels); in = out + pixels * channels;      // (in: inside the buffer only when reserved with kat)
    }
};

// run_denoise's plain branch with the payload riding along: the prepass and the payload's prepass (developed: [pixel][channels] on the
// device), plan.levels payload levels ping-ponging colour and payload, the epilogue and the payload's output kernel.  The results are
// left in DenoiseLayout::out[0] and DenoiseDevLayout::out; d_denoise and d_denoise_dev are reserved by the caller.  Events as in
// run_denoise: [0] both prepasses [1] level 0 .. both output kernels.
int run_denoise_developed(srt_ctx *c, const char *who, const DenoisePlan &plan, DenoisePrepassParams pre, const float *developed, uint32_t channels) {
    const size_t pixels = (size_t)pre.w * pre.h;
    const uint32_t groups = denoise_payload_groups(channels);
    const DenoiseLayout L(c->d_denoise, pixels);
    const DenoiseDevLayout D(c->d_denoise_dev, pixels, channels);
    pre.guides = L.guides; pre.colour = L.colour[0];
    c->denoise_timed = false;
    for (hipEvent_t &e : c->denoise_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    uint32_t n_ev = 0;
    HIP_TRY_AS(c, who, hipEventRecord(c->denoise_ev[n_ev++], nullptr));
    HIP_TRY_AS(c, who, launch_denoise_prepass(pre, nullptr));
    if (pre.counts) {      // (pixels with different sample counts: both prepasses use the pixel's own)
        DenoisePayloadPrepassCountsParams pp = {};
        pp.developed = developed; pp.payload = D.payload[0]; pp.counts = pre.counts; pp.tx = pre.tx; pp.ty = pre.ty; pp.bx = pre.bx;
        pp.w = pre.w; pp.h = pre.h; pp.channels = channels; pp.groups = groups;
        HIP_TRY_AS(c, who, launch_denoise_payload_prepass_counts(pp, nullptr));
    } else {
        DenoisePayloadPrepassParams pp = {};
        pp.developed = developed; pp.payload = D.payload[0]; pp.pixels = pixels; pp.channels = channels; pp.groups = groups; pp.samples = pre.samples;
        HIP_TRY_AS(c, who, launch_denoise_payload_prepass(pp, nullptr));
    }
    HIP_TRY_AS(c, who, hipEventRecord(c->denoise_ev[n_ev++], nullptr));
    const uint32_t level_ev = n_ev - 1;
    uint32_t cur = 0;
    for (uint32_t i = 0; i < plan.levels; i++) {
        const float sc = ldexpf(plan.sigma_color, -(int)i);      // (as in run_denoise)
        DenoiseLevelDevParams lp = {};
        lp.guides = L.guides; lp.src = L.colour[cur]; lp.dst = L.colour[cur ^ 1u];
        lp.psrc = D.payload[cur]; lp.pdst = D.payload[cur ^ 1u]; lp.groups = groups;
        lp.w = pre.w; lp.h = pre.h; lp.step = 1u << i;
        lp.kn = plan.kn; lp.ka = plan.ka; lp.kz = plan.kz; lp.kc = sc * sc;
        HIP_TRY_AS(c, who, launch_denoise_level_dev(lp, nullptr));
        HIP_TRY_AS(c, who, hipEventRecord(c->denoise_ev[n_ev++], nullptr));
        cur ^= 1u;
    }
    HIP_TRY_AS(c, who, launch_denoise_epilogue(reinterpret_cast<const float *>(L.colour[cur]), L.out[0], L.out[1], L.out[2], pixels, nullptr));
    HIP_TRY_AS(c, who, launch_denoise_dev_out(D.payload[cur], D.out, channels, groups, pixels, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->denoise_ev[n_ev++], nullptr));
    c->denoise_timed_levels = plan.levels; c->denoise_level_ev = level_ev; c->denoise_estimated = false; c->denoise_est_ev = 1; c->denoise_timed = true;
    return SRT_OK;
}

}  // namespace

int srt_denoise_developed(srt_ctx *c, const srt_denoise *cfg, const float *response, uint32_t channels, float scale, float *out_dev, float *out_xyz,
                          uint32_t image_width, uint32_t image_height) {
    const char *who = "srt_denoise_developed";
    if (!c || !cfg || !response) return fail(c, SRT_ERR_INVALID, "srt_denoise_developed: null argument");
    if ((!out_dev && !out_xyz) || image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, "srt_denoise_developed: no output / empty image");
    if (const char *why = denoise_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_developed: ") + why);
    if (const char *why = develop_args_error(response, channels, scale)) return fail(c, SRT_ERR_INVALID, std::string("srt_denoise_developed: ") + why);
    if (!c->accum.spectral() || !c->accum.featured() || !c->accum.bound())
        return fail(c, SRT_ERR_INVALID, "srt_denoise_developed: no spectral featured accumulation with a pass (srt_accum_reset_spectral_features or "
                                        "srt_accum_reset_adaptive_spectral_features, and srt_render_chunk_accum first)");
    if (!whole_for(c, true, true))
        return fail(c, SRT_ERR_UNSUPPORTED, std::string("srt_denoise_developed: ") + kNotWhole);
    HIP_TRY(c, set_device(c));
    // develop and filter run on the chunk's rectangle (clipped to the reference grid); the image clips only what is copied out
    const uint32_t w = clipped_w(c), h = clipped_h(c);
    const size_t pixels = (size_t)w * h;
    if (pixels) {
        if (const int rc = develop_reserve(c, who, c->d_develop, DevelopLayout::bytes(pixels, channels, false))) return rc;
        if (const int rc = develop_reserve(c, who, c->d_denoise, DenoiseLayout::bytes(pixels, false))) return rc;
        if (const int rc = develop_reserve(c, who, c->d_denoise_dev, DenoiseDevLayout::bytes(pixels, channels, false))) return rc;
        if (const int rc = run_develop(c, who, c->d_film.as<float>(), c->n_lanes, c->tx, c->ty, c->bx, w, h, response, channels, scale, 0u)) return rc;
        DenoisePrepassParams pre = {};
        pre.sums = AccumLayout(c).sums; pre.sum_pixel_stride = 1; pre.sum_comp_stride = c->n_lanes;
        pre.rows = reinterpret_cast<const float4 *>(feature_rows(c));
        pre.tx = c->tx; pre.ty = c->ty; pre.bx = c->bx; pre.w = w; pre.h = h; pre.samples = c->accum.total;
        // (an adaptive spectral featured accumulation: colour, guides and payload of a pixel are normalised by the pixel's own count)
        if (c->accum.adaptive()) pre.counts = AdaptPlanes(c).state;
        if (const int rc = run_denoise_developed(c, who, denoise_plan(cfg), pre, DevelopLayout(c->d_develop, pixels, channels).out, channels)) return rc;
        const ChunkRect rect = chunk_rect(c, image_width, image_height);
        const float *src[2] = {DenoiseDevLayout(c->d_denoise_dev, pixels, channels).out, DenoiseLayout(c->d_denoise, pixels).out[0]};
        float *const host[2] = {out_dev, out_xyz};
        for (int k = 0; k < 2; k++) {
            const size_t ch = k == 0 ? channels : 3;      // floats per pixel
            const size_t row = (size_t)rect.w * ch * sizeof(float), src_pitch = (size_t)w * ch * sizeof(float), pitch = (size_t)image_width * ch * sizeof(float);
            if (host[k] && rect.w && rect.h) HIP_TRY(c, hipMemcpy2D(host[k] + rect.first * ch, pitch, src[k], src_pitch, row, rect.h, hipMemcpyDeviceToHost));
        }
    }
    HIP_TRY(c, device_synchronize(c));
    return SRT_OK;
}

// srt_denoise_developed_kat / srt_denoise_developed_counts_kat behind their own null checks (sample_map: the second's [h][w] counts in the
// place of the scalar `samples`, which is not read then)
static int denoise_developed_kat(srt_ctx *c, const char *who, const srt_denoise *cfg, const float *xyz_sums, const float *features, const float *developed,
                                 uint32_t channels, uint32_t samples, const uint32_t *sample_map, uint32_t w, uint32_t h, float *out_dev, float *out_xyz) {
    const std::string w_(who);
    if (const char *why = denoise_cfg_error(cfg)) return fail(c, SRT_ERR_INVALID, w_ + ": " + why);
    if (channels == 0 || channels > kMaxDevelopChannels) return fail(c, SRT_ERR_INVALID, w_ + ": channels must be in 1 .. SRT_MAX_DEVELOP_CHANNELS (16)");
    if (samples == 0 || w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, w_ + ": samples, w and h must be positive, w x h below 2^31");
    const size_t pixels = (size_t)w * h;
    if (sample_map)
        for (size_t k = 0; k < pixels; k++)
            if ((sample_map[k] & ~kAdaptConverged) == 0) return fail(c, SRT_ERR_INVALID, w_ + ": a zero in samples (every pixel must hold at least one sample)");
    HIP_TRY(c, set_device(c));
    if (const int rc = develop_reserve(c, who, c->d_denoise, DenoiseLayout::bytes(pixels, false))) return rc;
    if (const int rc = develop_reserve(c, who, c->d_denoise_dev, DenoiseDevLayout::bytes(pixels, channels, true))) return rc;
    if (const int rc = develop_reserve(c, who, c->d_denoise_in, pixels * (kFeatureStride + 3 + 1) * sizeof(float))) return rc;
    const DenoiseDevLayout D(c->d_denoise_dev, pixels, channels);
    float *d_rows = c->d_denoise_in.as<float>(), *d_sums = d_rows + pixels * kFeatureStride, *d_map = d_sums + pixels * 3;
    HIP_TRY_AS(c, who, hipMemcpy(d_rows, features, pixels * kFeatureStride * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, who, hipMemcpy(d_sums, xyz_sums, pixels * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, who, hipMemcpy(D.in, developed, pixels * channels * sizeof(float), hipMemcpyHostToDevice));
    if (sample_map) HIP_TRY_AS(c, who, hipMemcpy(d_map, sample_map, pixels * sizeof(uint32_t), hipMemcpyHostToDevice));
    // a grid of one w x h block makes the prepass's block-linear lane the row-major pixel
    DenoisePrepassParams pre = {};
    pre.sums = d_sums; pre.sum_pixel_stride = 3; pre.sum_comp_stride = 1;
    pre.rows = reinterpret_cast<const float4 *>(d_rows);
    pre.tx = w; pre.ty = h; pre.bx = 1; pre.w = w; pre.h = h; pre.samples = samples;
    if (sample_map) pre.counts = reinterpret_cast<const uint32_t *>(d_map);
    if (const int rc = run_denoise_developed(c, who, denoise_plan(cfg), pre, D.in, channels)) return rc;
    if (out_dev) HIP_TRY_AS(c, who, hipMemcpy(out_dev, D.out, pixels * channels * sizeof(float), hipMemcpyDeviceToHost));
    if (out_xyz) HIP_TRY_AS(c, who, hipMemcpy(out_xyz, DenoiseLayout(c->d_denoise, pixels).out[0], pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY_AS(c, who, device_synchronize(c));
    return SRT_OK;
}

int srt_denoise_developed_kat(srt_ctx *c, const srt_denoise *cfg, const float *xyz_sums, const float *features, const float *developed, uint32_t channels,
                              uint32_t samples, uint32_t w, uint32_t h, float *out_dev, float *out_xyz) {
    if (!c || !cfg || !xyz_sums || !features || !developed || (!out_dev && !out_xyz)) return fail(c, SRT_ERR_INVALID, "srt_denoise_developed_kat: null argument");
    return denoise_developed_kat(c, "srt_denoise_developed_kat", cfg, xyz_sums, features, developed, channels, samples, nullptr, w, h, out_dev, out_xyz);
}

int srt_denoise_developed_counts_kat(srt_ctx *c, const srt_denoise *cfg, const float *xyz_sums, const float *features, const float *developed, uint32_t channels,
                                     const uint32_t *samples, uint32_t w, uint32_t h, float *out_dev, float *out_xyz) {
    if (!c || !cfg || !xyz_sums || !features || !developed || !samples || (!out_dev && !out_xyz))
        return fail(c, SRT_ERR_INVALID, "srt_denoise_developed_counts_kat: null argument");
    return denoise_developed_kat(c, "srt_denoise_developed_counts_kat", cfg, xyz_sums, features, developed, channels, 1u, samples, w, h, out_dev, out_xyz);
}

int srt_denoise_last_ms(srt_ctx *c, float *prepass_ms, float *level_ms, float *epilogue_ms, uint32_t *levels) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_denoise_last_ms: null ctx");
    if (!c->denoise_timed) return fail(c, SRT_ERR_INVALID, "srt_denoise_last_ms: no denoise has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n = c->denoise_timed_levels, l0 = c->denoise_level_ev;
    HIP_TRY(c, hipEventSynchronize(c->denoise_ev[l0 + n + 1]));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->denoise_ev[0], c->denoise_ev[1]));
    if (prepass_ms) *prepass_ms = ms;
    for (uint32_t i = 0; i < 8; i++) {
        ms = 0.0f;
        if (i < n) HIP_TRY(c, hipEventElapsedTime(&ms, c->denoise_ev[l0 + i], c->denoise_ev[l0 + 1 + i]));
        if (level_ms) level_ms[i] = ms;
    }
    HIP_TRY(c, hipEventElapsedTime(&ms, c->denoise_ev[l0 + n], c->denoise_ev[l0 + n + 1]));
    if (epilogue_ms) *epilogue_ms = ms;
    if (levels) *levels = n;
    return SRT_OK;
}

int srt_denoise_estimate_last_ms(srt_ctx *c, float *ms) {
    if (!c || !ms) return fail(c, SRT_ERR_INVALID, "srt_denoise_estimate_last_ms: null argument");
    if (!c->denoise_timed || !c->denoise_estimated) return fail(c, SRT_ERR_INVALID, "srt_denoise_estimate_last_ms: the context's last denoise was not variance-guided");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->denoise_ev[c->denoise_est_ev + 1]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->denoise_ev[c->denoise_est_ev], c->denoise_ev[c->denoise_est_ev + 1]));
    return SRT_OK;
}

// ---- the presented picture (srt_present.hip) -------------------------------------------------------------------------------------
namespace {

// d_present: [the packed picture: one word per pixel, padded to 16 bytes | a developed source only: its XYZ mean, three floats per pixel]
struct PresentLayout {
    uint32_t *rgba;
    float *mean;
    static size_t rgba_bytes(size_t pixels) { return (pixels * sizeof(uint32_t) + 15) & ~(size_t)15; }
    static size_t bytes(size_t pixels, bool mean) { return rgba_bytes(pixels) + (mean ? 3 * pixels * sizeof(float) : 0); }
    PresentLayout(const DeviceBuffer &d, size_t pixels) : rgba(d.as<uint32_t>()), mean(reinterpret_cast<float *>(d.as<char>() + rgba_bytes(pixels))) {}
};

// The present kernel over the w x h rectangle described by p (curve, gain, output and counters are filled in here) into PresentLayout::rgba;
// then rows [0, copy_h) x columns [0, copy_w) of it and the three counters through the pinned staging block, one synchronise, and the rows
// into the caller's buffer at `pitch` bytes per row.  d_present and d_expose are reserved by the caller.
int run_present(srt_ctx *c, const char *who, PresentParams p, const srt_tone *tone, float gain, uint32_t copy_w, uint32_t copy_h, uint8_t *out, size_t pitch,
                srt_tone_result *result) {
    const size_t pixels = (size_t)p.w * p.h, row = (size_t)copy_w * sizeof(uint32_t), image = (row * copy_h + 7) & ~(size_t)7;
    if (const hipError_t e = c->h_present.reserve(image + 3 * sizeof(unsigned long long))) {
        (void)hipGetLastError();
        return hip_fail(c, e, who);
    }
    const ExposeLayout L(c->d_expose);
    const PresentLayout I(c->d_present, pixels);
    c->present_timed = false;
    for (hipEvent_t &e : c->present_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    HIP_TRY_AS(c, who, hipMemsetAsync(L.tone_counts, 0, 3 * sizeof(unsigned long long), nullptr));
    p.curve = tone->curve; p.gain = gain; p.kw = tone->white * tone->white;
    p.out = I.rgba; p.counts = L.tone_counts;
    HIP_TRY_AS(c, who, hipEventRecord(c->present_ev[0], nullptr));
    HIP_TRY_AS(c, who, launch_present(p, (uint32_t)c->n_cu, !c->present_scalar, nullptr));
    HIP_TRY_AS(c, who, hipEventRecord(c->present_ev[1], nullptr));
    c->present_timed = true;
    char *stage = static_cast<char *>(c->h_present.ptr);
    if (copy_w && copy_h) {
        if (copy_w == p.w) HIP_TRY_AS(c, who, hipMemcpyAsync(stage, I.rgba, row * copy_h, hipMemcpyDeviceToHost, nullptr));
        else HIP_TRY_AS(c, who, hipMemcpy2DAsync(stage, row, I.rgba, (size_t)p.w * sizeof(uint32_t), row, copy_h, hipMemcpyDeviceToHost, nullptr));
    }
    HIP_TRY_AS(c, who, hipMemcpyAsync(stage + image, L.tone_counts, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY_AS(c, who, hipStreamSynchronize(nullptr));
    for (uint32_t j = 0; j < copy_h && copy_w; j++) memcpy(out + j * pitch, stage + j * row, row);
    unsigned long long counts[3];
    memcpy(counts, stage + image, sizeof(counts));
    result->blown = counts[0]; result->crushed = counts[1]; result->nonfinite = counts[2];
    return SRT_OK;
}

}  // namespace

namespace {

// srt_present (ds == null) and srt_present_despeckled (ds: the firefly filter in front of the chain; ds_result may be null);
// srt_present_temporal (tcfg: the temporal stage in front of the chain, behind the firefly filter when there is one; ts_result may be null)
int present_chain(srt_ctx *c, const char *who, const srt_present_cfg *cfg, const srt_despeckle *ds, uint8_t *out_rgba8, size_t pitch_bytes, uint32_t image_width,
                  uint32_t image_height, srt_present_result *result, srt_despeckle_result *ds_result, const srt_temporal *tcfg = nullptr,
                  srt_temporal_result *ts_result = nullptr, bool moving = false, srt_motion_result *mo_result = nullptr, const srt_temporal_vg *tv = nullptr,
                  uint64_t *n_temporal = nullptr) {
    const std::string w_(std::string(who) + ": ");
    if (!c || !cfg || !out_rgba8) return fail(c, SRT_ERR_INVALID, w_ + "null argument");
    for (const uint32_t r : cfg->reserved) if (r) return fail(c, SRT_ERR_INVALID, w_ + "the reserved words must be 0");
    if (cfg->source > SRT_PRESENT_DEVELOP) return fail(c, SRT_ERR_INVALID, w_ + "unknown source (SRT_PRESENT_ACCUM .. SRT_PRESENT_DEVELOP)");
    if (image_width == 0 || image_height == 0) return fail(c, SRT_ERR_INVALID, w_ + "empty image");
    if (pitch_bytes < (size_t)image_width * 4) return fail(c, SRT_ERR_INVALID, w_ + "pitch_bytes must be at least 4 * image_width");
    if (const char *why = tone_cfg_error(&cfg->tone)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (cfg->metered) if (const char *why = meter_cfg_error(&cfg->meter)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (ds) {
        if (const char *why = despeckle_cfg_error(ds)) return fail(c, SRT_ERR_INVALID, w_ + why);
        if (cfg->source != SRT_PRESENT_ACCUM && cfg->source != SRT_PRESENT_DENOISE && !(tv && cfg->source == SRT_PRESENT_DENOISE_VG))
            return fail(c, SRT_ERR_UNSUPPORTED, w_ + "the despeckled sources are SRT_PRESENT_ACCUM and SRT_PRESENT_DENOISE");
    }
    if (tcfg) {
        if (const char *why = temporal_cfg_error(tcfg)) return fail(c, SRT_ERR_INVALID, w_ + why);
        if (tv) {      // srt_present_temporal_vg
            if (const char *why = temporal_vg_cfg_error(tv)) return fail(c, SRT_ERR_INVALID, w_ + why);
            if (cfg->source != SRT_PRESENT_DENOISE_VG) return fail(c, SRT_ERR_UNSUPPORTED, w_ + "the one source is SRT_PRESENT_DENOISE_VG");
        } else if (cfg->source != SRT_PRESENT_ACCUM && cfg->source != SRT_PRESENT_DENOISE)
            return fail(c, SRT_ERR_UNSUPPORTED, w_ + "the temporal sources are SRT_PRESENT_ACCUM and SRT_PRESENT_DENOISE");
    }
    const bool denoised = cfg->source == SRT_PRESENT_DENOISE || cfg->source == SRT_PRESENT_DENOISE_VG || cfg->source == SRT_PRESENT_DENOISE_MV;
    const bool developed = cfg->source == SRT_PRESENT_DEVELOP;
    DenoisePlan plan = {};
    if (cfg->source == SRT_PRESENT_DENOISE) {
        if (const char *why = denoise_cfg_error(&cfg->denoise)) return fail(c, SRT_ERR_INVALID, w_ + why);
        plan = denoise_plan(&cfg->denoise);
    } else if (denoised) {
        if (const char *why = denoise_vg_cfg_error(&cfg->denoise_vg)) return fail(c, SRT_ERR_INVALID, w_ + why);
        plan = denoise_vg_plan(&cfg->denoise_vg);
        plan.measured = cfg->source == SRT_PRESENT_DENOISE_MV;
    }
    float cie[3 * kFilmSamples];
    const float *response3 = cfg->response3;
    if (developed) {
        if (!response3) {
            cie_response_rows(cie);
            response3 = cie;
        }
        if (const char *why = develop_args_error(response3, 3, cfg->scale)) return fail(c, SRT_ERR_INVALID, w_ + why);
    }
    if (!c->accum.bound()) return fail(c, SRT_ERR_INVALID, w_ + "no accumulation with a pass (srt_accum_reset* and srt_render_chunk_accum first)");
    if (denoised || tcfg) if (const int rc = denoise_accumulation_refusal(c, who, plan)) return rc;      // (the stage needs the guides, whatever the source)
    if (moving) if (const char *why = motion_bound_refusal(c)) return fail(c, SRT_ERR_INVALID, w_ + why);
    if (ds && !whole_for(c, false, false))
        return fail(c, SRT_ERR_UNSUPPORTED, w_ + kNotWhole);
    if (developed && !c->accum.spectral()) return fail(c, SRT_ERR_INVALID, w_ + "SRT_PRESENT_DEVELOP needs a spectral accumulation (srt_accum_reset_spectral*)");
    uint32_t rect[4] = {0, 0, 0, 0};
    if (cfg->metered) if (const char *why = meter_rect_error(&cfg->meter, clipped_w(c), clipped_h(c), rect)) return fail(c, SRT_ERR_INVALID, w_ + why);
    HIP_TRY(c, set_device(c));
    // the chain runs on the chunk's rectangle (clipped to the reference grid); the image clips only what is copied out
    const uint32_t w = clipped_w(c), h = clipped_h(c);
    const size_t pixels = (size_t)w * h;
    srt_present_result res = {};
    srt_despeckle_result ds_res = {};
    TemporalStage ts = {tcfg, !denoised, {}};
    ts.moving = moving; ts.tv = tv;
    if (pixels) {
        if (const int rc = develop_reserve(c, who, c->d_expose, ExposeLayout::kBytes)) return rc;
        if (const int rc = develop_reserve(c, who, c->d_present, PresentLayout::bytes(pixels, developed))) return rc;
        const uint32_t *state = c->accum.adaptive() ? AdaptPlanes(c).state : nullptr;
        // the source: null for the sums themselves, else a [h][w][3] XYZ mean on the device
        const float *picture = nullptr;
        if (denoised) {
            if (const int rc = denoise_accumulation(c, who, plan, w, h, ds, tcfg ? &ts : nullptr)) return rc;
            picture = DenoiseLayout(c->d_denoise, pixels).out[0];
        } else if (tcfg) {      // the prepass, the firefly filter if any, the stage: its output, [h][w][3] on the device
            if (const int rc = develop_reserve(c, who, c->d_temporal, TemporalLayout::bytes(pixels))) return rc;
            TemporalParams out = {};
            out.out_xyz = TemporalLayout(c->d_temporal, pixels).img[0];
            if (const int rc = denoise_accumulation(c, who, plan, w, h, ds, &ts, &out)) return rc;
            picture = out.out_xyz;
        } else if (ds) {      // the despeckled mean, [h][w][3] on the device
            if (const int rc = develop_reserve(c, who, c->d_despeckle, DespeckleLayout::bytes(pixels))) return rc;
            DespeckleParams dp = despeckle_accum_source(c, w, h);
            dp.out_xyz = DespeckleLayout(c->d_despeckle, pixels).img[0];
            if (const int rc = run_despeckle(c, who, dp, ds)) return rc;
            picture = dp.out_xyz;
        } else if (developed) {
            if (const int rc = develop_reserve(c, who, c->d_develop, DevelopLayout::bytes(pixels, 3, false))) return rc;
            if (const int rc = run_develop(c, who, c->d_film.as<float>(), c->n_lanes, c->tx, c->ty, c->bx, w, h, response3, 3, cfg->scale, 0u)) return rc;
            PresentNormaliseParams np = {};
            np.developed = DevelopLayout(c->d_develop, pixels, 3).out; np.mean = PresentLayout(c->d_present, pixels).mean;
            np.counts = state; np.samples = c->accum.total; np.tx = c->tx; np.ty = c->ty; np.bx = c->bx; np.w = w; np.h = h;
            HIP_TRY_AS(c, who, launch_present_normalise(np, nullptr));
            picture = np.mean;
        }
        float gain = cfg->tone.gain;
        if (cfg->metered) {
            MeterParams m = {};
            if (picture) {      // a grid of one w x h block makes the block-linear lane the row-major pixel, as srt_meter_kat's
                m.y = picture + 1; m.y_stride = 3; m.samples = 1; m.normalise = 0;
                m.n_lanes = (uint32_t)pixels; m.tx = w; m.ty = h; m.bx = 1;
            } else {
                m.y = AccumLayout(c).y; m.y_stride = 1; m.state = state; m.samples = c->accum.total; m.normalise = 1;
                m.n_lanes = c->n_lanes; m.tx = c->tx; m.ty = c->ty; m.bx = c->bx;
            }
            m.x0 = rect[0]; m.y0 = rect[1]; m.w = rect[2]; m.h = rect[3];
            m.tiles_x = c->tiles_x; m.rank = counted_rank(c); m.world = counted_world(c);
            if (const int rc = run_meter(c, who, m, &cfg->meter, nullptr, &res.meter)) return rc;
            gain = res.meter.gain;
        }
        PresentParams p = {};
        if (picture) p.xyz = picture;
        else { p.sums = AccumLayout(c).sums; p.comp_stride = c->n_lanes; p.state = state; p.samples = c->accum.total; }
        p.tx = c->tx; p.ty = c->ty; p.bx = c->bx; p.w = w; p.h = h;
        p.tiles_x = c->tiles_x; p.rank = counted_rank(c); p.world = counted_world(c);
        const ChunkRect place = chunk_rect(c, image_width, image_height);
        uint8_t *first = out_rgba8 + (size_t)c->last_offy * pitch_bytes + (size_t)c->last_offx * 4;      // (not formed into an address when nothing is copied)
        if (const int rc = run_present(c, who, p, &cfg->tone, gain, place.w, place.h, place.w && place.h ? first : out_rgba8, pitch_bytes, &res.tone)) return rc;
        if (ds) if (const int rc = read_despeckle_counts(c, who, &ds_res)) return rc;
        if (tcfg) if (const int rc = read_temporal_counts(c, who, &ts.res)) return rc;
        if (moving) if (const int rc = read_motion_counts(c, who, &ts.mres)) return rc;
        if (tv) if (const int rc = read_temporal_variance_count(c, who, &ts.n_temporal)) return rc;
    }
    HIP_TRY(c, device_synchronize(c));
    if (result) *result = res;
    if (ds_result) *ds_result = ds_res;
    if (ts_result) *ts_result = ts.res;
    if (mo_result) *mo_result = ts.mres;
    if (n_temporal) *n_temporal = ts.n_temporal;
    return SRT_OK;
}

}  // namespace

int srt_present(srt_ctx *c, const srt_present_cfg *cfg, uint8_t *out_rgba8, size_t pitch_bytes, uint32_t image_width, uint32_t image_height,
                srt_present_result *result) {
    return present_chain(c, "srt_present", cfg, nullptr, out_rgba8, pitch_bytes, image_width, image_height, result, nullptr);
}

int srt_present_despeckled(srt_ctx *c, const srt_present_cfg *present_cfg, const srt_despeckle *despeckle_cfg, uint8_t *out_rgba8, size_t pitch_bytes,
                           uint32_t image_width, uint32_t image_height, srt_present_result *result, srt_despeckle_result *despeckle_result) {
    if (!despeckle_cfg) return fail(c, SRT_ERR_INVALID, "srt_present_despeckled: null argument");
    return present_chain(c, "srt_present_despeckled", present_cfg, despeckle_cfg, out_rgba8, pitch_bytes, image_width, image_height, result, despeckle_result);
}

int srt_present_temporal(srt_ctx *c, const srt_present_cfg *present_cfg, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg, uint8_t *out_rgba8,
                         size_t pitch_bytes, uint32_t image_width, uint32_t image_height, srt_present_result *result, srt_temporal_result *temporal_result) {
    if (!temporal_cfg) return fail(c, SRT_ERR_INVALID, "srt_present_temporal: null argument");
    return present_chain(c, "srt_present_temporal", present_cfg, despeckle_cfg, out_rgba8, pitch_bytes, image_width, image_height, result, nullptr, temporal_cfg,
                         temporal_result);
}

int srt_present_temporal_moving(srt_ctx *c, const srt_present_cfg *present_cfg, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg, uint8_t *out_rgba8,
                                size_t pitch_bytes, uint32_t image_width, uint32_t image_height, srt_present_result *result, srt_temporal_result *temporal_result,
                                srt_motion_result *motion_result) {
    if (!temporal_cfg) return fail(c, SRT_ERR_INVALID, "srt_present_temporal_moving: null argument");
    return present_chain(c, "srt_present_temporal_moving", present_cfg, despeckle_cfg, out_rgba8, pitch_bytes, image_width, image_height, result, nullptr, temporal_cfg,
                         temporal_result, true, motion_result);
}

int srt_present_temporal_vg(srt_ctx *c, const srt_present_cfg *present_cfg, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg,
                            const srt_temporal_vg *tv_cfg, uint8_t *out_rgba8, size_t pitch_bytes, uint32_t image_width, uint32_t image_height,
                            srt_present_result *result, srt_temporal_result *temporal_result, uint64_t *n_temporal, srt_motion_result *motion_result) {
    if (!temporal_cfg || !tv_cfg) return fail(c, SRT_ERR_INVALID, "srt_present_temporal_vg: null argument");
    return present_chain(c, "srt_present_temporal_vg", present_cfg, despeckle_cfg, out_rgba8, pitch_bytes, image_width, image_height, result, nullptr, temporal_cfg,
                         temporal_result, tv_cfg->moving == 1u, motion_result, tv_cfg, n_temporal);
}

int srt_present_kat(srt_ctx *c, const srt_tone *tone, const float *xyz_mean, uint32_t w, uint32_t h, uint8_t *out_rgba8, srt_tone_result *result) {
    const char *who = "srt_present_kat";
    if (!c || !tone || !xyz_mean || !out_rgba8) return fail(c, SRT_ERR_INVALID, "srt_present_kat: null argument");
    if (w == 0 || h == 0 || (uint64_t)w * h > 0x7fffffffull) return fail(c, SRT_ERR_INVALID, "srt_present_kat: w x h must be in 1 .. 2^31 - 1");
    if (const char *why = tone_cfg_error(tone)) return fail(c, SRT_ERR_INVALID, std::string("srt_present_kat: ") + why);
    HIP_TRY(c, set_device(c));
    const size_t pixels = (size_t)w * h;
    if (const int rc = develop_reserve(c, who, c->d_present, PresentLayout::bytes(pixels, false))) return rc;
    if (const int rc = develop_reserve(c, who, c->d_expose, ExposeLayout::kBytes)) return rc;
    if (const int rc = upload_kat_xyz(c, who, xyz_mean, w, h)) return rc;
    PresentParams p = {};
    p.xyz = c->d_expose_in.as<float>(); p.w = w; p.h = h; p.tiles_x = (w + 7u) / 8u; p.rank = 0; p.world = 1;
    srt_tone_result res = {};
    if (const int rc = run_present(c, who, p, tone, tone->gain, w, h, out_rgba8, (size_t)w * 4, &res)) return rc;
    if (result) *result = res;
    return SRT_OK;
}

int srt_present_last_ms(srt_ctx *c, float *ms) {
    if (!c || !ms) return fail(c, SRT_ERR_INVALID, "srt_present_last_ms: null argument");
    if (!c->present_timed) return fail(c, SRT_ERR_INVALID, "srt_present_last_ms: no present kernel has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->present_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->present_ev[0], c->present_ev[1]));
    return SRT_OK;
}

int srt_get_tile_costs(srt_ctx *c, uint32_t *out, size_t n) {
    // n = tiles_local: the probe's cost per local tile; n = 2 * tiles_local: followed by the cost of each tile's most expensive pixel
    if (!c || !out || !c->d_tile_cost || (n > c->tiles_local && n != 2 * (size_t)c->tiles_local)) return fail(c, SRT_ERR_INVALID, "srt_get_tile_costs: no probe has run / bad size");
    if (const int rc = srt_synchronize(c)) return rc;
    HIP_TRY(c, hipMemcpy(out, c->d_tile_cost.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SRT_OK;
}

int srt_get_stats(srt_ctx *c, srt_stats *out) {
    if (!c || !out) return fail(c, SRT_ERR_INVALID, "srt_get_stats: null argument");
    if (const int rc = srt_synchronize(c)) return rc;
    unsigned long long h[kCounters];
    HIP_TRY(c, hipMemcpy(h, c->d_counters.ptr, sizeof(h), hipMemcpyDeviceToHost));
    if (h[23] != 0)      // instrumented launches: render_kernel S3's invariant (a wave's first fetch is made by all 64 lanes)
        return fail(c, SRT_ERR_HIP, "srt_get_stats: a wave made a partial first fetch from the pixel queue: its assigned first row was not rendered");
    memset(out, 0, sizeof(*out));
    out->rays = h[0]; out->node_visits = h[1]; out->tri_tests = h[2]; out->box_tests = h[3];
    for (int k = 0; k < 9; k++) out->util[k] = h[4 + k];
    out->reserved[0] = h[13]; out->reserved[1] = h[14];
    for (int k = 0; k < 4; k++) out->shade[k] = h[15 + k];
    for (int k = 0; k < 4; k++) out->waves[k] = h[19 + k];   // instrumented: waves, sum / max of their life times, drain time
    out->hits = h[24];
    if (c->stats_adaptive) {      // an adaptive pass: the pixels that rendered in it, counted on the device (adapt_flag_kernel)
        uint64_t rendered = 0;
        const int rc = read_adapt_counts(c, &rendered, nullptr);
        out->paths = rendered * c->stats_spp;
        return rc;
    }
    // paths = spp * pixels owned by this rank
    uint64_t pixels = 0;
    const uint32_t lim_w = clipped_w(c), lim_h = clipped_h(c);
    for (uint32_t t = c->rank; t < c->n_tiles; t += c->world) {
        const uint32_t tx0 = (t % c->tiles_x) * 8, ty0 = (t / c->tiles_x) * 8;
        const uint32_t w = tx0 < lim_w ? std::min<uint32_t>(8, lim_w - tx0) : 0, hgt = ty0 < lim_h ? std::min<uint32_t>(8, lim_h - ty0) : 0;
        pixels += (uint64_t)w * hgt;
    }
    out->paths = pixels * (c->stats_spp ? c->stats_spp : c->spp);
    return SRT_OK;
}

int srt_get_wave_debug(srt_ctx *c, uint32_t *out, size_t n_waves) {
    if (!c || !out || !c->d_wave_debug || n_waves > wave_debug_waves(c)) return fail(c, SRT_ERR_INVALID, "srt_get_wave_debug: no instrumented launch yet / bad size");
    if (const int rc = srt_synchronize(c)) return rc;
    HIP_TRY(c, hipMemcpy(out, c->d_wave_debug.as<const char>() + sizeof(OrderProfile), n_waves * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SRT_OK;
}

// Child order from a profile of the real rays.  The traversal is the reference's fixed left-first walk (bvh.cu:154-160), so which
// child of a node is visited first is a property of the TREE -- and for every ray whose closest hit lies under one child while the
// other child's box lies on its path beyond that hit, visiting the hit's side first lets closest_so_far prune the other subtree.
// The builder's rule (nearer child to the camera first) is right for camera rays; this call measures instead: one instrumented
// probe frame of the context's camera (width x height, spp, bounce_limit) in which every finished closest-hit query walks from
// its triangle's leaf to the root and notes, at every ancestor whose OTHER child's box the ray meets only beyond the hit, under
// which child the hit lay.  Children are swapped wherever the right one won more often (at least `min_samples` such rays at the
// node; elsewhere the existing order stays).  A second probe frame then checks the work counters (node records + 2 x triangle
// tests of the same frame, deterministic): if the new order is not cheaper the swaps are undone (cfg 5's mesh: no gain -> kept as
// built).  The scene is left (re-)ordered and uploaded; topology, boxes and depth do not change, and like any change of the tree
// it can only alter a result where two triangles tie exactly in t (Q11).  n_swapped (optional) = nodes changed (0 after an undo).
int srt_order_children_by_profile(srt_ctx *c, srt_scene *s, uint32_t width, uint32_t height, uint32_t spp, uint32_t bounce_limit,
                                  uint32_t min_samples, uint32_t *n_swapped) {
    if (n_swapped) *n_swapped = 0;
    if (!c || !s || !s->bvh_valid) return fail(c, SRT_ERR_INVALID, "srt_order_children_by_profile: null argument / BVH not built");
    c->accum.invalidate();
    if (!c->camera_ready) return fail(c, SRT_ERR_INVALID, "srt_order_children_by_profile: set the camera first (srt_set_camera)");
    if (width == 0 || height == 0 || spp == 0) return fail(c, SRT_ERR_INVALID, "srt_order_children_by_profile: empty probe frame");
    const size_t n_nodes = s->nodes.size(), n_tris = s->raw.size();
    int rc = srt_upload_scene(c, s);
    if (rc != SRT_OK || n_nodes < 3) return rc;
    std::vector<int32_t> leaf(n_tris, 0), up(n_nodes, -1);
    std::vector<float> sibbox(6 * n_nodes, 0.f);
    for (size_t k = 0; k < n_nodes; k++) {
        const BvhNode &nd = s->nodes[k];
        if (nd.prim >= 0) { leaf[(size_t)nd.prim] = (int32_t)k; continue; }
        up[(size_t)nd.left] = (int32_t)(2 * k); up[(size_t)nd.right] = (int32_t)(2 * k + 1);
        memcpy(&sibbox[6 * (size_t)nd.left], s->nodes[(size_t)nd.right].box, 6 * sizeof(float));
        memcpy(&sibbox[6 * (size_t)nd.right], s->nodes[(size_t)nd.left].box, 6 * sizeof(float));
    }
    HIP_TRY(c, set_device(c));
    DeviceBuffer d_leaf, d_up, d_sib, d_cnt;      // (the probe frames' c->order_profile points at them: probe_frame clears it before it returns)
    const char *what = "srt_order_children_by_profile: device buffers";
    HIP_TRY_AS(c, what, d_leaf.reserve(std::max<size_t>(n_tris, 1) * sizeof(int32_t)));
    HIP_TRY_AS(c, what, d_up.reserve(n_nodes * sizeof(int32_t)));
    HIP_TRY_AS(c, what, d_sib.reserve(6 * n_nodes * sizeof(float)));
    HIP_TRY_AS(c, what, d_cnt.reserve(2 * n_nodes * sizeof(uint32_t)));
    HIP_TRY_AS(c, what, hipMemcpy(d_leaf.ptr, leaf.data(), n_tris * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, what, hipMemcpy(d_up.ptr, up.data(), n_nodes * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, what, hipMemcpy(d_sib.ptr, sibbox.data(), 6 * n_nodes * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, what, hipMemset(d_cnt.ptr, 0, 2 * n_nodes * sizeof(uint32_t)));
    // instrumented probe frames on this context alone (its partition and counter setting are restored afterwards)
    const bool counting = c->count_traversal;
    const uint32_t rank = c->rank, world = c->world;
    const uint32_t tx = 28, ty = 16, bx = width / tx + 1, by = height / ty + 1;      // the reference's grid (render_manager.cu:84-94)
    auto probe_frame = [&](bool collect, unsigned long long &work) -> int {
        c->order_profile = OrderProfile{};
        if (collect) {
            c->order_profile.magic = kOrderProfileMagic; c->order_profile.leaf = d_leaf.as<int32_t>(); c->order_profile.up = d_up.as<int32_t>();
            c->order_profile.sibbox = d_sib.as<float>(); c->order_profile.cnt = d_cnt.as<uint32_t>(); c->order_profile.n_nodes = n_nodes;
        }
        c->count_traversal = true; c->rank = 0; c->world = 1;
        int r = srt_init_device_params(c, tx, ty, bx, by, width, height, spp, bounce_limit, SRT_DEFAULT_SEED);
        if (r == SRT_OK) r = srt_render_chunk(c, width, height, 0, 0, nullptr);
        if (r == SRT_OK) r = srt_synchronize(c);
        c->count_traversal = counting; c->rank = rank; c->world = world;
        c->order_profile = OrderProfile{};
        c->params_ready = false;      // (the probe's RNG state and grid are not the caller's: srt_init_device_params comes next)
        if (r != SRT_OK) return r;
        unsigned long long h[kCounters];
        HIP_TRY_AS(c, "srt_order_children_by_profile: counters", hipMemcpy(h, c->d_counters.ptr, sizeof(h), hipMemcpyDeviceToHost));
        work = h[1] + 2ull * h[2];      // node records visited + 2 x triangle tests
        return SRT_OK;
    };
    unsigned long long work_before = 0, work_after = 0;
    if ((rc = probe_frame(true, work_before)) != SRT_OK) return rc;
    std::vector<uint32_t> cnt(2 * n_nodes, 0u);
    HIP_TRY_AS(c, "srt_order_children_by_profile: read back", hipMemcpy(cnt.data(), d_cnt.ptr, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    {
        // a collecting launch that recorded nothing (header not seen by the kernel, or a probe frame without a single hit) must not read
        // as "the order was already the cheapest"
        unsigned long long samples = 0;
        for (uint32_t v : cnt) samples += v;
        if (samples == 0) return fail(c, SRT_ERR_INVALID, "srt_order_children_by_profile: the probe frame recorded no samples (no closest hit with the sibling's box beyond it)");
    }
    const uint32_t *won = cnt.data();      // [node * 2 + side]: hits under that child with the sibling's box beyond the hit
    std::vector<uint32_t> swapped_nodes;
    for (size_t k = 0; k < n_nodes; k++) {
        BvhNode &nd = s->nodes[k];
        if (nd.prim >= 0) continue;
        const uint32_t l = won[2 * k], r = won[2 * k + 1];
        if (l + r >= std::max<uint32_t>(min_samples, 1u) && r > l) { std::swap(nd.left, nd.right); swapped_nodes.push_back((uint32_t)k); }
    }
    if (!swapped_nodes.empty()) {
        rc = srt_upload_scene(c, s);
        if (rc == SRT_OK) rc = probe_frame(false, work_after);
        if (rc == SRT_OK && work_after >= work_before) {      // not cheaper on the very frame it was derived from: undo
            for (uint32_t k : swapped_nodes) std::swap(s->nodes[k].left, s->nodes[k].right);
            swapped_nodes.clear();
            rc = srt_upload_scene(c, s);
        }
    }
    if (rc == SRT_OK && n_swapped) *n_swapped = (uint32_t)swapped_nodes.size();
    return rc;
}

int srt_pixels_per_lane(const srt_ctx *c, uint32_t width, uint32_t height, uint32_t world, double *out) {
    if (!c || !c->scene_ready || !out) return fail(nullptr, SRT_ERR_INVALID, "srt_pixels_per_lane: no scene uploaded / null argument");
    const double lanes = (double)c->n_cu * plan_of(c).waves_per_cu * 64.0;
    *out = (double)width * height / (double)std::max<uint32_t>(world, 1u) / (lanes > 0 ? lanes : 1.0);
    return SRT_OK;
}

// One instrumented frame of the context's camera and uploaded scene on this context alone, as srt_order_children_by_profile's probe frames
// are rendered (the reference's grid; partition and counter setting restored afterwards; srt_init_device_params comes next).  segs != null:
// the frame samples its closest-hit queries (OrderProfile::seg, srt_internal.h) and *segs receives the sampled segments, 7 floats each, in
// canonical order -- ascending by the bit patterns of their seven words, so that the array does not depend on the order in which the waves
// took their tickets.  work (optional): node records + 2 x triangle tests of the frame.
static int segment_frame(srt_ctx *c, uint32_t width, uint32_t height, uint32_t spp, uint32_t bounce_limit, uint32_t stride, uint32_t phase,
                         size_t capacity, std::vector<float> *segs, uint64_t *n_queries, unsigned long long *work) {
    const char *what = "srt_collect_ray_segments: device buffers";
    // a launch draws at most one query per path and bounce: the tickets fit 32 bits, and so does ticket + phase
    const unsigned long long most_queries = (unsigned long long)width * height * spp * std::max<uint32_t>(bounce_limit, 1u);
    if (most_queries + stride >= (1ull << 32)) return fail(c, SRT_ERR_INVALID, "srt_collect_ray_segments: the frame may cast 2^32 queries or more");
    const size_t slots = segs ? (size_t)std::min<unsigned long long>(capacity, most_queries / stride + 1) : 0;
    HIP_TRY(c, set_device(c));
    DeviceBuffer d_seg, d_tickets;      // (the frame's c->order_profile points at them: cleared before this function returns)
    if (segs) {
        HIP_TRY_AS(c, what, d_seg.reserve(std::max<size_t>(slots, 1) * 2 * sizeof(float4)));
        HIP_TRY_AS(c, what, d_tickets.reserve(4 * sizeof(uint32_t)));
        HIP_TRY_AS(c, what, hipMemset(d_tickets.ptr, 0, 4 * sizeof(uint32_t)));
    }
    const bool counting = c->count_traversal;
    const uint32_t rank = c->rank, world = c->world;
    const uint32_t tx = 28, ty = 16, bx = width / tx + 1, by = height / ty + 1;      // the reference's grid (render_manager.cu:84-94)
    c->order_profile = OrderProfile{};
    if (segs) {
        c->order_profile.seg = d_seg.as<float4>(); c->order_profile.seg_tickets = d_tickets.as<uint32_t>();
        c->order_profile.seg_stride = stride; c->order_profile.seg_phase = phase; c->order_profile.seg_capacity = slots;
    }
    c->count_traversal = true; c->rank = 0; c->world = 1;
    int r = srt_init_device_params(c, tx, ty, bx, by, width, height, spp, bounce_limit, SRT_DEFAULT_SEED);
    if (r == SRT_OK) r = srt_render_chunk(c, width, height, 0, 0, nullptr);
    if (r == SRT_OK) r = srt_synchronize(c);
    c->count_traversal = counting; c->rank = rank; c->world = world;
    c->order_profile = OrderProfile{};
    c->params_ready = false;      // (the frame's RNG state and grid are not the caller's: srt_init_device_params comes next)
    if (r != SRT_OK) return r;
    unsigned long long h[kCounters];
    HIP_TRY_AS(c, "srt_collect_ray_segments: counters", hipMemcpy(h, c->d_counters.ptr, sizeof(h), hipMemcpyDeviceToHost));
    if (work) *work = h[1] + 2ull * h[2];
    if (!segs) return SRT_OK;
    uint32_t tickets = 0;
    HIP_TRY_AS(c, "srt_collect_ray_segments: read back", hipMemcpy(&tickets, d_tickets.ptr, sizeof(tickets), hipMemcpyDeviceToHost));
    if (n_queries) *n_queries = tickets;
    // sampled tickets: t in [0, tickets) with (t + phase) % stride == 0
    const unsigned long long sampled = tickets ? ((unsigned long long)tickets - 1 + phase) / stride - (phase ? 1 : 0) + 1 : 0;
    const size_t n = (size_t)std::min<unsigned long long>(sampled, slots);
    std::vector<float> raw(8 * n);
    if (n) HIP_TRY_AS(c, "srt_collect_ray_segments: read back", hipMemcpy(raw.data(), d_seg.ptr, raw.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<std::array<uint32_t, kSegmentFloats>> rows(n);
    for (size_t k = 0; k < n; k++) memcpy(rows[k].data(), &raw[8 * k], kSegmentFloats * sizeof(float));
    std::sort(rows.begin(), rows.end());
    segs->resize(kSegmentFloats * n);
    for (size_t k = 0; k < n; k++) memcpy(&(*segs)[kSegmentFloats * k], rows[k].data(), kSegmentFloats * sizeof(float));
    return SRT_OK;
}

int srt_collect_ray_segments(srt_ctx *c, uint32_t width, uint32_t height, uint32_t spp, uint32_t bounce_limit, uint32_t stride, uint64_t seed,
                             float *segments, size_t capacity, size_t *n_segments, uint64_t *n_queries) {
    if (n_segments) *n_segments = 0;
    if (n_queries) *n_queries = 0;
    if (!c || !n_segments || (!segments && capacity)) return fail(c, SRT_ERR_INVALID, "srt_collect_ray_segments: null argument");
    c->accum.invalidate();
    if (!c->scene_ready || !c->camera_ready) return fail(c, SRT_ERR_INVALID, "srt_collect_ray_segments: upload a scene and set the camera first");
    if (width == 0 || height == 0 || spp == 0 || stride == 0) return fail(c, SRT_ERR_INVALID, "srt_collect_ray_segments: empty frame / stride 0");
    std::vector<float> segs;
    const int rc = segment_frame(c, width, height, spp, bounce_limit, stride, (uint32_t)(seed % stride), capacity, &segs, n_queries, nullptr);
    if (rc != SRT_OK) return rc;
    *n_segments = segs.size() / kSegmentFloats;
    if (!segs.empty()) memcpy(segments, segs.data(), segs.size() * sizeof(float));
    return SRT_OK;
}

// The throughput tree-tuning recipe (include/srt_c_api.h): every constant of it, once.
static constexpr double kTunePixelsPerLane = 6.0;        // fewer: the launch is bound by its longest pixel chain and keeps the tree as built
static constexpr size_t kTuneReinsertionMaxTris = 8192;  // larger trees: measured no gain from reinsertion
static constexpr int kTuneReinsertionPasses = 3;         // (they converge)
static constexpr uint32_t kTuneProbeDivisor = 4, kTuneProbeMinSide = 32, kTuneProbeSpp = 8;      // probe frame: a quarter of the frame's size, 8 spp
static constexpr uint32_t kTuneDecidingRays = 16;        // a node's children are re-ordered from at least this many deciding rays
// the ray-weighted reinsertion of a throughput-bound launch: every query of a 1 spp frame at a twelfth of the frame's size (stride 1: the set
// does not depend on the waves' order), thinned evenly to 2048 segments in canonical order (the host time is linear in passes x segments:
// profiles/tree_rays/)
static constexpr uint32_t kTuneSegmentDivisor = 12, kTuneSegmentSpp = 1;
static constexpr size_t kTuneSegments = 2048;

static int tune_tree(srt_ctx *c, srt_scene *s, uint32_t width, uint32_t height, uint32_t world, uint32_t bounce_limit, int only_if_throughput_bound,
                     const float *user_segments, size_t n_user_segments, bool sample_given, srt_tree_tuning *out) {
    int rc = srt_upload_scene(c, s);
    if (rc == SRT_OK) rc = srt_pixels_per_lane(c, width, height, world, &out->pixels_per_lane);
    if (rc != SRT_OK) return rc;
    out->throughput_bound = out->pixels_per_lane >= kTunePixelsPerLane ? 1u : 0u;
    if (only_if_throughput_bound && !out->throughput_bound) return SRT_OK;
    // (reinsertion may deepen the tree: deeper LDS stacks, fewer cached records -- a tree that just fitted LDS no longer does, which
    // costs far more than the passes return.  The plan is a host function of the flattened tree: nothing is uploaded to decide)
    auto resident = [&](const FlatScene &f) { LaunchPlan lp; render_launch_plan(f.stack_depth, f.n_records, f.n_inner, c->knobs, lp); return lp.all_cached; };
    auto stays_resident = [&](const FlatScene &before, const FlatScene &after) { return !(resident(before) && !resident(after)); };
    if (s->raw.size() <= kTuneReinsertionMaxTris && !out->throughput_bound) {
        // asked for a launch that is bound by its longest pixel: box areas, as ever (no sample of total work is taken for it)
        out->reinsertion = optimise_bvh_unless(*s, kTuneReinsertionPasses, stays_resident) ? 1u : 2u;
    } else if (s->raw.size() <= kTuneReinsertionMaxTris) {
        // throughput-bound: the passes count the frame's own queries.  Frame 1 (the tree that walked in) samples them and sets the work to
        // beat; frame 2 (the new tree, same frame) must come out cheaper, or the tree that walked in is put back.
        const uint32_t sw = std::max(width / kTuneSegmentDivisor, kTuneProbeMinSide), sh = std::max(height / kTuneSegmentDivisor, kTuneProbeMinSide);
        srt_camera_data seg_cam{};
        rc = srt_scene_default_camera(s, (int)sw, (int)sh, &seg_cam);
        if (rc == SRT_OK) rc = srt_set_camera(c, &seg_cam);
        else fail(c, rc, global_error());
        std::vector<float> all, segs;
        unsigned long long work_before = 0, work_after = 0;
        if (rc == SRT_OK) {
            c->accum.invalidate();
            const size_t cap = (size_t)sw * sh * kTuneSegmentSpp * std::max<uint32_t>(bounce_limit, 1u);
            rc = segment_frame(c, sw, sh, kTuneSegmentSpp, bounce_limit, 1, 0, cap, sample_given ? nullptr : &all, nullptr, &work_before);
        }
        if (rc == SRT_OK) {
            const float *src = sample_given ? user_segments : all.data();
            const size_t n_src = sample_given ? n_user_segments : all.size() / kSegmentFloats, n_use = std::min(n_src, kTuneSegments);
            segs.resize(kSegmentFloats * n_use);
            for (size_t k = 0; k < n_use; k++)      // evenly through the canonical order
                memcpy(&segs[kSegmentFloats * k], src + kSegmentFloats * (size_t)((unsigned long long)k * n_src / n_use), kSegmentFloats * sizeof(float));
            out->segments = (uint32_t)usable_ray_segments(segs.data(), n_use);
            if (out->segments == 0) {
                out->reinsertion = 5u;      // nothing measured: the topology is not touched
            } else {
                const std::vector<BvhNode> nodes = s->nodes;
                const int32_t root = s->root;
                const int depth = s->depth;
                const bool has_order_eye = s->has_order_eye;
                float order_eye[3];
                memcpy(order_eye, s->order_eye, sizeof(order_eye));
                // the measured objective likes deeper trees than box areas do: the passes take no position that would push the stack bound
                // past the deepest one this tree's launch plan still keeps LDS resident (stays_resident keeps the last word)
                int max_internal_depth = INT_MAX;
                FlatScene flat;
                if (flatten_scene(*s, flat) == SRT_OK && resident(flat)) {
                    int d = flat.stack_depth;
                    auto resident_at = [&](int stack_depth) { LaunchPlan lp; render_launch_plan(stack_depth, flat.n_records, flat.n_inner, c->knobs, lp); return lp.all_cached; };
                    while (d < 1024 && resident_at(d + 1)) d++;
                    max_internal_depth = d + 1;      // (the last internal node of a path has a leaf child and needs no stack slot)
                }
                if (!optimise_bvh_unless(*s, kTuneReinsertionPasses, stays_resident, segs.data(), n_use, max_internal_depth)) {
                    out->reinsertion = 2u;
                } else {
                    rc = srt_upload_scene(c, s);
                    if (rc == SRT_OK) rc = segment_frame(c, sw, sh, kTuneSegmentSpp, bounce_limit, 1, 0, 0, nullptr, nullptr, &work_after);
                    out->reinsertion = 3u;
                    if (rc != SRT_OK || work_after >= work_before) {      // the veto: the work counters of the same frame did not fall
                        s->nodes = nodes; s->root = root; s->depth = depth; s->has_order_eye = has_order_eye;
                        memcpy(s->order_eye, order_eye, sizeof(order_eye));
                        out->reinsertion = 4u;
                    }
                }
            }
        }
        if (rc != SRT_OK) { out->order_status = rc; return SRT_OK; }
    }
    const uint32_t pw = std::max(width / kTuneProbeDivisor, kTuneProbeMinSide), ph = std::max(height / kTuneProbeDivisor, kTuneProbeMinSide);
    srt_camera_data probe_cam{};
    rc = srt_scene_default_camera(s, (int)pw, (int)ph, &probe_cam);
    if (rc == SRT_OK) rc = srt_set_camera(c, &probe_cam);
    if (rc == SRT_OK) {
        out->probe_width = pw; out->probe_height = ph; out->probe_spp = kTuneProbeSpp;
        rc = srt_order_children_by_profile(c, s, pw, ph, kTuneProbeSpp, bounce_limit, kTuneDecidingRays, &out->nodes_swapped);
    } else fail(c, rc, global_error());      // (the scene's message, where the front ends look for it)
    out->order_status = rc;
    return SRT_OK;
}

int srt_tune_tree_for_throughput(srt_ctx *c, srt_scene *s, uint32_t width, uint32_t height, uint32_t world, uint32_t bounce_limit,
                                 int only_if_throughput_bound, srt_tree_tuning *out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!c || !s || !out || !s->bvh_valid || width == 0 || height == 0)
        return fail(c, SRT_ERR_INVALID, "srt_tune_tree_for_throughput: null argument / BVH not built / empty frame");
    return tune_tree(c, s, width, height, world, bounce_limit, only_if_throughput_bound, nullptr, 0, false, out);
}

int srt_tune_tree_with_segments(srt_ctx *c, srt_scene *s, uint32_t width, uint32_t height, uint32_t world, uint32_t bounce_limit,
                                int only_if_throughput_bound, const float *segments, size_t n_segments, srt_tree_tuning *out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!c || !s || !out || !s->bvh_valid || width == 0 || height == 0 || (!segments && n_segments))
        return fail(c, SRT_ERR_INVALID, "srt_tune_tree_with_segments: null argument / BVH not built / empty frame");
    return tune_tree(c, s, width, height, world, bounce_limit, only_if_throughput_bound, segments, n_segments, true, out);
}

int srt_set_count_traversal(srt_ctx *c, int on) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_set_count_traversal: null ctx");
    c->count_traversal = on != 0;
    return SRT_OK;
}

int srt_last_kernel_ms(srt_ctx *c, float *ms) {
    if (!c || !ms || !c->timed) return fail(c, SRT_ERR_INVALID, "srt_last_kernel_ms: nothing rendered yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return SRT_OK;
}

int srt_trace_rays(srt_ctx *c, const float *rays, size_t n, float *out) {
    if (!c || !c->scene_ready || (!rays && n) || (!out && n)) return fail(c, SRT_ERR_INVALID, "srt_trace_rays: scene not uploaded / bad argument");
    if (n == 0) return SRT_OK;
    HIP_TRY(c, set_device(c));
    DeviceBuffer d_in, d_out;
    HIP_TRY_AS(c, "srt_trace_rays", d_in.reserve(6 * n * sizeof(float)));
    HIP_TRY_AS(c, "srt_trace_rays", d_out.reserve(4 * n * sizeof(float)));
    HIP_TRY_AS(c, "srt_trace_rays", hipMemcpy(d_in.ptr, rays, 6 * n * sizeof(float), hipMemcpyHostToDevice));
    RenderParams p;
    fill_params(c, p);
    HIP_TRY_AS(c, "srt_trace_rays", launch_trace(p, d_in.as<float>(), n, d_out.as<float>(), nullptr));
    HIP_TRY_AS(c, "srt_trace_rays", device_synchronize(c));
    HIP_TRY_AS(c, "srt_trace_rays", hipMemcpy(out, d_out.ptr, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
    return SRT_OK;
}

// ---- batched ray queries (srt_c_api.h, "Ray queries") ---------------------------------------------------------------------------
namespace {

// nullptr when the call may go ahead; else why it is refused (nothing enqueued, nothing written).  dev: the pointers are device pointers,
// whose 16-byte alignment is required for rays and hits.
const char *query_refusal(const srt_ctx *c, const void *rays, size_t n, const void *out, bool any, bool dev) {
    if (!c->scene_ready) return "no scene uploaded";
    if (n > 0 && (!rays || !out)) return "null pointer";
    if (dev && (((uintptr_t)rays & 15u) != 0 || (!any && ((uintptr_t)out & 15u) != 0))) return "a device rays / hits pointer is not 16-byte aligned";
    if (n > (size_t)SRT_QUERY_MAX_RAYS) return "n does not fit the 32-bit ray counter (n > SRT_QUERY_MAX_RAYS)";
    return nullptr;
}

// Enqueue one query launch of n > 0 rays on `st` (the context's order already taken care of): counter reset, events, kernel.
int query_enqueue(srt_ctx *c, const char *who, const float *rays_dev, size_t n, void *out_dev, bool any, hipStream_t st) {
    if (const int rc = develop_reserve(c, who, c->d_query, 256)) return rc;
    for (int k = 0; k < 2; k++) if (!c->query_ev[k]) HIP_TRY_AS(c, who, hipEventCreate(&c->query_ev[k]));
    const LaunchPlan lp = plan_of(c);
    const bool narrow = render_narrow_refs(c->n_records, c->knobs);
    const bool paired = render_paired_variant(c->paired, narrow, lp.all_cached);
    const QueryShape s = query_shape(lp, narrow, paired, c->stack_depth, c->n_records, c->knobs, (uint32_t)c->n_cu, c->query_max_waves, n);
    QueryParams p;
    memset(&p, 0, sizeof(p));
    p.nodes = c->d_nodes.as<const float4>(); p.fringe = c->d_fringe.as<const float4>(); p.tris = c->d_tris.as<const float4>();
    p.root_ref = c->root_ref; p.stack_depth = c->stack_depth; p.n_inner = c->n_inner; p.n_cached = s.n_cached; p.n_records = c->n_records;
    p.fringe_stride = c->fringe_stride;
    // the render launch's FRINGE weight for this plan (srt_render_chunk's choice, env SRT_SCORE_FRINGE included)
    p.score_fringe = c->score_fringe ? c->score_fringe : (lp.all_cached ? (paired ? 400u : 280u) : kScoreFringeL2);
    p.rays = reinterpret_cast<const float4 *>(rays_dev); p.n = (uint32_t)n;
    p.counter = c->d_query.as<uint32_t>();
    if (any) p.occluded = static_cast<uint8_t *>(out_dev); else p.hits = static_cast<float4 *>(out_dev);
    c->query_timed = false;
    HIP_TRY_AS(c, who, hipMemsetAsync(p.counter, 0, sizeof(uint32_t), st));
    HIP_TRY_AS(c, who, hipEventRecord(c->query_ev[0], st));
    HIP_TRY_AS(c, who, launch_query(p, s, any, st));
    HIP_TRY_AS(c, who, hipEventRecord(c->query_ev[1], st));
    c->query_timed = true;
    c->query_info = srt_query_info{};
    c->query_info.waves = s.waves; c->query_info.n_cached = (uint32_t)s.n_cached; c->query_info.narrow_refs = s.narrow ? 1u : 0u;
    c->query_info.all_cached = s.all_cached ? 1u : 0u; c->query_info.paired = s.paired ? 1u : 0u; c->query_info.any = any ? 1u : 0u;
    return SRT_OK;
}

// the host entries: rays in, answers out, through the context's staging block on the NULL stream; synchronises
int query_host(srt_ctx *c, const char *who, const float *rays, size_t n, void *out, bool any) {
    if (!c) return fail(c, SRT_ERR_INVALID, std::string(who) + ": null ctx");
    if (const char *why = query_refusal(c, rays, n, out, any, false)) return fail(c, SRT_ERR_INVALID, std::string(who) + ": " + why);
    if (n == 0) return SRT_OK;
    HIP_TRY_AS(c, who, set_device(c));
    const size_t in_bytes = 8 * n * sizeof(float), out_bytes = any ? n : 4 * n * sizeof(float);
    if (const int rc = develop_reserve(c, who, c->d_query_io, in_bytes + out_bytes)) return rc;
    HIP_TRY_AS(c, who, hipMemcpy(c->d_query_io.ptr, rays, in_bytes, hipMemcpyHostToDevice));
    void *d_out = c->d_query_io.as<char>() + in_bytes;      // (in_bytes is a multiple of 32: the answers stay 16-byte aligned)
    if (const int rc = query_enqueue(c, who, c->d_query_io.as<float>(), n, d_out, any, nullptr)) return rc;
    HIP_TRY_AS(c, who, device_synchronize(c));
    HIP_TRY_AS(c, who, hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    return SRT_OK;
}

// the device entries: the caller's device pointers, on the caller's stream, under the order of the context's calls; no synchronisation
int query_dev(srt_ctx *c, const char *who, const float *rays_dev, size_t n, void *out_dev, bool any, void *stream) {
    if (!c) return fail(c, SRT_ERR_INVALID, std::string(who) + ": null ctx");
    if (const char *why = query_refusal(c, rays_dev, n, out_dev, any, true)) return fail(c, SRT_ERR_INVALID, std::string(who) + ": " + why);
    if (n == 0) return SRT_OK;
    HIP_TRY_AS(c, who, set_device(c, (hipStream_t)stream));
    return query_enqueue(c, who, rays_dev, n, out_dev, any, (hipStream_t)stream);
}

}  // namespace

int srt_intersect_rays(srt_ctx *c, const float *rays, size_t n, float *hits) { return query_host(c, "srt_intersect_rays", rays, n, hits, false); }
int srt_occluded_rays(srt_ctx *c, const float *rays, size_t n, uint8_t *occluded) { return query_host(c, "srt_occluded_rays", rays, n, occluded, true); }
int srt_intersect_rays_dev(srt_ctx *c, const float *rays_dev, size_t n, float *hits_dev, void *query_stream) {
    return query_dev(c, "srt_intersect_rays_dev", rays_dev, n, hits_dev, false, query_stream);
}
int srt_occluded_rays_dev(srt_ctx *c, const float *rays_dev, size_t n, uint8_t *occluded_dev, void *query_stream) {
    return query_dev(c, "srt_occluded_rays_dev", rays_dev, n, occluded_dev, true, query_stream);
}

int srt_query_last(srt_ctx *c, srt_query_info *info) {
    if (!c || !info) return fail(c, SRT_ERR_INVALID, "srt_query_last: null argument");
    if (!c->query_timed) return fail(c, SRT_ERR_INVALID, "srt_query_last: no query kernel has run on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->query_ev[1]));
    *info = c->query_info;
    HIP_TRY(c, hipEventElapsedTime(&info->ms, c->query_ev[0], c->query_ev[1]));
    return SRT_OK;
}

int srt_set_query_test_grid(srt_ctx *c, uint32_t max_waves) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_set_query_test_grid: null ctx");
    c->query_max_waves = max_waves;
    return SRT_OK;
}

// ---- direct lighting (srt_light.hip; srt_c_api.h, "Direct lighting") ----------------------------------------------------------------
namespace {

constexpr uint32_t kLightDraws = 1u << 24;                       // N: the 24-bit draw
constexpr size_t kLightRowBytes = 32 + 16 + 32 + 32 + 16 + 2;    // camera row, hit row, two shadow rows, record, two occlusion bytes
constexpr size_t kLightBudgetBytes = 320u << 20;                  // the working buffers of a round stay under this (one sample at least)

// The round's working buffers: [cam: 2 float4 per row][hits: 1][light rows: 2][sky rows: 2][records: 1 uint4][occ_light][occ_sky]
struct LightWork {
    float4 *cam, *hits, *light_rows, *sky_rows;
    uint4 *records;
    uint8_t *occ_light, *occ_sky;
    static size_t bytes(size_t rows) { return rows * 128 + 2 * ((rows + 15) & ~(size_t)15); }
    LightWork(const DeviceBuffer &d, size_t rows)
        : cam(d.as<float4>()), hits(cam + 2 * rows), light_rows(hits + rows), sky_rows(light_rows + 2 * rows),
          records(reinterpret_cast<uint4 *>(sky_rows + 2 * rows)), occ_light(reinterpret_cast<uint8_t *>(records + rows)),
          occ_sky(occ_light + ((rows + 15) & ~(size_t)15)) {}
};
// The call's outputs: [counters: 8 u64][sum: 3 floats per pixel][m2: 3 per pixel]
struct LightOut {
    unsigned long long *counters;
    float *sum, *m2;
    static size_t bytes(size_t npix) { return 64 + 24 * npix; }
    LightOut(const DeviceBuffer &d, size_t npix) : counters(d.as<unsigned long long>()), sum(reinterpret_cast<float *>(d.as<char>() + 64)), m2(sum + 3 * npix) {}
};
// The tables: [thresholds: L + 1 words, padded to 16 bytes][records: 16 floats per light][t_light][t_sky][t_emit]
struct LightTables {
    uint32_t *thresholds;
    float *records, *t_light, *t_sky, *t_emit;
    static size_t head(size_t lights) { return ((lights + 1) * 4 + 15) & ~(size_t)15; }
    static size_t bytes(size_t lights, size_t mats, size_t slots) { return head(lights) + 4 * (16 * lights + 3 * mats * slots + 6 * mats) + 16; }
    LightTables(const DeviceBuffer &d, size_t lights, size_t mats, size_t slots)
        : thresholds(d.as<uint32_t>()), records(reinterpret_cast<float *>(d.as<char>() + head(lights))), t_light(records + 16 * lights),
          t_sky(t_light + 3 * mats * slots), t_emit(t_sky + 3 * mats) {}
};

// integral over [360, 830] of cmf[ch] a b (linear interpolants on the 5 nm grid; a null factor is 1): Simpson's rule per cell, in double
void light_integral(const float *cmf96x4, const float *a, const float *b, float out[3]) {
    for (int ch = 0; ch < 3; ch++) {
        double acc = 0.0;
        for (int j = 0; j + 1 < SRT_N_CIE_SAMPLES; j++) {
            const double c0 = cmf96x4[4 * j + ch], c1 = cmf96x4[4 * (j + 1) + ch];
            const double a0 = a ? (double)a[j] : 1.0, a1 = a ? (double)a[j + 1] : 1.0;
            const double b0 = b ? (double)b[j] : 1.0, b1 = b ? (double)b[j + 1] : 1.0;
            const double fa = (c0 * a0) * b0, fb = (c1 * a1) * b1;
            const double fm = (((c0 + c1) * 0.5) * ((a0 + a1) * 0.5)) * ((b0 + b1) * 0.5);
            acc += ((fa + 4.0 * fm) + fb) * (5.0 / 6.0);
        }
        out[ch] = (float)acc;
    }
}

// the host tables of the uploaded scene; SRT_ERR_UNSUPPORTED above 2^20 lights
int build_light_tables(srt_ctx *c, const char *who) {
    if (c->light_tables_ok) return SRT_OK;
    std::vector<float> cmf(96 * 4);
    cmf_rows(cmf.data());
    const size_t n_mats = c->light_mats.size();
    std::vector<float> t_emit(3 * n_mats), t_sky(3 * n_mats);
    for (size_t m = 0; m < n_mats; m++) {
        light_integral(cmf.data(), c->light_mats[m].spectral_distribution, nullptr, &t_emit[3 * m]);
        light_integral(cmf.data(), c->light_mats[m].spectral_distribution, c->light_bg, &t_sky[3 * m]);
    }
    float t_bg[3];
    light_integral(cmf.data(), c->light_bg, nullptr, t_bg);
    bool bg_nonzero = false;
    for (float v : c->light_bg) bg_nonzero |= v != 0.0f;
    // the table's lights: area > 0 and T_emit.y > 0
    std::vector<float> rec;
    std::vector<double> g;
    std::vector<uint32_t> slot_mat;
    for (const srt_ctx::LightSource &l : c->light_src) {
        float e1[3], e2[3];
        for (int k = 0; k < 3; k++) { e1[k] = l.v1[k] - l.v0[k]; e2[k] = l.v2[k] - l.v0[k]; }
        const double cx = (double)e1[1] * (double)e2[2] - (double)e1[2] * (double)e2[1];
        const double cy = (double)e1[2] * (double)e2[0] - (double)e1[0] * (double)e2[2];
        const double cz = (double)e1[0] * (double)e2[1] - (double)e1[1] * (double)e2[0];
        const float area = (float)(0.5 * std::sqrt((cx * cx + cy * cy) + cz * cz));
        const float ty = t_emit[3 * l.mat + 1];
        if (!(area > 0.0f) || !(ty > 0.0f)) continue;
        size_t slot = std::find(slot_mat.begin(), slot_mat.end(), l.mat) - slot_mat.begin();
        if (slot == slot_mat.size()) slot_mat.push_back(l.mat);
        const uint32_t words[3] = {l.mat, l.tri, (uint32_t)slot};
        const float *rows[4] = {l.v0, e1, e2, l.n};
        for (int r = 0; r < 4; r++) {
            rec.insert(rec.end(), rows[r], rows[r] + 3);
            float last = area;
            if (r > 0) memcpy(&last, &words[r - 1], 4);
            rec.push_back(last);
        }
        g.push_back((double)area * (double)ty);
    }
    const size_t L = g.size();
    if (L > (size_t)SRT_LIGHT_MAX_LIGHTS) return fail(c, SRT_ERR_UNSUPPORTED, std::string(who) + ": more than 2^20 lights");
    // thresholds by largest remainder, every light at least 1 wide
    std::vector<uint32_t> th(L + 1, 0u);
    if (L > 0) {
        std::vector<char> pinned(L, 0);
        size_t n_pinned = 0;
        double G = 0.0, B = 0.0;
        for (;;) {
            G = 0.0;
            for (size_t l = 0; l < L; l++) if (!pinned[l]) G += g[l];
            B = (double)(kLightDraws - n_pinned);
            bool changed = false;
            for (size_t l = 0; l < L; l++)
                if (!pinned[l] && g[l] / G * B < 1.0) { pinned[l] = 1; n_pinned++; changed = true; }
            if (!changed) break;
        }
        std::vector<uint32_t> width(L, 1u);
        std::vector<double> rem(L, -1.0);
        std::vector<uint32_t> order;
        uint64_t given = n_pinned;
        for (size_t l = 0; l < L; l++) {
            if (pinned[l]) continue;
            const double ideal = g[l] / G * B, fl = std::floor(ideal);
            width[l] = (uint32_t)fl; rem[l] = ideal - fl; given += width[l];
            order.push_back((uint32_t)l);
        }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rem[a] > rem[b]; });
        for (size_t k = 0; given < kLightDraws && !order.empty(); k++, given++) width[order[k % order.size()]]++;
        for (size_t l = 0; l < L; l++) th[l + 1] = th[l] + width[l];
        if (th[L] != kLightDraws) return fail(c, SRT_ERR_INVALID, std::string(who) + ": the light thresholds do not add up (internal error)");
    }
    const size_t n_slots = slot_mat.size();
    std::vector<float> t_light(3 * n_mats * n_slots);
    for (size_t m = 0; m < n_mats; m++)
        for (size_t s = 0; s < n_slots; s++)
            light_integral(cmf.data(), c->light_mats[m].spectral_distribution, c->light_mats[slot_mat[s]].spectral_distribution, &t_light[3 * (m * n_slots + s)]);
    c->light_thresholds.swap(th); c->light_records.swap(rec);
    c->light_t_light.swap(t_light); c->light_t_sky.swap(t_sky); c->light_t_emit.swap(t_emit);
    memcpy(c->light_t_bg, t_bg, sizeof(t_bg));
    c->light_slots = (uint32_t)n_slots; c->light_bg_nonzero = bg_nonzero;
    c->light_tables_ok = true; c->light_tables_on_device = false;
    return SRT_OK;
}

int light_tables_to_device(srt_ctx *c, const char *who) {
    if (c->light_tables_on_device) return SRT_OK;
    const size_t L = c->light_thresholds.size() - 1, mats = c->light_mats.size(), slots = c->light_slots;
    if (const int rc = develop_reserve(c, who, c->d_light_tab, LightTables::bytes(L, mats, slots))) return rc;
    const LightTables T(c->d_light_tab, L, mats, slots);
    auto put = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess; };
    HIP_TRY_AS(c, who, put(T.thresholds, c->light_thresholds.data(), (L + 1) * 4));
    HIP_TRY_AS(c, who, put(T.records, c->light_records.data(), c->light_records.size() * 4));
    HIP_TRY_AS(c, who, put(T.t_light, c->light_t_light.data(), c->light_t_light.size() * 4));
    HIP_TRY_AS(c, who, put(T.t_sky, c->light_t_sky.data(), c->light_t_sky.size() * 4));
    HIP_TRY_AS(c, who, put(T.t_emit, c->light_t_emit.data(), c->light_t_emit.size() * 4));
    c->light_tables_on_device = true;
    return SRT_OK;
}

struct LightKat { float *cam_rows, *hit_rows, *light_rows, *sky_rows; uint32_t *records; uint8_t *occ_light, *occ_sky; };

int direct_light_run(srt_ctx *c, const char *who, const srt_light *cfg, float *out_sum, float *out_m2, srt_light_result *result, uint32_t w,
                     uint32_t h, uint32_t ox, uint32_t oy, const LightKat *kat) {
    if (!c) return fail(c, SRT_ERR_INVALID, std::string(who) + ": null ctx");
    auto refuse = [&](const char *why) { return fail(c, SRT_ERR_INVALID, std::string(who) + ": " + why); };
    if (!cfg || !out_sum || !result) return refuse("null argument");
    if (!c->scene_ready) return refuse("no scene uploaded");
    if (!c->camera_ready) return refuse("no camera set");
    if (cfg->samples < 1 || cfg->samples > SRT_LIGHT_MAX_SAMPLES) return refuse("samples outside 1 .. 65536");
    if (kat && cfg->samples != 1) return refuse("the KAT entry runs one sample");
    const uint32_t all_parts = SRT_LIGHT_EMITTED | SRT_LIGHT_LIGHTS | SRT_LIGHT_SKY;
    if (cfg->parts == 0 || (cfg->parts & ~all_parts)) return refuse("parts is 0 or has unknown bits");
    if ((uint64_t)cfg->first_sample + cfg->samples > (1ull << 32)) return refuse("first_sample + samples does not fit 32 bits");
    if (w == 0 || h == 0) return refuse("empty rectangle");
    if ((uint64_t)ox + w > c->cam.width || (uint64_t)oy + h > c->cam.height) return refuse("the rectangle sticks out of the camera's image");
    if ((uint64_t)w * h > (1ull << 28)) return refuse("more than 2^28 pixels");
    if ((cfg->parts & SRT_LIGHT_LIGHTS) && c->light_refitted)
        return fail(c, SRT_ERR_UNSUPPORTED, std::string(who) + ": LIGHTS on a scene refitted since its upload (the light table's areas are stale)");
    if (const int rc = build_light_tables(c, who)) return rc;
    HIP_TRY_AS(c, who, set_device(c));
    if (const int rc = light_tables_to_device(c, who)) return rc;
    const size_t L = c->light_thresholds.size() - 1, mats = c->light_mats.size(), slots = c->light_slots;
    const LightTables T(c->d_light_tab, L, mats, slots);
    const bool lights_on = (cfg->parts & SRT_LIGHT_LIGHTS) && L > 0, sky_on = (cfg->parts & SRT_LIGHT_SKY) && c->light_bg_nonzero;
    const uint32_t parts = (cfg->parts & SRT_LIGHT_EMITTED) | (lights_on ? SRT_LIGHT_LIGHTS : 0u) | (sky_on ? SRT_LIGHT_SKY : 0u);
    const size_t npix = (size_t)w * h;
    const size_t max_rows = c->light_max_rows ? (size_t)c->light_max_rows : kLightBudgetBytes / kLightRowBytes;
    const uint32_t per_round = (uint32_t)std::max<size_t>(1, std::min<size_t>(cfg->samples, max_rows / npix));
    const size_t rows_cap = npix * per_round;
    if (rows_cap > (size_t)SRT_QUERY_MAX_RAYS) return refuse("a round of one sample has more rows than a query launch takes");
    if (const int rc = develop_reserve(c, who, c->d_light_work, LightWork::bytes(rows_cap))) return rc;
    if (const int rc = develop_reserve(c, who, c->d_light_out, LightOut::bytes(npix))) return rc;
    for (hipEvent_t &e : c->light_ev) if (!e) HIP_TRY_AS(c, who, hipEventCreate(&e));
    const LightWork W(c->d_light_work, rows_cap);
    const LightOut O(c->d_light_out, npix);
    HIP_TRY_AS(c, who, hipMemsetAsync(c->d_light_out.ptr, 0, LightOut::bytes(npix), nullptr));
    LightCamera cam;
    memcpy(cam.du, c->cam.pixel_delta_u, 12); memcpy(cam.dv, c->cam.pixel_delta_v, 12); memcpy(cam.p00, c->cam.pixel00_loc, 12);
    memcpy(cam.center, c->cam.camera_center, 12); memcpy(cam.disk_u, c->cam.defocus_disk_u, 12); memcpy(cam.disk_v, c->cam.defocus_disk_v, 12);
    cam.defocus_angle = c->cam.defocus_angle;
    c->light_timed = false;
    srt_light_info info = {};
    info.rows_per_round = (uint32_t)std::min<size_t>(rows_cap, 0xffffffffu);
    for (uint32_t done = 0; done < cfg->samples; done += per_round) {
        LightRound r;
        r.w = w; r.h = h; r.ox = ox; r.oy = oy; r.image_w = c->cam.width;
        r.n_samples = std::min(per_round, cfg->samples - done); r.first_sample = cfg->first_sample + done;
        r.seed_lo = (uint32_t)cfg->seed; r.seed_hi = (uint32_t)(cfg->seed >> 32); r.parts = parts;
        const size_t rows = npix * r.n_samples;
        HIP_TRY_AS(c, who, hipEventRecord(c->light_ev[0], nullptr));
        HIP_TRY_AS(c, who, launch_light_camera(r, cam, W.cam, nullptr));
        HIP_TRY_AS(c, who, hipEventRecord(c->light_ev[1], nullptr));
        if (const int rc = query_enqueue(c, who, reinterpret_cast<const float *>(W.cam), rows, W.hits, false, nullptr)) return rc;
        HIP_TRY_AS(c, who, hipEventRecord(c->light_ev[2], nullptr));
        LightShadeParams sp = {};
        sp.r = r; sp.cam_rows = W.cam; sp.hits = W.hits; sp.shade = c->d_shade.as<const float4>(); sp.n_tris = c->n_tris;
        sp.thresholds = T.thresholds; sp.lights = reinterpret_cast<const float4 *>(T.records); sp.n_lights = (uint32_t)L;
        sp.light_rows = lights_on ? W.light_rows : nullptr; sp.sky_rows = sky_on ? W.sky_rows : nullptr; sp.records = W.records;
        HIP_TRY_AS(c, who, launch_light_shade(sp, nullptr));
        HIP_TRY_AS(c, who, hipEventRecord(c->light_ev[3], nullptr));
        if (lights_on) if (const int rc = query_enqueue(c, who, reinterpret_cast<const float *>(W.light_rows), rows, W.occ_light, true, nullptr)) return rc;
        if (sky_on) if (const int rc = query_enqueue(c, who, reinterpret_cast<const float *>(W.sky_rows), rows, W.occ_sky, true, nullptr)) return rc;
        HIP_TRY_AS(c, who, hipEventRecord(c->light_ev[4], nullptr));
        LightGatherParams gp = {};
        gp.r = r; gp.records = W.records; gp.occ_light = lights_on ? W.occ_light : nullptr; gp.occ_sky = sky_on ? W.occ_sky : nullptr;
        gp.lights = reinterpret_cast<const float4 *>(T.records); gp.t_light = T.t_light; gp.t_sky = T.t_sky; gp.t_emit = T.t_emit;
        memcpy(gp.t_bg, c->light_t_bg, sizeof(gp.t_bg));
        gp.n_materials = (uint32_t)mats; gp.n_slots = (uint32_t)slots;
        gp.sum = O.sum; gp.m2 = out_m2 ? O.m2 : nullptr; gp.counters = O.counters;
        HIP_TRY_AS(c, who, launch_light_gather(gp, nullptr));
        HIP_TRY_AS(c, who, hipEventRecord(c->light_ev[5], nullptr));
        HIP_TRY_AS(c, who, device_synchronize(c));
        float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 5; k++) HIP_TRY_AS(c, who, hipEventElapsedTime(&ms[k], c->light_ev[k], c->light_ev[k + 1]));
        info.camera_ms += ms[0]; info.query_ms += ms[1] + ms[3]; info.shade_ms += ms[2]; info.gather_ms += ms[4];
        info.rounds++; info.query_launches += 1u + (lights_on ? 1u : 0u) + (sky_on ? 1u : 0u);
        if (kat) {
            auto get = [&](void *dst, const void *src, size_t bytes, bool valid) {
                if (!dst) return hipSuccess;
                if (!valid) { memset(dst, 0, bytes); return hipSuccess; }
                return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
            };
            HIP_TRY_AS(c, who, get(kat->cam_rows, W.cam, 32 * rows, true));
            HIP_TRY_AS(c, who, get(kat->hit_rows, W.hits, 16 * rows, true));
            HIP_TRY_AS(c, who, get(kat->light_rows, W.light_rows, 32 * rows, lights_on));
            HIP_TRY_AS(c, who, get(kat->sky_rows, W.sky_rows, 32 * rows, sky_on));
            HIP_TRY_AS(c, who, get(kat->records, W.records, 16 * rows, true));
            HIP_TRY_AS(c, who, get(kat->occ_light, W.occ_light, rows, lights_on));
            HIP_TRY_AS(c, who, get(kat->occ_sky, W.occ_sky, rows, sky_on));
        }
    }
    unsigned long long counts[kLightCounters];
    HIP_TRY_AS(c, who, hipMemcpy(counts, O.counters, sizeof(counts), hipMemcpyDeviceToHost));
    HIP_TRY_AS(c, who, hipMemcpy(out_sum, O.sum, 12 * npix, hipMemcpyDeviceToHost));
    if (out_m2) HIP_TRY_AS(c, who, hipMemcpy(out_m2, O.m2, 12 * npix, hipMemcpyDeviceToHost));
    srt_light_result res = {};
    res.miss = counts[0]; res.emitted = counts[1]; res.specular = counts[2]; res.shaded = counts[3];
    res.light_rows = counts[4]; res.light_unoccluded = counts[5]; res.sky_rows = counts[6]; res.sky_unoccluded = counts[7];
    res.lights = (uint32_t)L;
    *result = res;
    c->light_info = info; c->light_timed = true;
    return SRT_OK;
}

}  // namespace

int srt_direct_light(srt_ctx *c, const srt_light *cfg, float *out_sum, float *out_m2, srt_light_result *result, uint32_t w, uint32_t h,
                     uint32_t ox, uint32_t oy) {
    return direct_light_run(c, "srt_direct_light", cfg, out_sum, out_m2, result, w, h, ox, oy, nullptr);
}

int srt_direct_light_kat(srt_ctx *c, const srt_light *cfg, float *out_sum, float *out_m2, srt_light_result *result, uint32_t w, uint32_t h,
                         uint32_t ox, uint32_t oy, float *cam_rows, float *hit_rows, float *light_rows, float *sky_rows, uint32_t *records,
                         uint8_t *occ_light, uint8_t *occ_sky) {
    const LightKat kat = {cam_rows, hit_rows, light_rows, sky_rows, records, occ_light, occ_sky};
    return direct_light_run(c, "srt_direct_light_kat", cfg, out_sum, out_m2, result, w, h, ox, oy, &kat);
}

int srt_read_light_table(srt_ctx *c, uint32_t *n_lights, uint32_t *thresholds, float *records, size_t cap) {
    if (!c || !n_lights) return fail(c, SRT_ERR_INVALID, "srt_read_light_table: null argument");
    if (!c->scene_ready) return fail(c, SRT_ERR_INVALID, "srt_read_light_table: no scene uploaded");
    if (const int rc = build_light_tables(c, "srt_read_light_table")) return rc;
    const size_t L = c->light_thresholds.size() - 1;
    *n_lights = (uint32_t)L;
    if ((thresholds || records) && cap < L) return fail(c, SRT_ERR_INVALID, "srt_read_light_table: cap is smaller than the table");
    if (thresholds) memcpy(thresholds, c->light_thresholds.data(), (L + 1) * sizeof(uint32_t));
    if (records && L) memcpy(records, c->light_records.data(), 16 * L * sizeof(float));
    return SRT_OK;
}

int srt_direct_light_last(srt_ctx *c, srt_light_info *info) {
    if (!c || !info) return fail(c, SRT_ERR_INVALID, "srt_direct_light_last: null argument");
    if (!c->light_timed) return fail(c, SRT_ERR_INVALID, "srt_direct_light_last: no direct-light call has run on this context");
    *info = c->light_info;
    return SRT_OK;
}

int srt_set_light_test_batch(srt_ctx *c, uint32_t max_rows) {
    if (!c) return fail(c, SRT_ERR_INVALID, "srt_set_light_test_batch: null ctx");
    c->light_max_rows = max_rows;
    return SRT_OK;
}

int srt_device_op_sweep(srt_ctx *c, int which, const float *a, const float *b, size_t n, float *out) {
    if (!c || !a || !b || !out) return fail(c, SRT_ERR_INVALID, "srt_device_op_sweep: null argument");
    if (n == 0) return SRT_OK;
    HIP_TRY(c, set_device(c));
    DeviceBuffer buf;      // a | b | out
    HIP_TRY_AS(c, "srt_device_op_sweep", buf.reserve(3 * n * sizeof(float)));
    float *d = buf.as<float>();
    HIP_TRY_AS(c, "srt_device_op_sweep", hipMemcpy(d, a, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, "srt_device_op_sweep", hipMemcpy(d + n, b, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, "srt_device_op_sweep", launch_op_sweep(which, d, d + n, n, d + 2 * n, nullptr));
    HIP_TRY_AS(c, "srt_device_op_sweep", device_synchronize(c));
    HIP_TRY_AS(c, "srt_device_op_sweep", hipMemcpy(out, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return SRT_OK;
}

int srt_order_tiles_kat(srt_ctx *c, const uint32_t *cost, uint32_t n, uint32_t n_waves, uint32_t split_load_pct, uint32_t order_max_pct,
                        uint32_t *rows_out, size_t rows_cap, uint32_t *sorted_out, uint32_t *info_out) {
    if (!c || !cost || !rows_out || !sorted_out || !info_out) return fail(c, SRT_ERR_INVALID, "srt_order_tiles_kat: null argument");
    // (beyond 2^20 tiles the kernel must not split; one that wrongly did would write past any buffer sized for what it should do)
    if (n == 0 || n > (1u << 20)) return fail(c, SRT_ERR_INVALID, "srt_order_tiles_kat: n must be in 1 .. 2^20");
    if (rows_cap < (size_t)n * 64 + 64) return fail(c, SRT_ERR_INVALID, "srt_order_tiles_kat: rows_cap must be at least 64 * n + 64 (the largest queue and 64 guard words)");
    HIP_TRY(c, set_device(c));
    DeviceBuffer d_cost, d_rows, d_sorted, d_info;
    HIP_TRY_AS(c, "srt_order_tiles_kat", d_cost.reserve(TileSchedule::cost_bytes(n)));
    HIP_TRY_AS(c, "srt_order_tiles_kat", d_rows.reserve(rows_cap * sizeof(uint32_t)));
    HIP_TRY_AS(c, "srt_order_tiles_kat", d_sorted.reserve(n * sizeof(uint32_t)));
    HIP_TRY_AS(c, "srt_order_tiles_kat", d_info.reserve(4 * sizeof(uint32_t)));
    HIP_TRY_AS(c, "srt_order_tiles_kat", hipMemcpy(d_cost.ptr, cost, TileSchedule::cost_bytes(n), hipMemcpyHostToDevice));
    HIP_TRY_AS(c, "srt_order_tiles_kat", hipMemset(d_rows.ptr, 0xff, rows_cap * sizeof(uint32_t)));      // unwritten words stay visible
    HIP_TRY_AS(c, "srt_order_tiles_kat", hipMemset(d_sorted.ptr, 0xff, n * sizeof(uint32_t)));
    HIP_TRY_AS(c, "srt_order_tiles_kat", hipMemset(d_info.ptr, 0xff, 4 * sizeof(uint32_t)));
    HIP_TRY_AS(c, "srt_order_tiles_kat", launch_order_tiles(d_cost.as<uint32_t>(), d_sorted.as<uint32_t>(), d_rows.as<uint32_t>(), n, n_waves, split_load_pct,
                                                            d_info.as<uint32_t>(), order_max_pct, nullptr));
    HIP_TRY_AS(c, "srt_order_tiles_kat", device_synchronize(c));
    HIP_TRY_AS(c, "srt_order_tiles_kat", hipMemcpy(rows_out, d_rows.ptr, rows_cap * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY_AS(c, "srt_order_tiles_kat", hipMemcpy(sorted_out, d_sorted.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY_AS(c, "srt_order_tiles_kat", hipMemcpy(info_out, d_info.ptr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SRT_OK;
}

int srt_read_tile_schedule(srt_ctx *c, int which, uint32_t *rows_out, size_t rows_cap, srt_tile_schedule_info *info) {
    if (!c || !info || (!rows_out && rows_cap) || (which != 0 && which != 1)) return fail(c, SRT_ERR_INVALID, "srt_read_tile_schedule: bad argument");
    if (which == 0 ? !c->sched_probe_queue : !c->sched_compacted_queue)
        return fail(c, SRT_ERR_INVALID, which == 0 ? "srt_read_tile_schedule: the last launch ran no cost probe's queue (no probe, or too few samples or tiles for one)"
                                                   : "srt_read_tile_schedule: the last launch was no adaptive pass: no compacted queue");
    if (const int rc = srt_synchronize(c)) return rc;
    const uint32_t *d_rows = which == 0 ? TileSchedule(c).rows : AdaptQueue(c->d_adapt_queue).rows;
    const uint32_t *d_info = which == 0 ? TileSchedule(c).info : AdaptQueue(c->d_adapt_queue).info;
    uint32_t head[2] = {0u, 0u};      // queue_info: rows, the largest tile cost
    HIP_TRY(c, hipMemcpy(head, d_info, sizeof(head), hipMemcpyDeviceToHost));
    // (a compacted queue of an accumulation that runs unordered has the identity order as its source: no probe, nothing noted)
    srt_tile_schedule_info out = c->sched_probe_queue ? c->sched_note : srt_tile_schedule_info{};
    if (!c->sched_probe_queue) { out.tiles_local = c->tiles_local; out.streams = 1u; }
    out.n_rows = head[0]; out.cost_max = head[1];
    if (rows_cap < out.n_rows) return fail(c, SRT_ERR_INVALID, "srt_read_tile_schedule: rows_cap is smaller than the queue");
    if (out.n_rows) HIP_TRY(c, hipMemcpy(rows_out, d_rows, (size_t)out.n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *info = out;
    return SRT_OK;
}

int srt_calibrate(srt_ctx *c, int kind, uint32_t waves_per_simd, uint32_t iters, srt_calibration *out) {
    if (!c || !out || kind < 0 || kind >= calib_kinds() || waves_per_simd < 1 || waves_per_simd > 4 || iters == 0)
        return fail(c, SRT_ERR_INVALID, "srt_calibrate: bad argument");
    HIP_TRY(c, set_device(c));
    const uint32_t threads = waves_per_simd * 256u, n_blocks = (uint32_t)c->n_cu, n_waves = n_blocks * threads / 64u;
    DeviceBuffer d_cyc, d_sink, d_table;
    HIP_TRY_AS(c, "srt_calibrate", d_cyc.reserve(n_waves * sizeof(unsigned long long)));
    HIP_TRY_AS(c, "srt_calibrate", d_sink.reserve(1024 * sizeof(float)));
    // kinds 11+: a 16 MB table of 64-byte records (the size of the 100k-triangle mesh's tree: served by L2 / MALL)
    const uint32_t n_table = 1u << 18;
    if (kind >= 11) {
        HIP_TRY_AS(c, "srt_calibrate", d_table.reserve((size_t)n_table * 64));
        HIP_TRY_AS(c, "srt_calibrate", hipMemset(d_table.ptr, 0, (size_t)n_table * 64));
    }
    struct Event { hipEvent_t ev = nullptr; ~Event() { if (ev) (void)hipEventDestroy(ev); } } e0, e1;
    HIP_TRY_AS(c, "srt_calibrate", hipEventCreate(&e0.ev));
    HIP_TRY_AS(c, "srt_calibrate", hipEventCreate(&e1.ev));
    HIP_TRY_AS(c, "srt_calibrate", launch_calib(kind, n_blocks, threads, iters / 8u + 1u, d_sink.as<float>(), d_cyc.as<unsigned long long>(), d_table.as<float4>(), n_table, nullptr));   // warm-up (clocks, code)
    HIP_TRY_AS(c, "srt_calibrate", hipEventRecord(e0.ev, nullptr));
    HIP_TRY_AS(c, "srt_calibrate", launch_calib(kind, n_blocks, threads, iters, d_sink.as<float>(), d_cyc.as<unsigned long long>(), d_table.as<float4>(), n_table, nullptr));
    HIP_TRY_AS(c, "srt_calibrate", hipEventRecord(e1.ev, nullptr));
    HIP_TRY_AS(c, "srt_calibrate", hipEventSynchronize(e1.ev));
    float ms = 0.f;
    HIP_TRY_AS(c, "srt_calibrate", hipEventElapsedTime(&ms, e0.ev, e1.ev));
    std::vector<unsigned long long> h(n_waves);
    HIP_TRY_AS(c, "srt_calibrate", hipMemcpy(h.data(), d_cyc.ptr, n_waves * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double sum = 0, mx = 0, mn = 1e300;
    for (unsigned long long v : h) { sum += (double)v; mx = std::max(mx, (double)v); mn = std::min(mn, (double)v); }
    memset(out, 0, sizeof(*out));
    out->wave_cycles_mean = sum / n_waves; out->wave_cycles_max = mx; out->wave_cycles_min = mn; out->wall_ms = ms;
    out->instr_per_wave = (uint64_t)iters * 32u;
    out->n_waves = n_waves; out->n_cu = n_blocks; out->waves_per_simd = waves_per_simd;
    return SRT_OK;
}

}  // extern "C"
