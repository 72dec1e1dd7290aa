// srt_internal.h -- shared between the C-ABI implementation (srt_capi.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

struct srt_ctx;
extern "C" int srt_internal_init_device_params(srt_ctx *c, uint32_t tx, uint32_t ty, uint32_t bx, uint32_t by, uint32_t chunk_w, uint32_t chunk_h,
                                               uint32_t spp, uint32_t bounce_limit, uint64_t seed, int wait);      // not exported (hidden visibility)

// srt_refit_vertices; scanned != 0: the caller has already found every coordinate finite (a communicator scans once for all its contexts)
extern "C" int srt_internal_refit_vertices(srt_ctx *c, const float *verts, size_t n_tris, int scanned);
extern "C" uint32_t srt_internal_gather_planes(const srt_ctx *c);      // planes of the context's exchange unit (3 or 9); not exported

// srt_comm_gather_accum's view of a context (not exported).  The descriptor is what the ranks must agree on before anybody packs: [0] 1
// when srt_pack_accum(ctx, parts) would be accepted, [1] the accumulation's kind, [2] its total, [3] its streams, [4] .. [7] w, h, offx, offy
// of its chunk, [8] the parts resolved against the kind, [9] and [10] the low and the high word of the floats of its exchange unit, [11] 0.
// It never fails: a context that would refuse says so in word 0 and the others see it.
constexpr int kGatherDescriptorWords = 12;
extern "C" void srt_internal_gather_descriptor(const srt_ctx *c, uint32_t parts, uint32_t out[kGatherDescriptorWords]);
// the buffer srt_internal_pack_accum_own packs into, grown to n_floats: called BEFORE the ranks agree, so that a failed allocation is one
// more thing a rank says in word 0 of its descriptor
extern "C" int srt_internal_gather_reserve(srt_ctx *c, size_t n_floats);
// srt_pack_accum into a buffer the context owns (grown as needed); *unit_dev / *n_floats: where the unit lies and its size
extern "C" int srt_internal_pack_accum_own(srt_ctx *c, uint32_t parts, void *stream, void **unit_dev, size_t *n_floats);

namespace srt {

constexpr int kTilePlanes = 9;      // quantised rgb | unquantised sRGB | XYZ sums
constexpr int kTileGroups = 3;      // ... in three groups of three planes; group 0 (the quantised framebuffer) is what the multi-GPU gather moves
constexpr int kGroupPlanes = 3;
constexpr int kTileLanes = 64;      // one wave = one 8x8 pixel tile
constexpr int kCounters = 32;       // rays, node_visits, tri_tests, box_tests, utilisation counters (instrumented build); [23] queue invariant, [24] hits

// Row of a launch's pixel queue: local tile | part << 22 | level << 28 (queue_row_pack, srt_kernel_common.h).  A rank whose local tiles
// do not fit the tile field renders unordered: without a queue the row IS the local tile.
constexpr uint32_t kQueueTileBits = 22, kQueueTileMask = (1u << kQueueTileBits) - 1u;
constexpr uint32_t kQueuePartShift = kQueueTileBits, kQueuePartMask = 63u;
constexpr uint32_t kQueueLevelShift = 28, kQueueLevelMask = 7u;

// Kernel arguments of one render launch.  All pointers are device pointers.
struct RenderParams {
    // scene (HBM layout: DESIGN.md)
    const float4 *nodes;       // 4 float4 per INNER record (records [0, n_inner))
    const float *nodes_sw;     // 20 floats per INNER record, pre-swizzled (srt_host.cpp, flatten_scene); null when the tree is LDS resident
    const float4 *fringe;      // 6 float4 per FRINGE record (records [n_inner, n_records)), triangle data inline
    const float4 *tris;        // 3 float4 per triangle
    const float2 *mat_sd;      // per material 96 pairs (94 used): (sd[k], sd[k+1]); table n_materials = the background
    const float4 *shade;       // 3 float4 per triangle: {n, bits(mat)} {bits(type), fuzz, B0, B1} {B2, C0, C1, C2}
    const float4 *mat_par;     // per material 2 float4: {bits(type), fuzz, B0, B1}, {B2, C0, C1, C2}
    const float4 *cmf;         // 96 rows (95 used): { x_bar, y_bar, z_bar, D65n }
    int root_ref;              // >= 0 record index, < 0: ~triangle (single-leaf tree)
    int stack_depth;           // LDS stack entries per lane
    int n_inner;               // records below this index have two internal children (box tests only)
    int n_cached;              // records below this index are resident in LDS (top of the tree)
    int n_records;             // number of paired-child records
    uint32_t fringe_stride;    // bytes between two FRINGE records: 96 (packed) or 128 (one cache line each: trees served by L2)
    uint32_t n_materials;
    uint32_t n_tris;
    uint32_t paired;           // host side only (the launcher's choice of variant): the tree has no node with exactly one leaf child
    // camera_data (rendering/rendering.cuh:28-36)
    float du[3], dv[3], p00[3];
    float defocus_angle;
    float center[3], disk_u[3], disk_v[3];
    // launch geometry
    uint32_t width, height, offx, offy;   // chunk (rendering.cu:153)
    uint32_t tx, ty, bx, by;              // the reference's block / grid dims: define idx and the RNG seed
    uint32_t spp, bounce_limit;
    uint32_t tiles_x, tiles_y, n_tiles;   // 8x8 tiles covering the chunk
    uint32_t rank, world;                 // this launch renders tiles t with t % world == rank
    uint32_t tiles_local;                 // number of tiles this rank owns (pixel queue length / 64)
    uint32_t *pixel_counter;              // device word, zeroed before the launch: head of the pixel queue
    const uint32_t *tile_order;           // optional: queue slot -> local tile (cost-descending order); null = identity
    uint32_t *tile_cost;                  // probe mode: [0, tiles_local) per local tile, node records visited by its pixels; [tiles_local, 2 tiles_local) its most expensive pixel
    const uint32_t *queue_rows;           // optional: [0] = number of queue rows, [1] = the largest tile cost (device-written by order_tiles_kernel)
    const uint32_t *prio_cost;            // optional: the probe's per-tile cost, read by the render launch for its wave priorities
    uint32_t queue_rows_bound;            // host-side upper bound of the row count (= tiles_local without splitting)
    uint32_t waves_per_cu_override;       // 0 = occupancy API
    uint32_t score_shade, score_fringe;   // step-choice weights, 256 / relative step cost (both >= 1)
    uint32_t debug_lane_limit;            // experiments only (env SRT_DEBUG_LANE_LIMIT): lanes >= limit of every tile stay idle
    // state / outputs
    uint32_t *rng;                        // SoA: 6 planes of n_lanes words, indexed by the block-linear idx
    uint32_t n_lanes;                     // tx*ty*bx*by
    float *tile_out;                      // [group][local tile (tiles_padded of them)][plane of the group][lane]
    uint32_t tile_group_stride;           // floats between two groups = tiles_padded * 3 * 64
    uint32_t write_parity;                // 0: only group 0 (the reference's framebuffer values) is written; 1: + the two parity groups
    unsigned long long *counters;
    uint32_t *wave_debug;                 // instrumented build, optional: OrderProfile header, then 4 words per wave (see srt_get_wave_debug)
};

// Child-order profile of an instrumented launch (srt_order_children_by_profile): the pointers travel in a header IN FRONT of the
// per-wave words of RenderParams::wave_debug (this struct, then 4 words per launched wave) so that RenderParams -- the kernel argument
// of every variant -- stays as it is and the header's place does not depend on the number of waves a launch starts.  magic == kOrderProfileMagic marks a launch that collects the profile.
struct OrderProfile {
    unsigned long long magic;
    const int32_t *leaf;       // per triangle: node index of its leaf
    const int32_t *up;         // per node: parent node * 2 + (1 if the node is the right child), -1 for the root
    const float *sibbox;       // per node: the box of its sibling (xmin xmax ymin ymax zmin zmax)
    uint32_t *cnt;             // [parent * 2 + side]: closest hits found under that child while the sibling's box lay on the ray beyond the hit
    unsigned long long n_nodes;
    // Segment dump (srt_collect_ray_segments), independent of magic: seg != null marks a launch that samples its closest-hit queries.
    // Every finished query whose direction is not NaN takes a ticket from seg_tickets[0] (one wave-aggregated atomic); ticket t is
    // sampled when (t + seg_phase) % seg_stride == 0 and then owns slot (t + seg_phase) / seg_stride - (seg_phase ? 1 : 0) -- the number
    // of sampled tickets before it -- which it writes, when slot < seg_capacity, as two float4: (origin, dir.x) (dir.y, dir.z, t_end,
    // bits of the triangle found or -1).  t_end: the closest hit, FLT_MAX for a miss.
    float4 *seg;
    uint32_t *seg_tickets;
    uint32_t seg_stride, seg_phase;      // seg_stride >= 1, seg_phase < seg_stride
    unsigned long long seg_capacity;     // slots of seg
};
constexpr unsigned long long kOrderProfileMagic = 0x5352544f52444552ull;
constexpr uint32_t kSegmentFloats = 7;      // origin, direction, t_end: what the host calls exchange (the device slot has an eighth word)

// Accumulating launch (render_kernel MODE 3, srt_render_chunk_accum): RenderParams::wave_debug -- which no other production launch
// reads -- points at this header instead of the instrumented build's OrderProfile, so that RenderParams and with it the machine code of
// the plain production kernels stay as they are.  sums: three planes of n_lanes floats (X, Y, Z), indexed by the block-linear idx like
// the RNG planes; a pixel starts from its stored sum and stores it back when its samples of the pass are done.  spp_total: the samples
// per pixel the sums hold after this pass (the normalisation of the written framebuffer).
// Adaptive accumulations (MODE 4, srt_accum_reset_adaptive) read the fields behind `pad` as well: sum2, the plane of per-pixel sums of
// the squared per-sample luminance, and state, the plane of per-pixel state words (samples held | kAdaptConverged); the stopping
// criterion's parameters.  srt_accum_reset_adaptive writes them once; the per-pass kernel rewrites only sums and spp_total.
struct AccumHeader {
    float *sums;
    uint32_t spp_total;
    uint32_t pad;
    float *sum2;
    uint32_t *state;
    float rel_tol, abs_tol;
    uint32_t min_spp, pad2;
    float *film;
    uint32_t *stream_planes;
    uint32_t streams, pad3;
    float *features;
    const float *mat_col;
};
// Spectral accumulations (MODE 5, srt_accum_reset_spectral) read `film` as well: kFilmStride floats per lane of the grid, indexed by the
// block-linear idx, of which the first kFilmSamples are the raw sums on the CIE grid (360 + 5 j nm); srt_accum_reset_spectral writes it once.
// Streamed accumulations (MODE 6, srt_accum_reset_streams) read the two fields behind `film` instead: a pixel has `streams` = K RNG
// streams, and the launch's work item is (pixel, stream k).  stream_planes: nine planes of K * n_lanes words, entry idx' = k * n_lanes +
// idx of a plane belonging to stream k of lane idx -- planes 0 .. 5 its RNG state (except stream 0, which is the context's own state,
// RenderParams::rng: the k = 0 entries of these six planes are not used), planes 6 .. 8 (kStreamSumPlane) its XYZ sum.  MODE 6 writes no
// tile-buffer slot: stream_combine_kernel adds the K sums in stream order into `sums` and converts.  srt_accum_reset_streams writes the
// two fields once.
// Featured accumulations (MODE 7, srt_accum_reset_features) read the two fields behind `pad3` instead: features, kFeatureStride floats per
// lane of the grid indexed by the block-linear idx -- the raw first-hit sums [0..2] normal, [3..5] albedo, [6] distance, [7] hits -- and
// mat_col, the scene's per-material colour table (one float4 per material: srt_material.col, 0), uploaded with the scene.
// srt_accum_reset_features writes the two fields once.
// Adaptive featured accumulations (MODE 8, srt_accum_reset_adaptive_features) read the adaptive fields and the featured fields together.
// Spectral featured accumulations (MODE 9, srt_accum_reset_spectral_features) read `film` and the featured fields together.
// Adaptive spectral accumulations (MODE 10, srt_accum_reset_adaptive_spectral) read the adaptive fields and `film` together.
// Adaptive spectral featured accumulations (MODE 11, srt_accum_reset_adaptive_spectral_features) read the adaptive fields, `film` and
// mat_col; their rows lie behind the film in the film's own allocation, features == film + n_lanes * kFilmStride, and the kernel derives
// that address from `film` and n_lanes (LdsUniforms has no slot left for a fourth pointer).
constexpr uint32_t kFeatureStride = 8;      // 32 B per pixel: two 16-byte accesses
constexpr uint32_t kStreamSumPlane = 6;
constexpr uint32_t kMaxStreams = 16;      // SRT_MAX_STREAMS (srt_c_api.h)
constexpr uint32_t kFilmSamples = 95;
constexpr uint32_t kFilmStride = 96;      // 384 B: three 128-B lines per pixel, the last word unused
constexpr uint32_t kAdaptConverged = 0x80000000u;      // state word: the pixel has stopped (the low 31 bits: the samples it holds)

// The stopping test of render_kernel MODE 4 (srt_kernels.hip, adaptive_converged), fp32 without contraction, in this order
// (n = spp_total, S1 = the pixel's Y sum, S2 = its sum of squared per-sample Y):
//   mean = S1 / n;  v = S2 / n - mean * mean;  v = max(v, 0);  var_mean = v / (n - 1);  tol = rel_tol * mean + abs_tol
//   converged = n >= min_spp && var_mean <= tol * tol, and not converged when S1, S2, mean * mean or tol * tol is NaN or infinite

struct ScatterParams {
    const float *gathered;     // [rank][group (groups of them)][tiles_padded][plane of the group][lane]
    uint32_t groups;           // 1: only the quantised framebuffer was gathered (12 B / pixel); 3: the parity planes too
    float *fb[9];              // block-linear planes: r g b | lin r g b | X Y Z
    uint32_t width, height;
    uint32_t tx, ty, bx, by;
    uint32_t tiles_x, n_tiles, world, tiles_padded;
};

// XORWOW(seed + idx) for idx < n_lanes into six planes of n_lanes words.  (The streams of a streamed accumulation are one call: its planes
// hold K * n_lanes states, and stream k of lane idx is entry k * n_lanes + idx.)
hipError_t launch_init_rng(uint32_t *rng, uint32_t n_lanes, uint64_t seed, hipStream_t st);
// Test knobs of a context (srt_set_test_knobs; from the environment only under SRT_TEST_KNOBS=1, read once at srt_create): they pick
// the kernel variant / cache size a launch plan would not pick by itself, so that every instantiated variant can be held to the CPU oracle by the tests.
struct PlanKnobs { bool wide_refs = false; int lds_cache_max = -1; };
// The render launch's variant; the values are render_kernel's MODE template argument.  Plain: render; Counting: instrumented; Probe: cost
// probe; Accum: accumulating render (p.wave_debug -> AccumHeader); Adaptive / Spectral / Streams / Features: adaptive / spectral / streamed /
// featured accumulating render; AdaptiveFeatures: adaptive and featured at once; SpectralFeatures: spectral and featured at once;
// AdaptiveSpectral: adaptive and spectral at once; AdaptiveSpectralFeatures: all three.
enum RenderMode { Plain = 0, Counting = 1, Probe = 2, Accum = 3, Adaptive = 4, Spectral = 5, Streams = 6, Features = 7, AdaptiveFeatures = 8, SpectralFeatures = 9, AdaptiveSpectral = 10,
                  AdaptiveSpectralFeatures = 11 };
hipError_t launch_render(const RenderParams &p, const PlanKnobs &knobs, uint32_t n_cu, RenderMode mode, hipStream_t st);
hipError_t launch_accum_header(AccumHeader *dst, float *sums, uint32_t spp_total, hipStream_t st);      // writes *dst on the stream
// Pixel queue of the next adaptive pass (see adapt_flag_kernel): the rows of `src_rows` (src_info[0] of them; nullptr: the identity
// queue of n_identity local tiles) whose share of the tile still holds an active pixel, in their order, into dst_rows / dst_info[0..1];
// counts[0] += pixels that rendered in the pass that just ended, counts[1] += pixels still active.  flags: one word per source row.
struct AdaptQueueParams {
    const uint32_t *src_rows, *src_info;
    uint32_t n_identity;
    uint32_t *dst_rows, *dst_info, *flags;
    unsigned long long *counts;
    const uint32_t *state;
    uint32_t spp_total;
    uint32_t width, height, tx, ty, bx, by, tiles_x, n_tiles, rank, world, lane_limit;
};
hipError_t launch_adapt_queue(const AdaptQueueParams &p, uint32_t n_rows_bound, hipStream_t st);
// The film's grid samples [first, first + count) of the w x h pixels at the chunk's origin -> dst[((y * w) + x) * count + (j - first)].
hipError_t launch_film_unswizzle(const float *film, float *dst, uint32_t first, uint32_t count, uint32_t w, uint32_t h, uint32_t tx,
                                 uint32_t ty, uint32_t bx, hipStream_t st);
// The feature rows of the w x h pixels at the chunk's origin -> dst[((y * w) + x) * 8 + c].
hipError_t launch_features_unswizzle(const float *rows, float *dst, uint32_t w, uint32_t h, uint32_t tx, uint32_t ty, uint32_t bx, hipStream_t st);
// After a streamed pass (MODE 6): every pixel of this rank's share of the chunk adds its K stream sums in stream order into the
// accumulation's sum planes and writes its tile-buffer slots from them, as MODE 3's pixel switch does.
struct StreamCombineParams {
    const float *stream_sums;      // planes kStreamSumPlane .. of AccumHeader::stream_planes
    float *sums;                   // AccumHeader::sums
    float *tile_out;
    uint32_t streams, spp_total, n_lanes;
    uint32_t tile_group_stride, write_parity;
    uint32_t tiles_local;
    uint32_t width, height, tx, ty, bx, by, tiles_x, n_tiles, rank, world, lane_limit;
};
hipError_t launch_stream_combine(const StreamCombineParams &p, hipStream_t st);
// The denoiser (srt_denoise.hip; the filter is stated in srt_c_api.h at srt_denoise_features).  All images are row-major w x h.
// Prepass: pixel (x, y) reads lane idx = block_linear_idx(x, y, tx, ty, bx) -- its XYZ sum at sums[idx * sum_pixel_stride + c *
// sum_comp_stride] (an accumulation's planes: 1 and n_lanes; a caller's [h][w][3] array with tx = w, ty = h, bx = 1, which makes idx
// row-major: 3 and 1) and its feature row at rows[idx * 2] -- and writes colour[pix] = (c.xyz, 0), guides[2 pix] = (N.xyz, z),
// guides[2 pix + 1] = (A.xyz, coverage).
struct DenoisePrepassParams {
    const float *sums;
    size_t sum_pixel_stride, sum_comp_stride;
    const float4 *rows;
    uint32_t tx, ty, bx;
    uint32_t w, h, samples;
    float4 *guides, *colour;
    const uint32_t *counts;      // null: every pixel holds `samples`; else the pixel's own count, counts[idx] & ~kAdaptConverged (> 0)
};
// counts == null: the kernel every plain featured accumulation has always run; else its per-pixel-count sibling (inv = 1 / (float)n_p)
hipError_t launch_denoise_prepass(const DenoisePrepassParams &p, hipStream_t st);
// One level at step `step` (1 .. 128) from src to dst (never the same buffer); kn .. kc: the level's squared sigmas.
struct DenoiseLevelParams {
    const float4 *guides, *src;
    float4 *dst;
    uint32_t w, h, step;
    uint32_t tiles_x;      // filled in by the launcher
    float kn, ka, kz, kc;
};
hipError_t launch_denoise_level(const DenoiseLevelParams &p, hipStream_t st);
// colour (float4 per pixel) -> out_xyz / out_lin / out_q, n pixels of three floats each.
hipError_t launch_denoise_epilogue(const float *colour, float *out_xyz, float *out_lin, float *out_q, size_t n, hipStream_t st);
// The variance-guided path (srt_denoise_features_vg).  The estimator reads Y = colour[4 p + 1] and the guides, and writes the variance to
// colour[4 p + 3] and out_var[2 p]; kn .. kz: the squared guide sigmas.
struct DenoiseVarianceParams {
    const float4 *guides;
    float *colour, *out_var;
    uint32_t w, h;
    uint32_t tiles_x;      // filled in by the launcher
    float kn, ka, kz;
};
hipError_t launch_denoise_variance(const DenoiseVarianceParams &p, hipStream_t st);
// The measured estimator (srt_denoise_features_mv): pixel (x, y) reads lane idx as the prepass does -- its count counts[idx] &
// ~kAdaptConverged, its Y sum sum_y[idx * sum_pixel_stride] and its S2 sum_y2[idx] -- and writes the variance of its mean to
// colour[4 p + 3] and out_var[2 p].
struct DenoiseMeasuredParams {
    const float *sum_y, *sum_y2;
    const uint32_t *counts;
    size_t sum_pixel_stride;
    uint32_t tx, ty, bx;
    uint32_t w, h;
    float *colour, *out_var;
};
hipError_t launch_denoise_measured(const DenoiseMeasuredParams &p, hipStream_t st);
// One variance-guided level at step `step` (1 .. 128) from src to dst (never the same buffer), (colour.xyz, variance) per pixel;
// ks = sigma_variance * sigma_variance, floor = variance_floor.
struct DenoiseLevelVgParams {
    const float4 *guides, *src;
    float4 *dst;
    uint32_t w, h, step;
    uint32_t tiles_x;      // filled in by the launcher
    float kn, ka, kz, ks, floor;
};
hipError_t launch_denoise_level_vg(const DenoiseLevelVgParams &p, hipStream_t st);
// out_var[2 p + 1] = colour[p].w, n pixels.
hipError_t launch_denoise_var_out(const float *colour, float *out_var, size_t n, hipStream_t st);
// The developed payload (srt_denoise_developed; stated in srt_c_api.h).  The payload images are G = denoise_payload_groups(K) float4 per
// pixel, [group][pixel] over the row-major w x h pixels, channel k in lane k % 4 of group k / 4, the padding +0.
uint32_t denoise_payload_groups(uint32_t channels);      // KC / 4 with KC the smallest of 4, 8, 16 that holds the channels (0: too many)
// payload[g * pixels + pix] lane e = inv * developed[pix * channels + 4 g + e], inv = 1.0f / (float)samples
struct DenoisePayloadPrepassParams {
    const float *developed;      // [pixel][channels], row-major pixels
    float4 *payload;
    size_t pixels;
    uint32_t channels, groups, samples;
};
hipError_t launch_denoise_payload_prepass(const DenoisePayloadPrepassParams &p, hipStream_t st);
// Its per-pixel-count sibling: pixel (x, y) of the row-major w x h rectangle is normalised by its own count, inv = 1.0f / (float)n_p with
// n_p = counts[idx] & ~kAdaptConverged (> 0) and idx = block_linear_idx(x, y, tx, ty, bx), as DenoisePrepassParams::counts is read.
struct DenoisePayloadPrepassCountsParams {
    const float *developed;      // [pixel][channels], row-major pixels
    float4 *payload;
    const uint32_t *counts;
    uint32_t tx, ty, bx;
    uint32_t w, h;
    uint32_t channels, groups;
};
hipError_t launch_denoise_payload_prepass_counts(const DenoisePayloadPrepassCountsParams &p, hipStream_t st);
// One plain level (DenoiseLevelParams' fields mean what they mean there) that also filters the payload psrc -> pdst (never the same
// buffer) with the colour's weights.
struct DenoiseLevelDevParams {
    const float4 *guides, *src;
    float4 *dst;
    const float4 *psrc;
    float4 *pdst;
    uint32_t w, h, step;
    uint32_t tiles_x;      // filled in by the launcher
    uint32_t groups;
    float kn, ka, kz, kc;
};
hipError_t launch_denoise_level_dev(const DenoiseLevelDevParams &p, hipStream_t st);
// out_dev[pix * channels + k] = channel k of the payload, n pixels.
hipError_t launch_denoise_dev_out(const float4 *payload, float *out_dev, uint32_t channels, uint32_t groups, size_t n, hipStream_t st);
// The developed film (srt_develop.hip; the contraction is stated in srt_c_api.h at srt_develop_spectral).  Lane idx of the grid
// [0, n_lanes) holds the film row film[idx * kFilmStride ..]; the lane of pixel (x, y) = the inverse of block_linear_idx(x, y, tx, ty, bx)
// writes out[((y * w) + x) * channels + k] = (sum over j ascending of F_j * R[k][j]) * scale when x < w and y < h (a caller's
// film[n][96] with tx = n, ty = 1, bx = 1, w = n, h = 1 makes the map the identity).  response: the curves transposed and padded with
// +0, [kFilmSamples][develop_padded_channels(channels)], on the device.
constexpr uint32_t kMaxDevelopChannels = 16;      // SRT_MAX_DEVELOP_CHANNELS (srt_c_api.h)
struct DevelopParams {
    const float *film, *response;
    float *out;
    float scale;
    uint32_t channels;
    uint32_t n_lanes, tx, ty, bx;
    uint32_t w, h;
};
uint32_t develop_padded_channels(uint32_t channels);      // the kernel variant's channel count: the smallest of 1, 2, 3, 4, 8, 16 that holds them
hipError_t launch_develop(const DevelopParams &p, hipStream_t st);
// n pixels of three developed XYZ sums over `samples` samples -> out_lin / out_q (either may be null), three floats per pixel each.
hipError_t launch_develop_srgb(const float *xyz, float *out_lin, float *out_q, uint32_t samples, size_t n, hipStream_t st);
// Its per-pixel-count sibling (an adaptive spectral accumulation): pixel (x, y) of the row-major w x h rectangle is normalised by its own
// count n_p = counts[idx] & ~kAdaptConverged, idx = block_linear_idx(x, y, tx, ty, bx); a pixel without a sample (n_p == 0) by 1.
struct DevelopSrgbCountsParams {
    const float *xyz;
    float *out_lin, *out_q;
    const uint32_t *counts;
    uint32_t tx, ty, bx;
    uint32_t w, h;
};
hipError_t launch_develop_srgb_counts(const DevelopSrgbCountsParams &p, hipStream_t st);
// Exposure metering and tone mapping (srt_expose.hip; every operation is stated in srt_c_api.h at srt_meter_decide and srt_expose_accum).
// meter: lane idx of the grid [0, n_lanes) holds the luminance y[idx * y_stride] -- a Y sum that is multiplied by inv = 1.0f / (float)n
// when `normalise` is set, n = `samples`, or with `state` the lane's own count state[idx] & ~kAdaptConverged (0 counts as 1) -- of chunk
// pixel (i, j) = the inverse of block_linear_idx(i, j, tx, ty, bx).  The pixel is metered when it lies in the rectangle (x0, y0, w, h) and
// its 8 x 8 tile t = (j / 8) * tiles_x + i / 8 has t % world == rank.  hist[kMeterBins] and counts[3] (metered, dark, non-finite) are ADDED
// to: the caller zeroes them.  A caller's [h][w][3] array: y = its second component, y_stride = 3, tx = w, ty = h, bx = 1.
constexpr uint32_t kMeterBins = 4096;           // SRT_METER_BINS (srt_c_api.h)
constexpr uint32_t kMeterMaxBlocks = 1024;      // the grid's cap: the flush is at most this many workgroups' non-zero bins
struct MeterParams {
    const float *y;
    size_t y_stride;
    const uint32_t *state;
    uint32_t samples, normalise;
    uint32_t n_lanes, tx, ty, bx;
    uint32_t x0, y0, w, h;
    uint32_t tiles_x, rank, world;
    uint32_t *hist;
    unsigned long long *counts;
};
hipError_t launch_meter(const MeterParams &p, uint32_t n_cu, hipStream_t st);
// tone: pixel (x, y) of the row-major w x h rectangle takes its XYZ mean from the sum planes (sums[idx + c * comp_stride], idx =
// block_linear_idx(x, y, tx, ty, bx), times inv as above) or, with sums == null, from xyz[3 * pix + c]; gain, curve and kw = white * white
// as stated in srt_c_api.h; out_xyz / out_lin / out_q (any may be null) are row-major, three floats per pixel.  counts[3] (blown, crushed,
// non-finite) are ADDED to, for the pixels of this rank's tiles only.
struct ToneParams {
    const float *sums, *xyz;
    size_t comp_stride;
    const uint32_t *state;
    uint32_t samples;
    uint32_t tx, ty, bx;
    uint32_t w, h;
    uint32_t tiles_x, rank, world;
    uint32_t curve;
    float gain, kw;
    float *out_xyz, *out_lin, *out_q;
    unsigned long long *counts;
};
hipError_t launch_tone(const ToneParams &p, uint32_t n_cu, hipStream_t st);
// The presented picture (srt_present.hip; stated in srt_c_api.h at srt_present).  present: ToneParams' sources, curve and counters with one
// output -- out[y * w + x] = R | G << 8 | B << 16 | 255 << 24, the quantised sRGB of tone's out_q as bytes.  vec is the launcher's: groups of
// four pixels use 16-byte accesses where they are whole and aligned (allow_vector = false: never, the scalar path alone).
struct PresentParams {
    const float *sums, *xyz;
    size_t comp_stride;
    const uint32_t *state;
    uint32_t samples;
    uint32_t tx, ty, bx;
    uint32_t w, h;
    uint32_t tiles_x, rank, world;
    uint32_t curve;
    float gain, kw;
    uint32_t vec;
    uint32_t *out;
    unsigned long long *counts;
};
hipError_t launch_present(const PresentParams &p, uint32_t n_cu, bool allow_vector, hipStream_t st);
// mean[3 pix + c] = inv * developed[3 pix + c] over the row-major w x h pixels, inv = 1.0f / (float)samples -- with counts the pixel's own
// count counts[block_linear_idx(x, y, tx, ty, bx)] & ~kAdaptConverged (0 counts as 1), as DevelopSrgbCountsParams::counts is read.
struct PresentNormaliseParams {
    const float *developed;
    float *mean;
    const uint32_t *counts;
    uint32_t samples;
    uint32_t tx, ty, bx;
    uint32_t w, h;
};
hipError_t launch_present_normalise(const PresentNormaliseParams &p, hipStream_t st);
// The firefly filter (srt_despeckle.hip; stated in srt_c_api.h at srt_despeckle_accum) over the row-major w x h rectangle.  Exactly one
// source: sums (ToneParams' sum planes, comp_stride, state, samples and grid), xyz (a [h][w][3] XYZ mean) or src4 (the denoiser's float4
// colour image).  radius, rank_ppm, gain, floor: srt_despeckle's.  Outputs, any may be null: out_xyz / out_lin / out_q three floats per
// pixel, out_scale one, dst4 (never src4) the float4 image with the source's fourth word (+0 from another source).  counts[3] (clamped,
// non-finite, alone) are ADDED to.
struct DespeckleParams {
    const float *sums, *xyz;
    const float4 *src4;
    size_t comp_stride;
    const uint32_t *state;
    uint32_t samples;
    uint32_t tx, ty, bx;
    uint32_t w, h;
    uint32_t tiles_x;      // filled in by the launcher
    uint32_t radius, rank_ppm;
    float gain, floor;
    float *out_xyz, *out_lin, *out_q, *out_scale;
    float4 *dst4;
    unsigned long long *counts;
};
hipError_t launch_despeckle(const DespeckleParams &p, hipStream_t st);
// Temporal reprojection (srt_temporal.hip; stated in srt_c_api.h at srt_temporal_accum) over the row-major w x h rectangle of the chunk at
// image offset (ox, oy).  Exactly one colour source: xyz (a [h][w][3] XYZ mean) or src4 (the denoiser's float4 colour image); guides: two
// float4 per pixel, (N, z) and (A, coverage).  du .. center: the current camera; pcenter, pn, pe, pk, pbu, pbv: the previous camera's centre
// and its constants n', e', k', bu', bv'.  hist_c (one float4 per pixel: XYZ, len) and hist_g (two): the previous call's history, both
// null for none; new_c / new_g (never the old ones) receive the new one.  kn, ka, kz: the squared thresholds.  Outputs, any may be null:
// dst4 the float4 image with the source's fourth word (+0 from xyz), out_xyz / out_lin / out_q three floats per pixel, out_len one,
// out_motion two.  counts[5] (blended, fresh, offscreen, rejected, non-finite) are ADDED to.
struct TemporalParams {
    const float *xyz;
    const float4 *src4, *guides;
    const float4 *hist_c, *hist_g;
    float4 *new_c, *new_g;
    uint32_t w, h, ox, oy;
    uint32_t tiles_x;      // filled in by the launcher
    float du[3], dv[3], p00[3], center[3];
    float pcenter[3], pn[3], pe[3], pk, pbu[3], pbv[3];
    float kn, ka, kz, alpha_min, max_len;
    float4 *dst4;
    float *out_xyz, *out_lin, *out_q, *out_len, *out_motion;
    unsigned long long *counts;
    // the moving variant (srt_temporal_*_moving; null: the static stage): per pixel (Pprev, valid) of the surface-motion pass, which a hit
    // pixel projects in the place of the point it would reconstruct from the distance guide
    const float4 *prev_point;
    // the moments variant (srt_*_temporal_vg, srt_temporal_moments_kat; new_m null: the stage without moments): one float4 per pixel,
    // (m1, m2, mlen, 0) -- the first and second luminance moment carried through the colour's taps with the colour's weights, and their
    // own length.  hist_m: the previous call's (null: none, every finite pixel is seeded with (Y, Y * Y, 1, 0)); new_m (never hist_m)
    // receives the new one.
    const float4 *hist_m;
    float4 *new_m;
};
hipError_t launch_temporal(const TemporalParams &p, hipStream_t st);
// The choice of the variance behind the moments stage (srt_temporal.hip; stated in srt_c_api.h at srt_denoise_features_temporal_vg), over n
// pixels: moments[p] = Hm', len[len_stride * p] = len', spatial[spatial_stride * p] = vs_p, ml_min = (float)min_len.  v_p goes to
// out_var[out_stride * p] and, when colour_w is not null, to colour_w[4 * p] (the fourth word of the denoiser's colour image, which may be
// where `spatial` is read: the kernel is elementwise).  *count is ADDED to: the pixels that took the temporal variance.
struct TemporalVarianceParams {
    const float4 *moments;
    const float *len, *spatial;
    uint32_t len_stride, spatial_stride, out_stride;
    float ml_min;
    uint32_t n;
    float *colour_w, *out_var;
    unsigned long long *count;
};
hipError_t launch_temporal_variance(const TemporalVarianceParams &p, hipStream_t st);
// The surface-motion pass (srt_motion.hip; stated in srt_c_api.h at srt_surface_motion) over the row-major w x h rectangle at image offset
// (ox, oy): the closest hit of every pixel's centre ray on the scene images (nodes, fringe, tris: RenderParams'), then the hit point moved
// from the triangle's row of v_cur to its row of v_prev (9 floats per triangle each; v_prev null: nothing moved).  Outputs, any may be
// null: out_point (Pprev, valid) one float4 per pixel, out_tri one word, out_bary (t, beta, gamma) three floats.  counts[4] (hit, miss,
// moved, degenerate) are ADDED to.
struct MotionParams {
    const float4 *nodes, *fringe, *tris;
    int root_ref, stack_depth, n_inner, n_records;
    uint32_t fringe_stride, n_tris;
    const float *v_cur, *v_prev;
    uint32_t w, h, ox, oy;
    uint32_t tiles_x, stack_slots;      // filled in by the launcher
    float du[3], dv[3], p00[3], center[3];
    float4 *out_point;
    int32_t *out_tri;
    float *out_bary;
    unsigned long long *counts;
};
hipError_t launch_motion(const MotionParams &p, hipStream_t st);
// Batched ray queries (srt_query.hip; stated in srt_c_api.h at "Ray queries").  rays: two float4 per ray, (o, tmin) (d, tmax); the closest
// query writes hits[k] = (t, tri or -1, front_face, mat) as srt_trace_rays does, the any query occluded[k] = 0 / 1.  counter: one 32-bit word,
// zero when the kernel starts (the caller clears it on the same stream).  Scene fields: RenderParams'; n_cached: the plan's.
struct QueryParams {
    const float4 *nodes, *fringe, *tris;
    int root_ref, stack_depth, n_inner, n_cached, n_records;
    uint32_t fringe_stride;
    uint32_t score_fringe;      // step choice: FRINGE lanes x score_fringe against INNER lanes x 256 (RenderParams')
    const float4 *rays;
    uint32_t n;
    uint32_t *counter;
    float4 *hits;
    uint8_t *occluded;
};
// BVH refit (srt_refit.hip; stated in srt_c_api.h at srt_scene_refit and srt_refit_vertices).  verts: 9 floats per triangle.  The topology
// tables, made on the host at srt_upload_scene: tri_tab two words per triangle -- its raw aa_plane, then its slot 2 f + side, the FRINGE
// record f (an index into the FRINGE image) and the side whose block holds the triangle's copy, kRefitNoSlot when the root is a leaf; child
// two references per record (a record index, or ~triangle); sched the record indices grouped by height.  tris, shade, fringe (fringe_stride
// FLOATS between records), nodes, nodes_sw (null when the plan keeps none): the scene images.  leaf_box / rec_box: six floats per triangle
// / per record of scratch.  launch_refit_level handles the records sched[first .. first + count): one height.
constexpr uint32_t kRefitNoSlot = 0xffffffffu;
struct RefitParams {
    const float *verts;
    const uint32_t *tri_tab;
    const int32_t *child;
    const uint32_t *sched;
    float *tris, *shade, *fringe, *nodes, *nodes_sw;
    float *leaf_box, *rec_box;
    uint32_t n_tris, n_inner, fringe_stride;
};
// *count += the floats of verts[0 .. n_floats) that are not finite
hipError_t launch_refit_validate(const float *verts, size_t n_floats, uint32_t *count, hipStream_t st);
hipError_t launch_refit_triangles(const RefitParams &p, hipStream_t st);
hipError_t launch_refit_level(const RefitParams &p, uint32_t first, uint32_t count, hipStream_t st);
// The exchange unit of an accumulation (srt_gather.hip; srt_pack_accum / srt_unpack_accum in srt_c_api.h).  Internal, not ABI.
// The unit of rank r is tiles_padded tile records, the same size on every rank; record t is local tile t = global tile r + world * t, and
// slot lt of a tile is pixel tile_slot_pixel(tile, lt, tiles_x).  A record is tile_words 32-bit words, in this order:
//   plane words [word][slot], 64 each: the X, Y, Z sums; with n_planes == 5 (SRT_GATHER_COUNTS) then the state word and S2
//   features != null (SRT_GATHER_FEATURES): the feature rows [slot][kFeatureStride]
//   film != null (SRT_GATHER_FILM): the film rows [slot][kFilmStride], the unused word included
// so tile_words = 64 * (3 + 2 a + 8 f + 96 s).  Every word travels as its bit pattern (a transport is told ncclFloat).  Slots outside the
// chunk (queue_slot_in_chunk false) and tiles beyond the rank's tiles_local are +0 in a packed unit and ignored by the unpack.
// pack: `unit` receives the unit of (rank, world).  unpack: `unit` is `world` units, rank-major; the records of every rank but `rank` are
// written into the buffers, those of `rank` itself are not read.  vec is the launcher's (allow_vector = false: the 4-byte paths alone).
struct GatherParams {
    uint32_t *unit;
    uint32_t *sums;            // AccumLayout::sums: three planes of n_lanes words
    uint32_t *state, *sum2;    // AdaptPlanes (n_planes == 5), else null
    uint32_t *features, *film; // feature_rows(c) / d_film, null where the part does not travel
    uint32_t n_planes, tile_words, n_lanes;
    uint32_t width, height, tx, ty, bx, by;
    uint32_t tiles_x, n_tiles, rank, world, tiles_padded;
    uint32_t vec;
};
uint32_t gather_tile_words(uint32_t n_planes, bool features, bool film);
hipError_t launch_gather(const GatherParams &p, bool unpack, bool allow_vector, hipStream_t st);
hipError_t launch_order_tiles(const uint32_t *cost, uint32_t *sorted, uint32_t *rows, uint32_t n, uint32_t n_waves,
                              uint32_t split_load_pct, uint32_t *queue_info, uint32_t order_max_pct, hipStream_t st);
hipError_t launch_scatter(const ScatterParams &p, hipStream_t st);
hipError_t launch_unswizzle(const float *const src[3], float *const dst[3], uint32_t tx, uint32_t ty, uint32_t bx, uint32_t by,
                            uint32_t n_cols, uint32_t n_rows, uint32_t offx, uint32_t offy, uint32_t image_width,
                            uint32_t image_height, hipStream_t st);
hipError_t launch_trace(const RenderParams &p, const float *rays, size_t n, float *out, hipStream_t st);
hipError_t launch_op_sweep(int which, const float *a, const float *b, size_t n, float *out, hipStream_t st);
hipError_t launch_calib(int kind, uint32_t n_blocks, uint32_t threads, uint32_t iters, float *sink, unsigned long long *cycles, const float4 *table,
                        uint32_t n_records, hipStream_t st);
int calib_kinds();
bool render_narrow_refs(int n_records, const PlanKnobs &k);
bool render_paired_variant(bool tree_is_paired, bool narrow, bool all_cached);      // does launch_render pick render_kernel<.., PAIRED = true>?
size_t render_lds_bytes(int stack_depth, int waves_per_block, int n_cached, int n_records, const PlanKnobs &k);
void render_launch_shape(int stack_depth, int n_records, int n_inner, const PlanKnobs &k, int &waves_per_block, int &n_cached);
struct LaunchPlan { int waves_per_block, blocks_per_cu, waves_per_cu, waves_per_eu, n_cached; bool all_cached; };
void render_launch_plan(int stack_depth, int n_records, int n_inner, const PlanKnobs &k, LaunchPlan &lp);   // what launch_render will do for this scene
// The grid launch_render starts for a plan: workgroups of waves_per_block waves, `waves` = n_blocks * waves_per_block persistent waves in
// all -- every CU filled, never more waves than queue rows (queue_rows_bound: RenderParams'), rounded up to whole workgroups.
// waves_per_cu_override: RenderParams' experiment knob.  The launcher and whoever sizes a per-wave buffer both ask this function.
struct RenderGrid { int waves_per_block; uint32_t n_blocks, waves; };
RenderGrid render_launch_grid(const LaunchPlan &lp, uint32_t n_cu, uint32_t waves_per_cu_override, uint32_t queue_rows_bound);
// The launch of n ray queries (QueryParams) for a plan (render_launch_plan's; narrow / paired: render_narrow_refs / render_paired_variant):
// persistent workgroups of the plan's waves, every CU filled (n_cu x waves_per_cu), never more waves than rays / 64 rounded up or max_waves
// (> 0: the test grid, srt_set_query_test_grid).  lds: the inner-record cache and one stack per wave, without the render workgroup's tables.
struct QueryShape { bool narrow, all_cached, paired; int n_cached; uint32_t waves_per_block, n_blocks, waves; size_t lds; };
QueryShape query_shape(const LaunchPlan &lp, bool narrow, bool paired, int stack_depth, int n_records, const PlanKnobs &knobs, uint32_t n_cu,
                       uint32_t max_waves, size_t n_rays);
hipError_t launch_query(const QueryParams &p, const QueryShape &s, bool any, hipStream_t st);

}  // namespace srt
