/*
 * srt_c_api.h -- C-ABI of the MI355X-native spectral path-tracing hot path.
 *
 * This is the drop-in boundary for PieSil/CUDA-spectral-ray-tracer's render path.  The reference has
 * no FFI layer: the path sits behind the host classes `renderer` (rendering/rendering.cuh:39-155) and
 * `render_manager` (rendering/render_manager.cuh:37-224) and consumes device-heap objects built by
 * `scene_manager` (scene/scene.cuh:103-176).  Each entry point below names the reference interface it
 * replaces.  Plain pointers and sizes only; no C++/torch types.  All functions return 0 on success and
 * a negative srt_status on failure (never exit(): the reference's checkCudaErrors -> exit(99),
 * utils/cuda_utility.cu:8-18, is deliberately not reproduced); srt_last_error() gives the message.
 *
 * Host-side objects (srt_scene) need no GPU.  A device context (srt_ctx) needs a gfx950 device and
 * fails loudly without one -- there is no CPU fallback behind this API.
 */
#ifndef SRT_C_API_H
#define SRT_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_API __attribute__((visibility("default")))

#define SRT_N_CIE_SAMPLES 95      /* utils/cie_const.cuh:8 */
#define SRT_N_RAY_WAVELENGTHS 7   /* ray/ray.cuh:12 */
#define SRT_DEFAULT_SEED 1984u    /* rendering/rendering.cu:137, scene/scene.cu:14 */
#define SRT_DEFAULT_TX 28u        /* rendering/render_manager.cu:93-94 */
#define SRT_DEFAULT_TY 16u

typedef enum {
    SRT_OK = 0,
    SRT_ERR_INVALID = -1,      /* bad argument / call order (reference: message on cerr, call ignored) */
    SRT_ERR_NO_DEVICE = -2,    /* no gfx950 device / HIP runtime error at context creation */
    SRT_ERR_HIP = -3,          /* HIP runtime error (reference: checkCudaErrors -> exit(99)) */
    SRT_ERR_BVH = -4,          /* BVH build failed (reference: scene.cu:413-416 "Error building BVH") */
    SRT_ERR_UNSUPPORTED = -5,  /* e.g. non-grey sRGB colour without the (missing) rgb2spec table */
    SRT_ERR_NOMEM = -6
} srt_status;

/* material_type ids, materials/material.cuh:16-22 */
enum { SRT_MAT_LAMBERTIAN = 0, SRT_MAT_METALLIC = 1, SRT_MAT_DIELECTRIC = 2, SRT_MAT_EMISSIVE = 4, SRT_MAT_NO_MAT = 6 };
/* AAPlane, primitives/tri.cuh:8-13 */
enum { SRT_AAP_NONE = 0, SRT_AAP_XY = 1, SRT_AAP_YZ = 2, SRT_AAP_XZ = 3 };
/* scene ids: the reference's three (io/params.h:15-19) plus this build's synthetic benchmark scenes */
enum { SRT_SCENE_CORNELL = 0, SRT_SCENE_PRISM = 1, SRT_SCENE_TRIS = 2, SRT_SCENE_RANDOM_SPHERES = 100, SRT_SCENE_MESH100K = 101 };
/* BVH builders */
enum { SRT_BVH_REFERENCE = 0,  /* bit-faithful reference topology, bvh/bvh.cu:206-346 (x/y-only median split, Q14) */
       SRT_BVH_SAH = 1 };      /* this build's binned-SAH builder (same node semantics, better tree) */

/* Raw triangle as scene construction leaves it, before tri::init (primitives/tri.cu:47-84).
 * aa_plane is the value the member holds BEFORE init runs (sticky); NONE for a fresh tri. */
typedef struct { float v0[3], v1[3], v2[3]; uint32_t mat_index; uint32_t aa_plane; } srt_tri_in;

/* Same field order and size (428 B) as `material`, materials/material.cuh:140-148. */
typedef struct {
    float col[3];
    float reflection_fuzz;
    uint32_t material_type;
    float spectral_distribution[SRT_N_CIE_SAMPLES];
    float emission_power;
    float sellmeier_B[3];
    float sellmeier_C[3];
} srt_material;

/* Same field order and size (84 B) as `camera_data`, rendering/rendering.cuh:28-36. */
typedef struct {
    uint32_t width, height;
    float pixel_delta_u[3], pixel_delta_v[3], pixel00_loc[3];
    float defocus_angle;
    float camera_center[3], defocus_disk_u[3], defocus_disk_v[3];
} srt_camera_data;

/* Per-launch counters: a ray = one closest-hit query (bvh::hit call). */
typedef struct {
    uint64_t rays, paths;
    uint64_t node_visits;   /* traversal iterations = paired-child records fetched (V) */
    uint64_t tri_tests;     /* leaf (triangle) tests (T) */
    uint64_t box_tests;
    /* instrumented kernel only: [0] wave-level traversal steps, [1] sum over those steps of lanes that still own
     * work, [2] closest-hit queries answered without traversal because the direction is NaN (the reference walks
     * the whole tree for them and finds nothing), [3] fringe steps, [4] lanes served by them, [5] lanes served by
     * inner steps.  SIMD utilisation of traversal =
     * node_visits / (64 * util[0]).  node_visits / tri_tests / box_tests count the work actually done. */
    uint64_t util[9];   /* [6..8]: wave cycles spent in the shading phase / inner steps / fringe steps */
    uint64_t reserved[2];   /* instrumented: max node visits / max rays of any single pixel */
    /* instrumented kernel only: [0] shading passes (wave level), [1] lanes that shaded a finished query in them,
     * [2] lanes that generated a camera ray, [3] wave-level iterations of the unit-sphere rejection loop */
    uint64_t shade[4];
    /* instrumented kernel only, the tail of a launch: [0] waves, [1] sum of their life times (shader cycles from the start of
     * their state machine to their exit), [2] the longest life, [3] sum of the cycles waves lived on after the pixel queue had
     * run dry for them (drain time: lanes finishing their last pixels).  mean / max life = [1] / ([0] * [2]). */
    uint64_t waves[4];
    /* instrumented kernel only: closest-hit queries that found a triangle (each reads one 48-byte shading record); rays - hits =
     * misses (background look-up) + queries answered without traversal */
    uint64_t hits;
} srt_stats;

typedef struct srt_scene srt_scene;   /* host-side flattened scene (replaces scene_manager's device heap) */
typedef struct srt_ctx srt_ctx;       /* one GPU's renderer (replaces `renderer`, rendering.cuh:39-155) */

/* ---------------------------------------------------------------------------------------------------
 * Host side: scene inputs (no GPU).  Replaces scene_manager::init_world (scene/scene.cu:349-428),
 * create_world_kernel (:22-54) and create_bvh_kernel (:9-20).
 * ------------------------------------------------------------------------------------------------- */
SRT_API const char *srt_version(void);

/* camera::initialize, rendering/camera.cu:7-58 (camera_builder::getCamera, camera_builder.cuh:57-61). */
SRT_API int srt_camera_init(int image_width, int image_height, float vfov, const float lookfrom[3], const float lookat[3],
                            const float vup[3], float defocus_angle, float focus_dist, srt_camera_data *out);

/* Empty scene / one of the built-in scenes (scene/scene.cu:73-226; synthetic ids documented in DESIGN.md).
 * `seed` drives the synthetic scenes' layout PRNG; ignored for the reference scenes. */
SRT_API srt_scene *srt_scene_create(void);
SRT_API srt_scene *srt_scene_builtin(int scene_id, uint64_t seed);
SRT_API void srt_scene_destroy(srt_scene *s);
/* Default camera of a built-in scene (scene/scene.cu:259-320) for the given image size. */
SRT_API int srt_scene_default_camera(const srt_scene *s, int image_width, int image_height, srt_camera_data *out);

/* Scene construction.  srt_scene_set_* replace the whole list. */
SRT_API int srt_scene_set_triangles(srt_scene *s, const srt_tri_in *tris, size_t n);
SRT_API int srt_scene_set_materials(srt_scene *s, const srt_material *mats, size_t m);
SRT_API int srt_scene_set_background(srt_scene *s, const float spectrum[SRT_N_CIE_SAMPLES]);
SRT_API size_t srt_scene_tri_count(const srt_scene *s);
SRT_API size_t srt_scene_material_count(const srt_scene *s);
SRT_API int srt_scene_get_triangles(const srt_scene *s, srt_tri_in *out);       /* raw inputs, original order */
SRT_API int srt_scene_get_materials(const srt_scene *s, srt_material *out);
SRT_API int srt_scene_get_background(const srt_scene *s, float out[SRT_N_CIE_SAMPLES]);
/* tri::init results, 12 floats per triangle: normal(3) D clockwise aa_plane bbox(xmin xmax ymin ymax zmin zmax). */
SRT_API int srt_scene_get_tri_records(const srt_scene *s, float *out);

/* material::compute_spectral_distr (materials/material.cuh:71-84) for table-free colours (grey, white,
 * light, glass); SRT_ERR_UNSUPPORTED for non-grey sRGB (utils/srgb_to_spectrum.cu is absent upstream). */
SRT_API int srt_material_bake(srt_material *m);
/* Quirks of the reference's scene construction (Sellmeier C := B, materials/material.cuh:66-67; Q2: a grey colour's
 * sigmoid coefficient lands in the quadratic slot, color_to_spectrum.cuh:118-120): on (1, default) reproduces the reference as
 * written -- every parity statement refers to that --, 0 builds / bakes what was evidently meant (real Sellmeier C coefficients,
 * grey albedo g -> constant spectrum g).  Process-wide, affects srt_scene_builtin and srt_material_bake / srt_background_spectrum
 * calls made afterwards; returns the previous setting.  The render path itself has no switch. */
SRT_API int srt_set_reference_quirks(int on);
/* dev_srgb_to_spectrum / dev_srgb_to_illuminance_spectrum evaluated from explicit sigmoid coefficients
 * (color/color_to_spectrum.cuh:173-186,204-219): value = [scale * D65n(l)] * sigmoid(c[2] l^2 + c[1] l + c[0]). */
SRT_API int srt_bake_sigmoid_spectrum(const float coeffs[3], float scale, int times_d65, float out[SRT_N_CIE_SAMPLES]);
/* Own Jakob-Hanika style fit of the sigmoid coefficients of a NON-grey sRGB colour (replaces the lookup in the pbrt
 * rgb2spec table of color/color_to_spectrum.cuh:109-151, which the reference mount lacks).  coeffs are in the layout
 * srt_bake_sigmoid_spectrum expects.  Not pinned against the author's table. */
SRT_API int srt_fit_sigmoid_coeffs(const float rgb[3], float coeffs[3]);
/* host srgb_to_illuminance_spectrum for the background (rendering/rendering.cu:324), grey colours only. */
/* The constant tables the path computes with: cmf = 95 rows {x_bar, y_bar, z_bar, normalised D65} (cie_x / cie_y / cie_z /
 * normalized_cie_d65, utils/cie_const.cu:12-122, the host copies the reference uploads into dev_cie_* with
 * cudaMemcpyToSymbol) and the row-major d65_XYZ_to_sRGB matrix (utils/color_const.cu:17-19).  tests/test_ref_tables.py
 * compares them bit for bit with the reference's own arrays compiled from its sources (oracle/Makefile, target `ref`). */
SRT_API int srt_color_tables(float cmf[SRT_N_CIE_SAMPLES * 4], float xyz_to_srgb[9]);
SRT_API int srt_background_spectrum(const float rgb[3], float out[SRT_N_CIE_SAMPLES]);

/* transform::assign_rot_matrix (primitives/transform.cu:4-34): writes the rotation entries of a row-major 3x3 matrix for `axis`
 * 1 = X, 2 = Y, 3 = Z (transform::AXIS, transform.cuh:5-10) into m, which the caller initialised (the reference starts from the
 * identity, tri.cu:97-99); other axis values leave m untouched.  Points are rotated as vec3::matrix_mul does (math/vec3.cuh:80-91):
 * out[i] = m[3i] x + m[3i+1] y + m[3i+2] z.  The matrix the built-in scenes' boxes / pyramid / prism are turned with
 * (scene/scene.cu:115-128,166); tests/test_ref_host.py holds it against the reference's own function compiled from its source. */
SRT_API int srt_rotation_matrix(float theta, int axis, float m[9]);

/* BVH: `mode` SRT_BVH_REFERENCE reproduces create_bvh_kernel (fresh XORWOW(seed), bvh/bvh.cu:206-346);
 * SRT_BVH_SAH is this build's builder.  Either way the node semantics are the reference's: binary tree,
 * one triangle per leaf, leaf box = padded triangle box, internal box = union of children (Q22).  SRT_BVH_SAH (and srt_scene_optimise_bvh*)
 * leaves no node with two leaf children whose box is thinner on an axis than 2^-18 of its largest coordinate where another pair of leaves
 * is near enough to exchange a triangle with: the reference's slab test rejects such a box from afar. */
SRT_API int srt_scene_build_bvh(srt_scene *s, int mode, uint64_t seed);
/* The traversal is the reference's left-first walk, so the child order is part of the tree; SRT_BVH_SAH orders every node's
 * children by distance to the scene's default camera.  For another viewpoint: re-order the built tree for `eye` (the nearer
 * child becomes the left one; topology, boxes and depth unchanged), then srt_upload_scene again. */
SRT_API int srt_scene_order_children(srt_scene *s, const float eye[3]);
/* Topology optimisation of a built tree for throughput-bound launches (host only; no reference counterpart -- the tree is an input
 * of bvh::hit, bvh/bvh.cu:98-166): `passes` rounds of insertion-based optimisation (every subtree is taken out and put back where
 * it adds the least surface area; 3 rounds converge), then boxes, depth and the builder's child order again.  Fewer node records per
 * ray on average; NOT a cheaper worst pixel -- measured slower on launches bound by their longest pixel (few pixels per lane), so it
 * is a call of its own and not part of srt_scene_build_bvh.  Upload the scene afterwards. */
SRT_API int srt_scene_optimise_bvh(srt_scene *s, int passes);
/* srt_scene_optimise_bvh against the rays of a frame instead of box areas alone (host only, driven by the caller's array: no device).
 * segments[n_segments][7] = origin xyz, direction xyz (not normalised), t_end of a closest-hit query -- t_end the hit, or the query's
 * upper limit for a miss -- as srt_collect_ray_segments returns them.  The search, the canonical form, the paired-tree rules and the
 * FRINGE weight are srt_scene_optimise_bvh's; the price of a box is area + mu x (segments [0, t_end] that meet it, by the traversal's own
 * box test with closest_so_far = t_end: a box beyond the hit costs nothing), mu = 4 x area(root box) / segments used, so the area stays
 * as a prior of one fifth where every segment meets a box, and alone where none does.  Segments with a NaN or infinite origin, a
 * NaN or all-zero direction or t_end <= 0 are not used.  With no usable segment this IS srt_scene_optimise_bvh, bit for bit.  The
 * objective (srt_scene_bvh_ray_cost) never comes out higher than on the tree that walked in: a result that would is put back.  The same
 * segments in the same order give the same tree: single-threaded, integer counts.  Cost: about passes x nodes x segments box tests. */
SRT_API int srt_scene_optimise_bvh_for_rays(srt_scene *s, int passes, const float *segments, size_t n_segments);
/* The objective of srt_scene_optimise_bvh_for_rays for the built tree and a sample: the sum over the internal nodes of price x visit cost
 * (2.5 for a node with a leaf child, a FRINGE record, 1 otherwise). */
SRT_API int srt_scene_bvh_ray_cost(const srt_scene *s, const float *segments, size_t n_segments, double *cost);/* 1 when every internal node of the built tree has two leaf children or none ("paired": what SRT_BVH_SAH builds for an even triangle
 * count -- it cuts every span into two even halves -- and what srt_scene_optimise_bvh preserves).  The render launch of such a tree uses
 * the kernel variant whose FRINGE visit carries no box test (a node with one leaf child is the only kind that needs it). */
SRT_API int srt_scene_is_paired(const srt_scene *s);
SRT_API size_t srt_scene_node_count(const srt_scene *s);
SRT_API int srt_scene_bvh_depth(const srt_scene *s);
/* Pre-order dump (same convention as the oracle): left/right = pre-order ranks or -1, prim = original
 * triangle index for leaves else -1, boxes = 6 floats per node (xmin xmax ymin ymax zmin zmax). */
SRT_API int srt_scene_get_bvh(const srt_scene *s, int32_t *left, int32_t *right, int32_t *prim, float *boxes);
/* BVH refit (no reference counterpart: the reference's world is static): new vertices on the built topology, for geometry that deforms.
 * verts[n_tris][9] = v0 v1 v2 of every triangle, each xyz.  In this order: the vertices of every triangle are replaced -- its mat_index
 * and its stored aa_plane are inputs and stay -- and its tri::init products (normal, D, projection plane, winding, padded box) are
 * recomputed exactly as srt_scene_set_triangles computes them; then every node's box, leaves from their triangle's box and internal nodes
 * from their children's in one post-order sweep, and the depth, exactly as srt_scene_build_bvh finishes a tree.  Topology, child order, the
 * ordering viewpoint and the built state are not touched, so the scene equals in every bit one built from the moved triangles with this
 * topology.  SRT_ERR_INVALID with nothing changed: a null pointer, a BVH that is not built, n_tris != srt_scene_tri_count, a coordinate
 * that is not finite.  Host only; srt_upload_scene afterwards, or srt_refit_vertices with the same vertices on a context that holds the
 * scene.  Out of scope: changes of topology and any heuristic for when a tree degraded by motion should be rebuilt (build it again),
 * motion vectors for moving objects (the temporal stage knows camera motion only), and refit of materials. */
SRT_API int srt_scene_refit(srt_scene *s, const float *verts, size_t n_tris);
/* The level schedule a refit of this scene runs on the device (tests and tools; host only): *n_levels receives the number of record
 * heights -- height = 1 + the largest height of a child record, a leaf child counting 0; 0 when the root is a leaf -- and
 * level_counts[k], when not NULL (cap >= *n_levels, else SRT_ERR_INVALID), the records of height k + 1, one level launch each, bottom up.
 * Record indices do not order parents and children (every INNER record precedes every FRINGE record, and a FRINGE node may have an INNER
 * child), so the heights come from a walk over the references.  SRT_ERR_INVALID for a null argument or a BVH that is not built. */
SRT_API int srt_scene_refit_schedule(const srt_scene *s, uint32_t *level_counts, size_t cap, uint32_t *n_levels);

/* ---------------------------------------------------------------------------------------------------
 * Device side.  Replaces `renderer` (rendering/rendering.cuh:39-155) + the device half of
 * render_manager::step (rendering/render_manager.cu:3-66).
 * ------------------------------------------------------------------------------------------------- */
/* renderer ctor + hipSetDevice.  Fails with SRT_ERR_NO_DEVICE when no GPU is usable. */
SRT_API int srt_create(int device, srt_ctx **out);
SRT_API void srt_destroy(srt_ctx *ctx);
SRT_API const char *srt_last_error(const srt_ctx *ctx);   /* ctx may be NULL: last global error */

/* Uploads triangles, paired-child BVH records, material spectra and background to HBM
 * (replaces the device-heap world behind bvh** / material*, scene.cuh:163-170).  The BVH must be built. */
SRT_API int srt_upload_scene(srt_ctx *ctx, const srt_scene *s);
/* BVH refit on the device (srt_refit.hip; no reference counterpart): srt_scene_refit's operation applied to the scene images a context
 * holds, without a scene build or an upload.  The images are a function of the vertices and the topology alone; the topology -- record
 * order, references, root, stack depth, pairedness, launch plan, LDS residency and kernel variant -- stays, so only these are rewritten:
 * the triangle records, words 0 .. 2 (the normal) of every shading record, every triangle's inline copy in its FRINGE block (flag bits
 * included, the reference word kept), the children's boxes in every INNER record (and in its pre-swizzled copy where the plan keeps one)
 * and the box words of internal children in FRINGE records, at either FRINGE stride (padding words stay +0).
 *   Order.  (1) srt_refit_vertices_dev only: a kernel counts the coordinates that are not finite and the count is read back.  (2) One
 * thread per triangle restates tri::init operation by operation -- the cross product, the division by the length with the host's order of
 * sums, D, the perpendicularity tests with the three-term dots, the plane choice, the signed area, the padded box.  (3) Records are grouped
 * by height (1 + the largest height of a child record, a leaf child counting 0); one launch per height, bottom up, one thread per record,
 * writes the children's boxes and keeps the record's own box, the union taken as (left, right), for the launch above.
 *   Value equality.  The device takes minima and maxima as a compare and a select, (b < a) ? b : a and (b > a) ? b : a, where the host
 * calls fminf / fmaxf: they agree on all finite inputs except for the sign of a zero when +0 meets -0, and a degenerate triangle's NaN
 * normal may carry other bits than the host's.  The images therefore equal those srt_upload_scene makes of the host-refitted scene AS
 * VALUES: two words are equal when their bits are equal, or both are NaN, or both are zero.  Ray hits and frames are bit-identical.
 *   A successful refit invalidates what srt_upload_scene invalidates -- the accumulation (the next pass fails until a reset), the temporal
 * history (kept on a context that tracks motion: "Surface motion" below), the scheduler's remembered queues -- and leaves camera, device parameters, partition, knobs and RNG state alone.  Both entries
 * work on the NULL stream under the order of a context's calls, and both synchronise.  verts_dev is a device pointer (a torch tensor's
 * data_ptr(), say) whose contents must be complete, or ordered before the NULL stream, when the call is made.
 *   Refused with SRT_ERR_INVALID and nothing changed on the device: no scene uploaded (srt_set_test_knobs ends an upload too), a null
 * pointer, n_tris other than the uploaded scene's, a coordinate that is not finite -- nothing changed means the scene images and the
 * context's state; a refused srt_refit_vertices_dev may have allocated the context's scratch block, which the validation kernel counts
 * into.  A failed allocation: SRT_ERR_HIP.  The topology
 * tables are made on the host at srt_upload_scene and reach the device with the first refit; srt_upload_scene itself enqueues and
 * allocates nothing for them.  Out of scope as at srt_scene_refit: topology changes, object motion vectors (srt_temporal_track_motion
 * adds them, opt-in), materials.
 *   srt_refit_last_ms     kernel-only times in ms, from HIP events, of the context's last refit: the triangle kernel, all level launches
 *                         together, and their number.  Any pointer may be NULL.  SRT_ERR_INVALID before a refit has run.
 *   srt_read_scene_image  read-back of one scene image for tests and tools; synchronises, only reads.  *n_bytes receives the image's size
 *                         (0 for an image the plan does not keep: SRT_IMAGE_NODES_SW of an LDS-resident tree); out may be NULL to ask
 *                         for the size alone, else cap_bytes must hold it (SRT_ERR_INVALID). */
enum { SRT_IMAGE_NODES = 0, SRT_IMAGE_NODES_SW = 1, SRT_IMAGE_FRINGE = 2, SRT_IMAGE_TRIS = 3, SRT_IMAGE_SHADE = 4 };
SRT_API int srt_refit_vertices(srt_ctx *ctx, const float *verts_host, size_t n_tris);
SRT_API int srt_refit_vertices_dev(srt_ctx *ctx, const float *verts_dev, size_t n_tris);
SRT_API int srt_refit_last_ms(srt_ctx *ctx, float *tri_ms, float *levels_ms, uint32_t *n_levels);
SRT_API int srt_read_scene_image(srt_ctx *ctx, int which, void *out, size_t cap_bytes, size_t *n_bytes);
/* renderer::assign_cam_data, rendering/rendering.cu:237-242 */
SRT_API int srt_set_camera(srt_ctx *ctx, const srt_camera_data *cam);
/* What the render launch of the uploaded scene looks like (diagnostics / measurement bookkeeping): persistent waves per CU, inner
 * records resident in LDS, whether that is the whole inner tree (kernel variant ALL_CACHED) and whether record references fit 15
 * bits (variant NARROW).  Any pointer may be NULL. */
SRT_API int srt_launch_plan(const srt_ctx *ctx, int *waves_per_cu, int *n_cached, int *all_cached, int *narrow_refs);
/* 1 when the render launch of the uploaded scene uses the PAIRED kernel variant (FRINGE visit without a box test): the tree is paired
 * (srt_scene_is_paired), fits LDS and has 16-bit references. */
SRT_API int srt_launch_paired(const srt_ctx *ctx, int *paired);
/* TEST KNOBS of a context (no reference counterpart; tests/ and tools/ only).  They force a launch through kernel variants the plan
 * would not pick for the scene, so that every instantiated variant is held to the oracle: wide_refs != 0 -> 32-bit child references
 * for small trees too; lds_cache_max >= 0 caps the inner records kept in LDS (0: every inner record from L2; -1: no cap);
 * lane_limit > 0 renders only the first lane_limit pixels of every 8x8 tile (latency experiments; 0: all 64).  Defaults 0 / -1 / 0.
 * Upload the scene again after a change.  The environment never changes them at launch time: SRT_WIDE_REFS, SRT_LDS_CACHE_MAX and
 * SRT_DEBUG_LANE_LIMIT are read ONCE, at srt_create, and ONLY when SRT_TEST_KNOBS=1 is set as well -- a stray variable in a user's
 * shell does not alter the kernel that runs.  srt_get_test_knobs reports what the context uses (from_env: 1 if srt_create took a
 * value from the environment); srt_launch_plan reflects it.  Any out pointer may be NULL. */
SRT_API int srt_set_test_knobs(srt_ctx *ctx, int wide_refs, int lds_cache_max, uint32_t lane_limit);
SRT_API int srt_get_test_knobs(const srt_ctx *ctx, int *wide_refs, int *lds_cache_max, uint32_t *lane_limit, int *from_env);
/* Dynamic LDS bytes of one workgroup of that launch (tables + inner-record cache + traversal stacks): the counterpart of the
 * reference's shared_mem_size (rendering/rendering.cu:290-301), which its run log reports as "shared memory byte size" (:342). */
SRT_API int srt_launch_lds_bytes(const srt_ctx *ctx, size_t *bytes);
/* renderer::init_device_params (rendering/rendering.cu:279-357) + render_manager::init_renderer
 * (render_manager.cu:121-133): threads (tx,ty), grid (bx,by), chunk size, spp, bounce limit, RNG base seed.
 * Allocates the block-linear planar framebuffer and seeds the per-lane RNG states (init_random_states,
 * rendering.cu:120-138: XORWOW(seed + idx)).  spp / bounce_limit are narrowed to 16 bit like the reference (Q17). */
SRT_API int srt_init_device_params(srt_ctx *ctx, uint32_t tx, uint32_t ty, uint32_t bx, uint32_t by, uint32_t chunk_w,
                                   uint32_t chunk_h, uint32_t spp, uint32_t bounce_limit, uint64_t seed);
/* Multi-GPU split: this context renders tiles t with t % world == rank (8x8-pixel tiles of the chunk grid).
 * Seeds depend on the pixel only, so any split gives a bit-identical image.  Default rank 0, world 1. */
SRT_API int srt_set_partition(srt_ctx *ctx, uint32_t rank, uint32_t world);

/* renderer::render(w,h,offx,offy) -> call_render_kernel (rendering.cu:244-277).  Asynchronous on `stream`
 * (a hipStream_t passed as void*, NULL = default stream); the reference's device-wide sync is srt_synchronize.
 * Renders this rank's tiles into the context's compact tile buffer.
 *
 * Order of a context's calls.  A context's calls take effect in the order they were made, whichever streams they name.  A stream
 * handed to a call must stay valid until the next call on that context that synchronises.
 * The calls that take a stream are srt_render_chunk, srt_render_chunk_accum, srt_copy_tile_buffer, srt_scatter_tiles, the ray queries'
 * device entries (srt_intersect_rays_dev, srt_occluded_rays_dev), srt_pack_accum and srt_unpack_accum; every other
 * call works on the NULL stream.  The context remembers the stream of the work it enqueued last: a call that enqueues on another
 * stream -- the NULL stream included, and a hipStreamNonBlocking stream as well as a blocking one -- first makes its stream wait for
 * an event recorded behind that work, so a pass on one stream may be followed at once by a pass on another, a reset, a stage or a
 * read-back.  A caller that stays on one stream pays nothing for this.  The calls that synchronise -- they return with nothing of the
 * context in flight on any stream, and the remembered stream is not touched again after them, so it may be destroyed -- are
 * srt_synchronize; every read-back (srt_read_fb, srt_read_fb_aux, srt_read_fb_rowmajor, srt_read_accum_stats, srt_read_spectral,
 * srt_read_features, srt_accum_active on a bound accumulation, srt_get_stats, srt_get_tile_costs, srt_get_wave_debug,
 * srt_read_tile_schedule, srt_read_scene_image); srt_refit_vertices and srt_refit_vertices_dev; srt_intersect_rays and srt_occluded_rays; srt_direct_light and srt_direct_light_kat; every stage call that returns host data (srt_meter_*, srt_expose_*, srt_develop_*, srt_despeckle_*,
 * srt_temporal_*, srt_denoise_*, srt_present* -- not their *_last_ms timing queries, which wait for their own events alone);
 * srt_init_device_params and every srt_accum_reset*.  srt_comm_synchronize waits for the
 * communicator's own streams only and is none of them; srt_comm_destroy synchronises every context before it destroys those streams.
 * What is NOT ordered: work the caller itself enqueues on its streams (a copy out of srt_dev_fb, say) against later calls of the
 * context on other streams -- the context cannot see it. */
SRT_API int srt_render_chunk(srt_ctx *ctx, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy, void *stream);
SRT_API int srt_synchronize(srt_ctx *ctx);

/* Progressive rendering (no reference counterpart: the reference renders all spp samples of a chunk in one launch).  The context
 * keeps one accumulation: a per-pixel XYZ sum (12 B per lane of the grid, allocated on first use) and its running sample total.
 * srt_accum_reset zeroes both (no re-seeding); each srt_render_chunk_accum adds spp_add samples per pixel to the sums, continuing
 * the per-pixel RNG streams, and writes the tile buffer (and so, after a scatter, the framebuffer, the parity planes and the
 * row-major read-back) from the running mean.  Reset + passes of s1 .. sk samples leave framebuffer, parity planes, row-major
 * image and RNG state bit-identical to ONE srt_render_chunk with spp = s1 + .. + sk issued at the moment of the reset.
 * The accumulation belongs to the chunk (width, height, offx, offy) and the partition of its first pass.  It is invalidated by
 * srt_init_device_params, srt_set_partition, srt_upload_scene, srt_set_camera, srt_order_children_by_profile and a plain
 * srt_render_chunk: the next pass then fails with SRT_ERR_INVALID until srt_accum_reset.  Refused with nothing changed on the device:
 * spp_add == 0, a total above 65535 (the 16-bit spp, Q17), another chunk or offset (SRT_ERR_INVALID), an instrumented context
 * (srt_set_count_traversal on: SRT_ERR_UNSUPPORTED).  srt_get_stats after a pass reports that pass (paths = pixels x spp_add).
 * The spp of srt_init_device_params plays no part in a pass. */
SRT_API int srt_accum_reset(srt_ctx *ctx);
SRT_API int srt_render_chunk_accum(srt_ctx *ctx, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy, uint32_t spp_add, void *stream);
SRT_API int srt_accum_samples(const srt_ctx *ctx, uint32_t *spp_total);     /* samples per pixel the sums hold (0 right after a reset) */

/* Adaptive sampling (no reference counterpart).  An ADAPTIVE accumulation also keeps, per pixel, S2 -- the sum of the squared
 * per-sample luminance (the Y each sample's path adds to the pixel's XYZ sum; 0 for a path ended by the bounce limit) -- and a
 * state word: the samples the pixel holds and a "converged" flag.  Each srt_render_chunk_accum adds spp_add samples to the ACTIVE
 * pixels only; a converged pixel is left alone (no RNG draw, sums, S2 and tile-buffer slots unchanged), so every active pixel holds
 * the running total.  At the end of a pass every pixel that rendered in it tests, in fp32 without contraction and in this order
 * (n = (float)spp_total, S1 = its Y sum):
 *     mean = S1 / n;  v = S2 / n - mean * mean;  v = v > 0 ? v : 0;  var_mean = v / (n - 1);  tol = rel_tol * mean + abs_tol;
 *     converged = spp_total >= min_spp && var_mean <= tol * tol     (never when S1, S2, mean * mean or tol * tol is NaN or inf)
 * A pixel that stopped after n samples holds exactly what a plain launch of n spp gives it: quantised and parity planes, XYZ sums
 * and RNG state.  Decisions depend on the pixel's own sums alone, so the image does not depend on partition, world size or launch.
 * After each pass the next pass's pixel queue is compacted on the device (rows of tiles with an active pixel, in the probe's
 * order); the tile buffer is not cleared between adaptive passes (converged pixels keep their slots).
 *   srt_accum_reset_adaptive  srt_accum_reset + zeroed S2 and state planes (allocated on first use, 8 B per lane of the grid).
 *                             cfg: min_spp >= 2, rel_tol >= 0, abs_tol >= 0, rel_tol + abs_tol > 0, all finite, reserved == 0 --
 *                             else SRT_ERR_INVALID with nothing changed; an instrumented context: SRT_ERR_UNSUPPORTED.
 *                             srt_accum_reset makes the next accumulation a plain one again.  srt_set_gather_planes invalidates
 *                             an adaptive accumulation (converged pixels would keep stale planes); the other invalidations are
 *                             those of srt_accum_reset.  A pass with no active pixel is legal: it changes nothing but the total.
 *   srt_accum_active          pixels still active after the last pass (synchronises); 0 before the first pass, which binds the
 *                             chunk.  SRT_ERR_INVALID when the context holds no adaptive accumulation.
 *   srt_read_accum_stats      row-major maps of the accumulation's chunk, placed like srt_read_fb_rowmajor (only the chunk's
 *                             rectangle of the caller's arrays is written): samples per pixel, Y sums, S2.  Any pointer may be
 *                             NULL; samples and sum_y2 need an adaptive accumulation, sum_y any accumulation with a pass.  Pixels
 *                             owned by other ranks read as 0.
 * srt_get_stats after an adaptive pass: paths = pixels that rendered in it x spp_add, counted on the device. */
typedef struct { float rel_tol, abs_tol; uint32_t min_spp, reserved; } srt_adaptive;
SRT_API int srt_accum_reset_adaptive(srt_ctx *ctx, const srt_adaptive *cfg);
SRT_API int srt_accum_active(srt_ctx *ctx, uint64_t *active);
SRT_API int srt_read_accum_stats(srt_ctx *ctx, uint32_t *samples, float *sum_y, float *sum_y2, uint32_t image_width, uint32_t image_height);

/* Spectral film (no reference counterpart).  A SPECTRAL accumulation is a plain progressive accumulation (srt_accum_reset semantics:
 * passes of s1 .. sk samples equal one launch of their sum in every output above) that also keeps a FILM: 95 raw fp32 sums per pixel,
 * one per sample of the CIE grid the material spectra and colour tables use, F_j at lambda_j = 360 + 5 j nm, j = 0 .. 94.
 * The deposit rule (render_kernel MODE 5):
 *   - at every path end that is converted to XYZ -- a miss, or a hit that does not scatter -- and only there: a path ended by the bounce
 *     limit deposits nothing, as it adds nothing to XYZ;
 *   - for each of the path's 7 wavelengths k: (off_k, w_k) = the interpolation coordinates of wl[k] on the grid (the ones its XYZ
 *     conversion uses: off = (int)((wl - 360) * (94 / 470)) clamped to [0, 93], w = (wl - 360) * (94 / 470) - off), p_k = the path's
 *     power at wl[k] when k < valid (the wavelengths still valid), +0 otherwise;
 *   - F[off_k] += (1 - w_k) * p_k;  F[off_k + 1] += w_k * p_k   (fp32, no contraction, each product rounded once).
 * Paths are added in sample order; a pixel's film is written only by the lane that renders it (no atomics), so the film is the same bits
 * in every run, launch shape and partition.  The 7 wavelengths of a path lie 470/7 nm apart and never share a grid sample.  With
 * d = 470/7 and x, y, z the colour-matching rows of srt_color_tables, d * sum_j F_j * (x_j, y_j, z_j) equals the XYZ sums up to
 * reassociation.  The device stores raw sums; the mean spectral radiance at lambda_j of a pixel holding n samples is estimated by
 *   L_j = F_j * 470 / (35 n)  for 0 < j < 94, and twice that at j = 0 and j = 94 (their hats are half as wide).
 *   srt_accum_reset_spectral  srt_accum_reset + a zeroed film (allocated on first use and when n_lanes changes, kFilmStride = 96 floats
 *                             = 384 B per lane of the grid).  Later srt_render_chunk_accum passes run MODE 5.  An instrumented context:
 *                             SRT_ERR_UNSUPPORTED; device parameters not set: SRT_ERR_INVALID; a failed allocation: SRT_ERR_HIP -- in
 *                             every refusal the previous accumulation is unchanged.  Always a PLAIN (non-adaptive) accumulation.
 *                             (This sentence used to go on "adaptive + spectral is not supported": it is now, as an accumulation kind of
 *                             its own -- srt_accum_reset_adaptive_spectral, below.  Spectral + features is another:
 *                             srt_accum_reset_spectral_features, below.)  srt_accum_reset and srt_accum_reset_adaptive make the next
 *                             accumulation non-spectral again.  Invalidation, the 65535-sample limit and the chunk binding are those of
 *                             srt_accum_reset; srt_get_stats after a spectral pass reports that pass.
 *   srt_read_spectral         the raw sums of grid samples [first, first + count) of the accumulation's chunk, row-major:
 *                             out[((y * image_width) + x) * count + (j - first)]; only the chunk's rectangle is written (the placement
 *                             of srt_read_fb_rowmajor), pixels owned by other ranks read +0.  Synchronises.  SRT_ERR_INVALID without a
 *                             spectral accumulation with at least one pass, for count == 0, first + count > 95 or a null out. */
SRT_API int srt_accum_reset_spectral(srt_ctx *ctx);
SRT_API int srt_read_spectral(srt_ctx *ctx, uint32_t first, uint32_t count, float *out, uint32_t image_width, uint32_t image_height);

/* The film developed on the device (no reference counterpart; kernels in csrc/srt_develop.hip).  Everything a film is used for is a
 * contraction over its 95 grid samples -- another sensor's response curves, a colour filter in front of the lens, a band image, the
 * colour-matching rows themselves -- and only the K resulting planes have to leave the device.  The operation, for a pixel's film row
 * F_0 .. F_94, K response curves R[k][j] (row-major [K][95], fp32) and an fp32 scale -- everything fp32, not contracted, in this order,
 * so that a float32 restatement (tests/develop_reference.py) predicts the device's bits:
 *     a_k = +0.0f
 *     for j = 0, 1, .., 94 in this order:   t = F_j * R[k][j];   a_k = a_k + t      (the product rounded, then the sum rounded)
 *     out_k = a_k * scale
 *   1 <= K <= SRT_MAX_DEVELOP_CHANNELS.  Every R[k][j] and scale must be finite (checked on the host); the film's own NaN and infinite
 *   sums propagate as the arithmetic says (0 * inf = NaN: a pixel with a non-finite sum is non-finite in every channel, and no other pixel is).
 *   The 96th word of a film row (the unused one of its 384 bytes) never enters.  A filter of transmittances T_j is folded into the curves
 *   by the caller, R'[k][j] = R[k][j] * T_j, one fp32 product per entry.
 *   srt_develop_spectral      develops the context's spectral accumulation: out[((y * image_width) + x) * channels + k]; only the chunk's
 *                             rectangle is written, with the placement of srt_read_spectral; pixels owned by other ranks hold a zero
 *                             film row and come out zero in value.  Synchronises.  It only READS the accumulation: later passes, the
 *                             film, the frame and the RNG state are what they would be without the call.  Any partition is accepted (no
 *                             pixel reads a neighbour).  Working blocks (the transposed curves and the developed planes) belong to the
 *                             context, are reused and grow with the chunk.  Refused with nothing changed on the device: no spectral
 *                             accumulation with at least one pass, a null pointer, channels == 0 or > SRT_MAX_DEVELOP_CHANNELS, an empty
 *                             image, a response or scale that is NaN or infinite (SRT_ERR_INVALID); a failed allocation (SRT_ERR_HIP).
 *   srt_develop_spectral_srgb three channels developed by the same kernel and taken as XYZ SUMS of the accumulation's n samples.
 *                             response3 == NULL selects the colour-matching rows x, y, z of srt_color_tables (with scale = the fp32
 *                             470/7 the sums are the accumulation's XYZ sums up to reassociation).  out_xyz receives the developed
 *                             sums S; out_lin and out_q the conversion the render kernel applies to an accumulation's XYZ sums and its
 *                             sample total:  inv = 1.0f / (float)n;  c = (inv * S.x, inv * S.y, inv * S.z);  then XYZ -> linear sRGB rows,
 *                             correct_channel, (float)(int)(v * 255.99f) (xyz_mean_to_srgb, as the denoiser's epilogue).  Layout
 *                             out[((y * image_width) + x) * 3 + c], placement as above.  Any of the three outputs may be NULL, not all.
 *                             Refusals as above.
 *   srt_develop_kat           KAT entry point: the same kernel on a caller-supplied host array film[n_pixels][95]; the library uploads it
 *                             into 96-float rows (the 96th word set to a NaN: a kernel that let it enter would show) and the pixel
 *                             mapping is the identity; out[n_pixels][channels].  Needs neither a scene nor an accumulation and touches
 *                             neither.  SRT_ERR_INVALID for a null argument, n_pixels == 0 or >= 2^31, channels, response or scale as above.
 *   srt_develop_last_ms       kernel-only times of the context's last develop (any entry point) in ms, from HIP events: the contraction,
 *                             and the sRGB epilogue (0 when the call had none).  Either pointer may be NULL.  Measurement support
 *                             (tools/develop_cost.py).  SRT_ERR_INVALID before the first develop. */
#define SRT_MAX_DEVELOP_CHANNELS 16
SRT_API int srt_develop_spectral(srt_ctx *ctx, const float *response, uint32_t channels, float scale, float *out,
                                 uint32_t image_width, uint32_t image_height);
SRT_API int srt_develop_spectral_srgb(srt_ctx *ctx, const float *response3, float scale, float *out_xyz, float *out_lin, float *out_q,
                                      uint32_t image_width, uint32_t image_height);
SRT_API int srt_develop_kat(srt_ctx *ctx, const float *film, uint32_t n_pixels, const float *response, uint32_t channels, float scale,
                            float *out);
SRT_API int srt_develop_last_ms(srt_ctx *ctx, float *contract_ms, float *epilogue_ms);

/* Exposure metering and tone mapping on the device (no reference counterpart: the reference clamps whatever it is given; kernels in
 * csrc/srt_expose.hip).  A luminance histogram is taken where the sums live, an exposure gain is decided from it on the host, and a tone
 * curve runs in front of the conversion every other picture ends in (xyz_mean_to_srgb: linear sRGB clamped to [0, 1], gamma-encoded,
 * quantised).  Operation by operation -- everything fp32, not contracted, left to right, selects and never fmax; the restatement is
 * tests/expose_reference.py, which the device equals in every integer and every bit:
 *   Luminance of a pixel.  From an accumulation: Y_p = inv * S_y with S_y the pixel's Y sum and inv = 1.0f / (float)n, n the sample
 *     total -- on an adaptive kind the pixel's own count n_p = state & 0x7fffffff, and inv = 1 where n_p == 0 -- as the epilogues
 *     normalise.  From a caller's XYZ-mean array [h][w][3]: Y_p is the second component, untouched.
 *   Classification of a pixel inside the metered rectangle, the tests in this order:
 *     1. non-finite when (Y - Y) == 0 is false;
 *     2. otherwise dark when Y >= FLT_MIN (1.17549435e-38f) is false: zeros of both signs, negatives, denormals;
 *     3. otherwise metered, into bin b = float_as_uint(Y) >> 19: the 8 exponent bits and the top 4 mantissa bits, 16 bins per octave,
 *        b in [16, 4080); a histogram has SRT_METER_BINS = 4096 uint32 counts.
 *   Ownership.  Pixel (i, j) of the chunk lies in the 8 x 8 tile t = (j / 8) * tiles_x + i / 8 (tiles_x = ceil(tx * bx / 8), the tiles of
 *     srt_set_partition).  A pixel of a tile this rank does not own (t % world != rank) is skipped: counted in no bin and in no counter.
 *     So the histograms and counters of the ranks of a partition add up to those of partition (0, 1), exactly -- they are integers.
 *   Decision (srt_meter_decide: host only, no context, no GPU), from hist[4096] and cfg:
 *     n = sum of hist[16 .. 4079] in uint64.  n == 0: bin_ref = 0, y_ref = 0, g = 1.0f.  Otherwise
 *       target = max(1, (n * percentile_ppm + 999999) / 1000000)  (uint64);  bin_ref = the smallest B with sum of hist[16 .. B] >= target;
 *       y_ref = uint_as_float((bin_ref << 19) | (1 << 18)), the bin's midpoint;  g = key / y_ref.
 *     In every case  g = g < gain_min ? gain_min : g;  g = g > gain_max ? gain_max : g.  result->metered = n; dark and nonfinite are
 *     left as the caller passed them in (the histogram does not hold them).
 *     What follows: metering is scale invariant for powers of two -- a picture scaled by 2^k (no overflow, no underflow, no clamp of the
 *     gain) shifts its histogram by 16 k bins and gets exactly 2^-k times the gain, so its exposed picture is the same, bit for bit.
 *   cfg (srt_meter), validated by every entry point that takes one, else SRT_ERR_INVALID: 1 <= percentile_ppm <= 1000000; key finite and
 *     > 0; 0 < gain_min <= gain_max, both finite; the reserved words 0; the rectangle (x0, y0, w, h) in chunk pixels either all zero --
 *     the whole chunk -- or non-empty (w > 0 and h > 0) and, where there is a chunk, inside it.
 *   Tone (srt_tone), per pixel with XYZ mean c, g = gain and kw = white * white formed once on the host:
 *     c' = (g * c.x, g * c.y, g * c.z);  y = c'.y
 *     curve 0 (linear):  o = c'
 *     curve 1 (extended Reinhard on luminance):  t = y / kw;  num = 1.0f + t;  den = 1.0f + y;  s = num / den;  s = (y > 0) ? s : 1.0f;
 *       o = (s * c'.x, s * c'.y, s * c'.z)      -- white = +inf: t = 0 and the curve is plain Reinhard
 *     o goes through xyz_mean_to_srgb unchanged: out_xyz = o, out_lin the unquantised and out_q the quantised sRGB.  A non-finite pixel
 *     propagates as the arithmetic says and touches no other pixel.  The kernel counts, over the pixels of this rank's tiles, with
 *     integer atomics after a wave-level reduction: blown -- any quantised channel equals 255; crushed -- all three equal 0; nonfinite --
 *     (v - v) == 0 is false for a component v of o.  With curve 0 and gain 1, out_lin and out_q are the frame's own planes.
 *     Validated, else SRT_ERR_INVALID: curve 0 or 1; gain finite and > 0; white > 0 (+inf allowed, NaN not); the reserved words 0.
 *   srt_meter_decide      as above.  SRT_ERR_INVALID for a null pointer or a bad cfg (the rectangle: all zero or non-empty).
 *   srt_meter_accum       meters the context's bound accumulation of ANY kind -- streamed included: every kind keeps its XYZ sums in the
 *                         same planes -- under any partition, decides, and fills *result (counters included); hist, unless NULL,
 *                         receives the 4096 counts.  Synchronises.  Only reads the accumulation.  SRT_ERR_INVALID, nothing changed, for
 *                         no accumulation with at least one pass, a bad cfg (a rectangle outside the chunk clipped to the reference
 *                         grid included) or a null ctx / cfg / result; SRT_ERR_HIP for a failed allocation.
 *   srt_meter_kat         the same kernel on a caller's row-major host array xyz_mean[h][w][3] (the chunk is w x h, one rank).  Needs
 *                         neither a scene nor an accumulation and touches neither: also the door for denoised and developed XYZ means.
 *                         SRT_ERR_INVALID also for a null array, an empty image or w x h >= 2^31.
 *   srt_expose_accum      the tone kernel on the bound accumulation.  Placement and clipping are srt_develop_spectral_srgb's: the kernel
 *                         runs on the chunk's rectangle and the images receive the part of it inside image_width x image_height at the
 *                         chunk's offset; nothing else of them is written.  Any of out_xyz / out_lin / out_q may be NULL, not all;
 *                         result may be NULL.  Synchronises; only reads the accumulation.  Pixels of another rank's tiles hold +0 sums
 *                         and come out as +0.  SRT_ERR_INVALID for no accumulation with a pass, a bad srt_tone, all outputs NULL, an
 *                         empty image, a null ctx / tone; SRT_ERR_HIP for a failed allocation.
 *   srt_expose_kat        the same kernel on xyz_mean[h][w][3]; outputs [h][w][3]; refusals as srt_meter_kat's and srt_expose_accum's.
 *   srt_expose_last_ms    kernel-only times in ms, from HIP events, of the context's last meter kernel and last tone kernel (0 for one
 *                         that has not run); SRT_ERR_INVALID before either has run.  Either pointer may be NULL.
 * Working blocks (the global histogram and counters, 16 KiB; nine floats per pixel of the rectangle for the images; three per pixel for a
 * KAT input) belong to the context and are reused.  No call here invalidates or alters an accumulation, the frame or the RNG state. */
#define SRT_METER_BINS 4096
typedef struct srt_meter { uint32_t x0, y0, w, h; uint32_t percentile_ppm; float key, gain_min, gain_max; uint32_t reserved[4]; } srt_meter;
typedef struct srt_meter_result { uint64_t metered, dark, nonfinite; uint32_t bin_ref; float y_ref, gain; uint32_t reserved; } srt_meter_result;
typedef struct srt_tone { uint32_t curve; float gain, white; uint32_t reserved[5]; } srt_tone;
typedef struct srt_tone_result { uint64_t blown, crushed, nonfinite; } srt_tone_result;
SRT_API int srt_meter_decide(const uint32_t *hist, const srt_meter *cfg, srt_meter_result *result);
SRT_API int srt_meter_accum(srt_ctx *ctx, const srt_meter *cfg, uint32_t *hist, srt_meter_result *result);
SRT_API int srt_meter_kat(srt_ctx *ctx, const srt_meter *cfg, const float *xyz_mean, uint32_t w, uint32_t h, uint32_t *hist, srt_meter_result *result);
SRT_API int srt_expose_accum(srt_ctx *ctx, const srt_tone *tone, float *out_xyz, float *out_lin, float *out_q, srt_tone_result *result,
                             uint32_t image_width, uint32_t image_height);
SRT_API int srt_expose_kat(srt_ctx *ctx, const srt_tone *tone, const float *xyz_mean, uint32_t w, uint32_t h,
                           float *out_xyz, float *out_lin, float *out_q, srt_tone_result *result);
SRT_API int srt_expose_last_ms(srt_ctx *ctx, float *meter_ms, float *tone_ms);

/* First-hit feature buffers (no reference counterpart): the geometric side channels a denoiser or compositor takes as input.  A FEATURED
 * accumulation is a plain progressive accumulation (the semantics of srt_accum_reset: passes of s1 .. sk samples equal one launch of
 * their sum in every output above, RNG state included) that also keeps, per pixel, 8 raw fp32 sums F[0..7]:
 *   F[0..2] normal, F[3..5] albedo, F[6] distance, F[7] hits.
 * The deposit rule (render_kernel MODE 7):
 *   - at the shading of the FIRST closest-hit query of every sample (the camera ray's, bounce 0), and only when that query found a
 *     triangle: nothing on a miss, nothing for a query answered without traversal because its direction holds a NaN, nothing on later
 *     bounces, and nothing at all with bounce_limit == 0;
 *   - normal: the face-forwarded normal the shading forms (front_face ? n_geo : -n_geo);
 *   - albedo: the hit material's srt_material.col, from a per-material table uploaded with the scene and read with a range-checked
 *     load: a material index beyond the table adds +0;
 *   - distance: t * sqrtf(dx*dx + dy*dy + dz*dz), t the accepted hit parameter and d the camera ray's unnormalised direction, the sum
 *     left to right, fp32, not contracted;
 *   - hits: 1.0f;
 *   - F[c] = F[c] + f[c] in fp32, in sample order.
 * The deposit draws nothing from the RNG and touches neither the image nor the path.  A pixel's row is written only by the lane that
 * renders it (no atomics), so the eight sums are the same bits for every split into passes, launch shape, partition and world size.
 * The device stores raw sums; with n the samples a pixel holds, normal / n and albedo / n are the means over all samples (a miss counts
 * as zero), distance / hits the mean hit distance and hits / n the pixel's coverage.
 *   srt_accum_reset_features  srt_accum_reset + zeroed feature rows (allocated on first use and when n_lanes grows, 32 B per lane of the
 *                             grid).  Later srt_render_chunk_accum passes run MODE 7.  Refused with the previous accumulation unchanged:
 *                             device parameters not set (SRT_ERR_INVALID); an instrumented context (SRT_ERR_UNSUPPORTED); a failed
 *                             allocation (SRT_ERR_HIP).  Always a PLAIN accumulation: features combined with the spectral film or
 *                             streams are NOT supported.  (Features with the spectral film have since become an accumulation kind of
 *                             their own: srt_accum_reset_spectral_features, below.)  (This paragraph used to end "adaptive + features is the intended next step":
 *                             that step is srt_accum_reset_adaptive_features, below, and both denoisers take either kind.)
 *                             srt_accum_reset, srt_accum_reset_adaptive, srt_accum_reset_spectral and
 *                             srt_accum_reset_streams make the next accumulation non-featured again.  Invalidation, the 65535-sample
 *                             limit and the chunk binding are those of srt_accum_reset.
 *   srt_read_features         the raw sums of the accumulation's chunk, row-major: out[((y * image_width) + x) * 8 + c]; only the
 *                             chunk's rectangle is written (the placement of srt_read_fb_rowmajor), pixels owned by other ranks read
 *                             +0.  Synchronises.  SRT_ERR_INVALID without a featured accumulation with at least one pass, or for a
 *                             null out. */
SRT_API int srt_accum_reset_features(srt_ctx *ctx);
SRT_API int srt_read_features(srt_ctx *ctx, float *out, uint32_t image_width, uint32_t image_height);

/* Adaptive sampling and first-hit features in ONE accumulation (no reference counterpart): the frames whose noise differs from pixel to
 * pixel are the ones a denoiser is for.  An ADAPTIVE FEATURED accumulation is an adaptive accumulation (srt_accum_reset_adaptive: the
 * same cfg, stopping rule, state words, S2 and queue compaction) that also keeps the feature rows of srt_accum_reset_features (the same
 * deposit rule).  Later srt_render_chunk_accum passes run render_kernel MODE 8: MODE 4 in every respect -- converged pixels are skipped
 * at the fetch, the decision and the state word are written at the pixel switch, the pixel queue is compacted on the device between
 * passes -- plus MODE 7's deposit at the first hit, which draws nothing from the RNG.  What holds, and is tested:
 *   - under the same cfg and the same pass schedule the image, all nine planes, the XYZ sums, S2, the state words, the active counts and
 *     the RNG state are bit-identical to an adaptive accumulation's (MODE 4);
 *   - a pixel that stopped after n samples holds the feature row of a PLAIN featured n-spp frame at that pixel, bit for bit; an active
 *     pixel holds the row of the running total;
 *   - a converged pixel's row is not touched by later passes;
 *   - the result is independent of partition, world size, launch shape and split into passes, as for either parent.
 *   srt_accum_reset_adaptive_features  validation, refusals and invalidation are srt_accum_reset_adaptive's (cfg as there; an instrumented
 *                             context; device parameters not set), the rows are allocated by srt_accum_reset_features' rule (on first use
 *                             and when n_lanes grows; a failed allocation is SRT_ERR_HIP); every refusal leaves the previous
 *                             accumulation unchanged.  The accumulation is adaptive AND featured: srt_accum_active,
 *                             srt_read_accum_stats and srt_read_features all work on it, srt_set_gather_planes invalidates it, and
 *                             srt_denoise_features / _vg / _mv take it.  srt_accum_reset, srt_accum_reset_adaptive,
 *                             srt_accum_reset_features, srt_accum_reset_spectral and srt_accum_reset_streams make the next accumulation
 *                             something else again.  (srt_read_features still refuses a plain adaptive accumulation, srt_accum_active a
 *                             plain featured one.) */
SRT_API int srt_accum_reset_adaptive_features(srt_ctx *ctx, const srt_adaptive *cfg);

/* The spectral film and first-hit features in ONE accumulation (no reference counterpart): the previews that most need a denoiser -- a
 * few samples through a narrow band or another sensor -- are developed from a film, and the denoiser needs the feature rows.  A SPECTRAL
 * FEATURED accumulation is a spectral accumulation (srt_accum_reset_spectral: the same film, the same deposit rule) that also keeps the
 * feature rows of srt_accum_reset_features (the same deposit rule).  Later srt_render_chunk_accum passes run render_kernel MODE 9: MODE 5
 * and MODE 7 at once.  MODE 7's deposit draws nothing from the RNG and MODE 5's deposit touches nothing MODE 7 reads, so no new code runs
 * in the kernel body.  What holds, and is tested, under the same pass schedule and seed:
 *   - the image, all nine planes, the XYZ sums, the RNG state and the 95 film sums are bit-identical to a spectral accumulation's (MODE 5);
 *   - the eight feature sums are bit-identical to a featured accumulation's (MODE 7);
 *   - the result is independent of partition, world size, launch shape and split into passes, as for either parent.
 *   srt_accum_reset_spectral_features  srt_accum_reset + a zeroed film, allocated by srt_accum_reset_spectral's rule, + zeroed feature
 *                             rows, allocated by srt_accum_reset_features' rule.  Refused with the previous accumulation unchanged: an
 *                             instrumented context (SRT_ERR_UNSUPPORTED); device parameters not set (SRT_ERR_INVALID); a failed
 *                             allocation (SRT_ERR_HIP; both blocks are allocated before either old one goes).  Invalidation, the
 *                             65535-sample limit and the chunk binding are those of srt_accum_reset.  The accumulation is spectral AND
 *                             featured: srt_read_spectral, srt_develop_spectral / _srgb, srt_read_features and srt_denoise_features /
 *                             _vg return on it what they return on the single-kind accumulations, and srt_denoise_developed, below,
 *                             needs it.  It is NOT adaptive: srt_accum_active, the sample map and S2 of srt_read_accum_stats and
 *                             srt_denoise_features_mv keep refusing it.  Every other srt_accum_reset* makes the next accumulation
 *                             something else again. */
SRT_API int srt_accum_reset_spectral_features(srt_ctx *ctx);

/* Adaptive sampling of the spectral film (no reference counterpart).  The film deposit is the most expensive thing a pass does per path
 * end, and adaptive sampling is what stops spending samples on pixels that have converged.  An ADAPTIVE SPECTRAL accumulation is an
 * adaptive accumulation (srt_accum_reset_adaptive: the same cfg, the same stopping rule on Y, the same state words and sample map) that
 * also keeps the film of srt_accum_reset_spectral (the same deposit rule); an ADAPTIVE SPECTRAL FEATURED accumulation keeps the feature
 * rows of srt_accum_reset_features as well.  Later srt_render_chunk_accum passes run render_kernel MODE 10 / MODE 11: MODE 4 with MODE 5's
 * deposit (and MODE 7's) compiled in, no new code in the hot loops (MODE 11's first-hit deposit adds one offset to its row address).  The
 * deposits draw nothing from the RNG and the stopping rule reads neither film nor rows.  What holds, and is tested, under the same cfg, seed and pass schedule:
 *   - the image, all nine planes, the XYZ sums, S2, the state words, the sample map, the active counts, srt_get_stats' paths and the RNG
 *     state are bit-identical to an adaptive accumulation's (MODE 4);
 *   - a pixel that stopped after n samples holds the film row of a plain spectral n-spp frame at that pixel, bit for bit; an active pixel
 *     holds the row of the running total; a converged pixel's film row is never touched again;
 *   - in the featured kind the eight feature sums are bit-identical to an adaptive featured accumulation's (MODE 8);
 *   - none of this depends on launch shape, partition, world size, chunk offset or the split into passes.
 *   srt_accum_reset_adaptive_spectral           validation, refusals and invalidation are srt_accum_reset_adaptive's (cfg as there; an
 *   srt_accum_reset_adaptive_spectral_features  instrumented context: SRT_ERR_UNSUPPORTED; device parameters not set: SRT_ERR_INVALID;
 *                             srt_set_gather_planes ends the accumulation); a failed allocation: SRT_ERR_HIP.  Every refusal leaves the
 *                             previous accumulation unchanged.  Buffers: the adaptive planes, the film (384 B per lane) and, featured,
 *                             the rows (32 B per lane; they live behind the film in the film's allocation).  The accumulation is adaptive
 *                             AND spectral (AND featured): srt_accum_active, srt_read_accum_stats, srt_read_spectral and
 *                             srt_develop_spectral (which still returns SUMS) take both kinds; srt_read_features and srt_denoise_features /
 *                             _vg / _mv take the featured kind as they take srt_accum_reset_adaptive_features', and refuse the other.
 *                             srt_develop_spectral_srgb on either kind normalises each pixel by its own count, n = n_p = the samples
 *                             field of the pixel's state word (a kernel of its own; a non-adaptive accumulation runs the kernel it
 *                             always ran; a pixel of another rank, n_p = 0, has +0 sums and is normalised by 1).  srt_denoise_developed
 *                             takes the featured kind: both prepasses use n_p,  d_p[k] = inv_p * D_p[k]  with  inv_p = 1.0f / (float)n_p
 *                             (the payload's by a kernel of its own), and out_xyz stays srt_denoise_features' out_xyz on the same
 *                             accumulation, bit for bit.  Every other srt_accum_reset* makes the next accumulation something else again;
 *                             a plain spectral accumulation still refuses srt_accum_active, a plain adaptive one srt_read_spectral.
 *                             Streams stay uncombined. */
SRT_API int srt_accum_reset_adaptive_spectral(srt_ctx *ctx, const srt_adaptive *cfg);
SRT_API int srt_accum_reset_adaptive_spectral_features(srt_ctx *ctx, const srt_adaptive *cfg);

/* Edge-avoiding a-trous denoiser over the first-hit feature buffers (no reference counterpart; kernels in csrc/srt_denoise.hip).  It
 * consumes a FEATURED accumulation: the XYZ sums are filtered by `levels` passes of a 5x5 B3-spline stencil whose taps are weighted down
 * where normal, albedo, hit distance or the colour itself differ.  The filter, operation by operation -- everything fp32, not contracted,
 * evaluated left to right as written, so that a float32 restatement (tests/denoise_reference.py) predicts the device's bits:
 *   Inputs, for the w x h rectangle of the accumulation's chunk (clipped to the grid of srt_init_device_params): S[p][3] the XYZ sums,
 *     F[p][8] the raw feature sums, n = the accumulation's sample total.
 *     (On an ADAPTIVE featured accumulation -- srt_accum_reset_adaptive_features -- n is the pixel's own count n_p, the samples field of
 *     its state word: inv = 1.0f / (float)n_p, by a prepass kernel of its own; the global total is not used, and nothing else in the filter
 *     changes.  With partition (0, 1) every pixel of the chunk holds at least the first pass's samples, so n_p > 0.)
 *   Prepass, per pixel:  inv = 1.0f / (float)n;  c_p = inv * S_p;  N_p = inv * F[0..2];  A_p = inv * F[3..5];
 *     z_p = F[7] > 0 ? F[6] / F[7] : 0.  A sample that missed counts as a zero vector: N and A fade with coverage, which so needs no
 *     term of its own.
 *   Level i = 0 .. levels-1: step s = 1 << i; taps h = {1/16, 1/4, 3/8, 1/4, 1/16} at offsets (dx * s, dy * s), dy = -2 .. 2 in the
 *     outer loop, dx = -2 .. 2 in the inner one; a tap outside the rectangle is skipped.  Per-level constants, computed on the host in
 *     fp32: kn = sigma_normal * sigma_normal, ka = sigma_albedo * sigma_albedo, kz = sigma_depth * sigma_depth, kc = sc * sc with
 *     sc = sigma_color * 2^-i (an exact scaling: the colour term tightens as the stencil widens).
 *     Edge term  e(d2, k):  t = 1 - d2 / k;  t = (t > 0) ? t : 0;  return t * t.     (NaN gives 0, an infinite k gives 1.)
 *     For tap q of pixel p:
 *       dn = (N_p.x - N_q.x)^2 + (N_p.y - N_q.y)^2 + (N_p.z - N_q.z)^2;   da the same on A;   dc the same on the level's input colour;
 *       m = z_p > z_q ? z_p : z_q;   r = m > 0 ? (z_p - z_q) / m : 0;   dz = r * r;
 *       wt = h[dy+2] * h[dx+2];  wt = wt * e(dn, kn);  wt = wt * e(da, ka);  wt = wt * e(dz, kz);  wt = wt * e(dc, kc);
 *       if (wt > 0) { sw += wt;  sx += wt * c_q.x;  sy += wt * c_q.y;  sz += wt * c_q.z; }
 *     Output of the level:  sw > 0 ? (sx / sw, sy / sw, sz / sw) : c_p.  Levels ping-pong between two images; levels == 0 returns c_p.
 *     (A pixel whose colour is NaN keeps it -- every one of its taps has wt = 0 -- and no neighbour takes it in.)
 *   Epilogue: the filtered XYZ mean goes through the render kernel's own conversion (XYZ -> linear sRGB rows, correct_channel,
 *     (float)(int)(v * 255.99f)): out_lin the unquantised, out_q the quantised sRGB.
 *   srt_denoise_features  filters the context's featured accumulation and writes out[((y * image_width) + x) * 3 + c] with the placement
 *                         of srt_read_features: only the chunk's rectangle is written (the filter always runs on the whole chunk; the
 *                         image clips only what is copied).  Any of the three outputs may be NULL, not all.  Synchronises.  It only
 *                         READS the accumulation: later passes, the frame, the feature rows and the RNG state are what they would be
 *                         without the call.  Working images (100 B per pixel of the chunk) belong to the context, are reused and grow
 *                         with the chunk.  Refused, the accumulation unchanged: null ctx / cfg, all outputs NULL, no featured accumulation
 *                         with at least one pass, levels > 8, a sigma that is NaN or <= 0 (+inf is allowed and switches its term off),
 *                         non-zero reserved words (SRT_ERR_INVALID); a partition other than (0, 1) (SRT_ERR_UNSUPPORTED: the neighbours
 *                         other ranks own read +0 here -- unless srt_unpack_accum / srt_comm_gather_accum has made the context whole); a
 *                         failed allocation (SRT_ERR_HIP).
 *   srt_denoise_kat       KAT entry point, like srt_order_tiles_kat: the same prepass, level and epilogue kernels on caller-supplied
 *                         row-major host arrays xyz_sums[h][w][3] and features[h][w][8] holding `samples` samples; out_xyz[h][w][3]
 *                         receives the filtered XYZ mean.  Needs neither a scene nor an accumulation and touches neither.
 *                         SRT_ERR_INVALID for a null argument, a cfg as above, samples == 0, an empty image or w x h >= 2^31. */
typedef struct srt_denoise { uint32_t levels; float sigma_color, sigma_normal, sigma_albedo, sigma_depth; uint32_t reserved[3]; } srt_denoise;
SRT_API int srt_denoise_features(srt_ctx *ctx, const srt_denoise *cfg, float *out_xyz, float *out_lin, float *out_q,
                                 uint32_t image_width, uint32_t image_height);
SRT_API int srt_denoise_kat(srt_ctx *ctx, const srt_denoise *cfg, const float *xyz_sums, const float *features,
                            uint32_t samples, uint32_t w, uint32_t h, float *out_xyz);
/* Kernel-only times of the context's last denoise (either entry point) in ms, from HIP events around each kernel: the prepass, level i in
 * level_ms[i] (8 entries; 0 from the call's `levels` on, which *levels receives), the epilogue.  Any pointer may be NULL.  Measurement
 * support (tools/denoise_cost.py), like srt_last_kernel_ms.  SRT_ERR_INVALID before the first denoise. */
SRT_API int srt_denoise_last_ms(srt_ctx *ctx, float *prepass_ms, float level_ms[8], float *epilogue_ms, uint32_t *levels);

/* Variance-guided mode of the a-trous denoiser (opt-in; the entry points above and their results are what they were).  The plain filter
 * stops at colour edges with one absolute width, sigma_color, so the same picture rendered four times brighter is filtered differently.
 * This mode compares a luminance difference to the pixel's own noise instead, as SVGF does (Schied et al. 2017, sections 4.2 - 4.4): it
 * estimates a per-pixel variance of the luminance, carries it through the levels, and scales the edge-stopping width with it.  The
 * plain featured accumulation keeps no second moments, so the estimate is SPATIAL (SVGF's answer for pixels without history): the
 * guide-weighted variance of Y over a 7x7 window.  Scaling the XYZ sums by a power of two s and variance_floor by s * s scales the
 * filtered XYZ by s and both variances by s * s, exactly (barring overflow and underflow).
 * The filter, operation by operation -- everything fp32, not contracted, left to right as written, selects and not fmax; the restatement
 * is tests/denoise_vg_reference.py.  Prepass, e(d2, k), dn, da, dz, kn, ka, kz and the B3 taps h are those of srt_denoise_features above;
 * Y is the colour's second component (XYZ's Y is luminance); dc is the plain filter's, on the level's input colour.
 *   Host constants, fp32: ks = sigma_variance * sigma_variance (formed once), vf = variance_floor.
 *   Estimator, per pixel p: taps q at offsets (dx, dy), dy = -3 .. 3 in the outer loop, dx = -3 .. 3 in the inner one (distance 1, the
 *     centre included); a tap outside the rectangle is skipped.
 *       g = e(dn, kn);  g = g * e(da, ka);  g = g * e(dz, kz);
 *       if (g > 0 && (Y_q - Y_q) == 0) { s0 += g;  s1 += g * Y_q;  s2 += g * (Y_q * Y_q); }       ((Y_q - Y_q) == 0: Y_q is finite.
 *         Without the clause one NaN or inf pixel would zero the variance of its whole 7x7 neighbourhood.)
 *       mu = s1 / s0;  m2 = s2 / s0;  v = m2 - mu * mu;  v_p = (s0 > 0 && v > 0) ? v : 0.        (NaN goes to 0.)
 *   Variance-guided level i = 0 .. levels-1, step s = 1 << i, from (c, v) to (c, v):
 *       vb_p: the 3x3 blur of the level's input v at distance 1 (not s), b = {1/4, 1/2, 1/4}, dy = -1 .. 1 outer, dx inner, a tap
 *         outside the rectangle skipped:  k = b[dy+1] * b[dx+1];  bk += k;  bv += k * v_q;   vb_p = bv / bk.
 *       kc_p = ks * vb_p + vf.
 *       For tap q of pixel p (the 25 taps of the plain level, in its order):
 *         d = Y_p - Y_q;  dl = d * d;
 *         wt = h[dy+2] * h[dx+2];  wt = wt * e(dn, kn);  wt = wt * e(da, ka);  wt = wt * e(dz, kz);  wt = wt * e(dl, kc_p);
 *         if (wt > 0 && (dc - dc) == 0) { sw += wt;  sx += wt * c_q.x;  sy += wt * c_q.y;  sz += wt * c_q.z;  sv += (wt * wt) * v_q; }
 *       Output of the level:  sw > 0 ? (sx / sw, sy / sw, sz / sw, sv / (sw * sw)) : (c_p, v_p).
 *       ((dc - dc) == 0: the colour difference is finite in all three components.  dl sees Y alone, so without the clause a pixel whose
 *        X or Z is inf or NaN would be taken in by its neighbours.  With it, a non-finite pixel keeps its colour and its variance and no
 *        neighbour takes it in, and at variance_floor = +inf -- e(dl, +inf) is 1 for a finite dl -- the colour output IS
 *        srt_denoise_features' at sigma_color = +inf, bit for bit, on every input: the plain filter is a special case.)
 *   Epilogue: unchanged.  levels == 0 returns (c_p, the estimate).
 *   srt_denoise_features_vg  srt_denoise_features in this mode: placement, clipping, synchronisation, the read-only behaviour towards the
 *                         accumulation and the partition refusal are its.  out_var[((y * image_width) + x) * 2 + k]: k = 0 the
 *                         estimator's variance, k = 1 the variance after the last level (equal at levels == 0).  Any of the four
 *                         outputs may be NULL, not all.  Working images: 108 B per pixel of the chunk.  Refused as srt_denoise_features
 *                         refuses, the accumulation unchanged, and for: levels > 8; sigma_variance NaN, <= 0 or infinite; a guide sigma
 *                         NaN or <= 0 (+inf still switches a guide off); variance_floor NaN or <= 0 (+inf is allowed and switches the
 *                         luminance term off); non-zero reserved words.
 *   srt_denoise_vg_kat    srt_denoise_kat in this mode; out_var[h][w][2] as above.  No argument may be NULL.
 *   srt_denoise_last_ms   works after either kind of denoise; after this one the epilogue's time includes the kernel that copies the
 *                         final variance out.  srt_denoise_estimate_last_ms gives the estimator kernel's time: SRT_ERR_INVALID when the
 *                         context's last denoise was not variance-guided (or none has run). */
typedef struct srt_denoise_vg { uint32_t levels; float sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor; uint32_t reserved[2]; } srt_denoise_vg;
SRT_API int srt_denoise_features_vg(srt_ctx *ctx, const srt_denoise_vg *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_var,
                                    uint32_t image_width, uint32_t image_height);
SRT_API int srt_denoise_vg_kat(srt_ctx *ctx, const srt_denoise_vg *cfg, const float *xyz_sums, const float *features,
                               uint32_t samples, uint32_t w, uint32_t h, float *out_xyz, float *out_var);
SRT_API int srt_denoise_estimate_last_ms(srt_ctx *ctx, float *ms);

/* Measured-variance mode: the variance-guided filter above, guided by the variance the sampler MEASURED instead of a spatial guess.  An
 * adaptive featured accumulation holds, per pixel, the count n_p, S1 (the Y sum) and S2 (the sum of squared per-sample Y): the stopping
 * rule's inputs.  cfg, its validation, the levels, the 3x3 variance blur, the epilogue, the placement and the refusals are those of
 * srt_denoise_features_vg; the prepass is the per-pixel-count one; only the estimator differs.  Per pixel, fp32, not contracted, left to
 * right, with n = (float)n_p:
 *       mean = S1 / n;  v = S2 / n - mean * mean;  v = v > 0 ? v : 0;  vm = v / (n - 1.0f);  v_p = (n_p >= 2 && (vm - vm) == 0) ? vm : 0
 * -- the first four operations of the stopping rule above (srt_accum_reset_adaptive), so the filter is guided by the very number the
 * sampler stopped on; a non-finite vm (a NaN or inf pixel) gives 0, as the spatial estimator does.
 *   srt_denoise_features_mv  needs an ADAPTIVE FEATURED accumulation holding spp_total >= 2, else SRT_ERR_INVALID (a plain featured
 *                         accumulation included): then every pixel holds at least two samples -- an active one the total, a converged one
 *                         at least min_spp >= 2.  out_var[..][0] is the estimate above, out_var[..][1] the variance after the last level.
 *                         At variance_floor = +inf the colour output equals srt_denoise_features at sigma_color = +inf on the same
 *                         accumulation, bit for bit: the plain filter stays a special case.  srt_denoise_estimate_last_ms reports this
 *                         estimator's kernel time.
 *   srt_denoise_mv_kat    the same kernels on caller-supplied row-major host arrays: xyz_sums[h][w][3], features[h][w][8],
 *                         samples[h][w] (the pixel's count in the low 31 bits, the layout of a state word) and sum_y2[h][w]; S1 is
 *                         xyz_sums[..][1].  The synthetic door to the per-pixel-count prepass and to the estimator (a pixel with
 *                         n_p = 1 gets v_p = 0).  A zero count anywhere in samples is SRT_ERR_INVALID, checked on the host; the other
 *                         refusals are srt_denoise_vg_kat's.  No argument may be NULL. */
SRT_API int srt_denoise_features_mv(srt_ctx *ctx, const srt_denoise_vg *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_var,
                                    uint32_t image_width, uint32_t image_height);
SRT_API int srt_denoise_mv_kat(srt_ctx *ctx, const srt_denoise_vg *cfg, const float *xyz_sums, const float *features,
                               const uint32_t *samples, const float *sum_y2, uint32_t w, uint32_t h, float *out_xyz, float *out_var);

/* The developed film, denoised: the plain a-trous filter of srt_denoise_features with a K-channel PAYLOAD (kernels in
 * csrc/srt_denoise.hip behind the others).  It needs a SPECTRAL FEATURED accumulation (srt_accum_reset_spectral_features, or the adaptive
 * srt_accum_reset_adaptive_spectral_features, on which n below is the pixel's own count n_p in both prepasses): the film is
 * developed through K response curves, and the K planes ride through the levels on the weights the XYZ colour and the guides produce.
 * Operation by operation -- everything fp32, not contracted, left to right; the restatement is tests/denoise_developed_reference.py:
 *   Develop:  D_p[k], k = 0 .. K-1, is the contraction stated at srt_develop_spectral (the same kernel): response[K][95], channels = K
 *     and scale are validated as there, 1 <= K <= SRT_MAX_DEVELOP_CHANNELS.
 *   Prepass:  srt_denoise_features' prepass, and in addition  d_p[k] = inv * D_p[k]  with the prepass's inv = 1.0f / (float)n.
 *   Level i:  the plain filter's tap loop and weights, unchanged -- wt = h[dy+2] * h[dx+2], then * e(dn, kn), * e(da, ka), * e(dz, kz),
 *     * e(dc, kc), dc on the level's XYZ colour, never on the payload -- and inside the same  if (wt > 0) { .. },  after sz:
 *       sd[k] += wt * d_q[k]   for k = 0 .. K-1
 *     Output of the level:  sw > 0 ? sd[k] / sw : d_p[k],  next to the unchanged colour output.  Colour and payload both ping-pong
 *     through the levels; levels == 0 returns (c_p, d_p).
 *     What follows: the weights never see the payload; every channel is filtered by the same stencil; a tap with wt == 0 never
 *     multiplies its payload, so a non-finite payload there does not enter; a pixel whose colour is NaN keeps its own payload and no
 *     neighbour takes it in; a payload NaN at a tap with wt > 0 propagates as the arithmetic says.
 *   Outputs:  out_dev[((y * image_width) + x) * K + k] the filtered developed mean; out_xyz[((y * image_width) + x) * 3 + c] the
 *     filtered XYZ mean, which is bit-identical to srt_denoise_features' out_xyz on the same accumulation and cfg.  Either may be NULL,
 *     not both.
 *   srt_denoise_developed placement, clipping, synchronisation, the read-only behaviour towards the accumulation and the partition
 *                         refusal are srt_denoise_features'.  Refused, the accumulation unchanged: a null ctx / cfg / response, both
 *                         outputs NULL, an empty image, a cfg as srt_denoise_features refuses it, response / channels / scale as
 *                         srt_develop_spectral refuses them, an accumulation that is not spectral AND featured with at least one pass --
 *                         a plain spectral, a plain featured and an adaptive featured one are all refused -- (SRT_ERR_INVALID); a
 *                         partition other than (0, 1) (SRT_ERR_UNSUPPORTED); a failed allocation (SRT_ERR_HIP).  Working images: the
 *                         plain filter's and the develop's, plus 2 * KC * 4 + K * 4 bytes per pixel of the chunk for the payload, KC
 *                         the smallest of 4, 8, 16 that holds K.  srt_denoise_last_ms and srt_develop_last_ms report this call's
 *                         kernels (prepass: both prepasses; level i: the payload level; epilogue: both output kernels).
 *   srt_denoise_developed_kat  the same prepass, level and output kernels on caller-supplied row-major host arrays xyz_sums[h][w][3],
 *                         features[h][w][8] and developed[h][w][K] (the planes D, sums over `samples` samples: no develop runs);
 *                         out_dev[h][w][K] and out_xyz[h][w][3], either may be NULL, not both.  Needs neither a scene nor an
 *                         accumulation and touches neither.  SRT_ERR_INVALID for a null input, a cfg as above, channels == 0 or >
 *                         SRT_MAX_DEVELOP_CHANNELS, samples == 0, an empty image or w x h >= 2^31.
 *   srt_denoise_developed_counts_kat  the same with a per-pixel sample map samples[h][w] (each >= 1; bit 31 is ignored, as in a state
 *                         word) in the place of the scalar: the kernels an adaptive spectral featured accumulation runs -- both
 *                         per-pixel-count prepasses, the same levels and output kernels.  With a constant map it equals
 *                         srt_denoise_developed_kat bit for bit.  Checks as srt_denoise_developed_kat's, and as srt_denoise_mv_kat's for
 *                         the map: a null map or a zero in it is SRT_ERR_INVALID. */
SRT_API int srt_denoise_developed(srt_ctx *ctx, const srt_denoise *cfg, const float *response, uint32_t channels, float scale,
                                  float *out_dev, float *out_xyz, uint32_t image_width, uint32_t image_height);
SRT_API int srt_denoise_developed_kat(srt_ctx *ctx, const srt_denoise *cfg, const float *xyz_sums, const float *features,
                                      const float *developed, uint32_t channels, uint32_t samples, uint32_t w, uint32_t h,
                                      float *out_dev, float *out_xyz);
SRT_API int srt_denoise_developed_counts_kat(srt_ctx *ctx, const srt_denoise *cfg, const float *xyz_sums, const float *features,
                                             const float *developed, uint32_t channels, const uint32_t *samples, uint32_t w, uint32_t h,
                                             float *out_dev, float *out_xyz);

/* The presented picture (no reference counterpart; kernels in csrc/srt_present.hip): the bound accumulation through a chosen chain --
 * nothing, a denoiser or a develop; then the meter or a given gain; then the tone curve -- without leaving the device, into the 4 bytes per
 * pixel a display, an encoder or an image writer wants.  Only the packed picture crosses the bus (and the three counters, and the 16 KiB
 * histogram when metering), through a pinned staging block of the context.  Operation by operation:
 *   Source (cfg->source), each stage the existing call's kernels on the chunk's rectangle (clipped to the reference grid), w x h pixels:
 *     SRT_PRESENT_ACCUM        the XYZ sums, normalised in present_kernel as the tone kernel normalises them: inv = 1.0f / (float)n, n the
 *                              sample total, on an adaptive kind the pixel's own count (0 counts as 1); c = inv * S per component.
 *     SRT_PRESENT_DENOISE      srt_denoise_features' filter (cfg->denoise); the picture is its out_xyz, left on the device.
 *     SRT_PRESENT_DENOISE_VG   srt_denoise_features_vg's (cfg->denoise_vg); SRT_PRESENT_DENOISE_MV: srt_denoise_features_mv's.
 *     SRT_PRESENT_DEVELOP      srt_develop_spectral_srgb's contraction of the film with cfg->response3 (three curves [3][95] taken as X,
 *                              Y, Z; NULL: the colour-matching rows of srt_color_tables) and cfg->scale, D; then m = inv * D per component
 *                              with the inv of that call's epilogue (the sample total, or the pixel's own count, 0 counting as 1): the
 *                              XYZ mean its out_lin / out_q are made of.  (out_xyz of that call is D, the sums: m = inv * out_xyz.)
 *   Exposure: cfg->metered != 0 meters the source picture -- srt_meter_accum on SRT_PRESENT_ACCUM, else the meter kernel on the device
 *     array as srt_meter_kat runs it on a host array, under the context's partition -- with cfg->meter, decides as srt_meter_decide decides
 *     and takes the gain decided; cfg->tone.gain is validated but not used.  cfg->metered == 0: the gain is cfg->tone.gain.
 *   Tone and pack, per pixel with XYZ mean c: o = Tone(c) and (lin, q) = xyz_mean_to_srgb(o) exactly as stated at "Tone" above; q holds
 *     whole numbers in 0 .. 255 always (a NaN channel fails every compare of the transfer function and comes out 255), and the pixel's
 *     word is  (uint32)q.r | (uint32)q.g << 8 | (uint32)q.b << 16 | 255 << 24:  byte 0 R, byte 1 G, byte 2 B, byte 3 A = 255 -- the bytes of
 *     srt_expose_accum's / srt_expose_kat's out_q.  blown, crushed and nonfinite are counted as the tone kernel counts them, over the
 *     pixels of this rank's tiles.  A pixel of another rank's tile holds +0 and comes out as (0, 0, 0, 255).
 *     The kernel handles four consecutive pixels of a row per thread with 16-byte accesses where the group is whole and 16-byte aligned
 *     and pixel by pixel elsewhere; the bytes do not depend on the path.
 *   srt_present           runs the chain and writes row j of the picture at out_rgba8 + (offy + j) * pitch_bytes + 4 * offx.  Placement
 *                         and clipping are srt_expose_accum's: the image receives the part of the chunk's rectangle inside image_width x
 *                         image_height at the chunk's offset, and no other byte of the caller's buffer -- padding included -- is written.
 *                         *result, unless NULL, receives the metering (all zero when the gain was given) and the counters.  Synchronises;
 *                         only reads the accumulation.  Refusals are those of the calls it chains, nothing changed and nothing written:
 *                         SRT_ERR_INVALID for a null ctx / cfg / out_rgba8, non-zero reserved words, an unknown source, an empty image,
 *                         pitch_bytes < 4 * image_width, a bad srt_tone, with metering a bad srt_meter (a rectangle outside the chunk
 *                         included), a bad srt_denoise / srt_denoise_vg of a denoising source, non-finite curves or scale of
 *                         SRT_PRESENT_DEVELOP, no accumulation with a pass, a denoising source without a featured accumulation
 *                         (SRT_PRESENT_DENOISE_MV: an adaptive featured one holding at least 2 samples), SRT_PRESENT_DEVELOP without a
 *                         film; SRT_ERR_UNSUPPORTED for a denoising source under a partition other than (0, 1); SRT_ERR_HIP for a failed
 *                         allocation.  The configuration of a stage the source does not run is not read.
 *   srt_present_kat       present_kernel on a caller's row-major host array xyz_mean[h][w][3] at tone->gain; out_rgba8[h][w][4], tightly
 *                         packed; result may be NULL.  Needs neither a scene nor an accumulation.  Refusals as srt_expose_kat's.
 *   srt_present_last_ms   kernel-only time in ms, from HIP events, of the context's last present_kernel; SRT_ERR_INVALID before one has
 *                         run.  srt_denoise_last_ms, srt_develop_last_ms and srt_expose_last_ms report the stages srt_present ran.
 * Working blocks (four bytes per pixel on the device and in pinned host memory, grown on demand; twelve more per pixel on the device for a
 * developed mean) belong to the context and are freed with it.  No call here invalidates or alters an accumulation, the frame or the
 * RNG state. */
#define SRT_PRESENT_ACCUM 0
#define SRT_PRESENT_DENOISE 1
#define SRT_PRESENT_DENOISE_VG 2
#define SRT_PRESENT_DENOISE_MV 3
#define SRT_PRESENT_DEVELOP 4
typedef struct srt_present_cfg {
    uint32_t source;               /* SRT_PRESENT_* */
    uint32_t metered;              /* != 0: the gain is metered with `meter`; 0: tone.gain */
    srt_meter meter;
    srt_tone tone;
    srt_denoise denoise;           /* SRT_PRESENT_DENOISE */
    srt_denoise_vg denoise_vg;     /* SRT_PRESENT_DENOISE_VG, SRT_PRESENT_DENOISE_MV */
    const float *response3;        /* SRT_PRESENT_DEVELOP: [3][95], NULL = the colour-matching rows */
    float scale;                   /* SRT_PRESENT_DEVELOP */
    uint32_t reserved[5];          /* must be 0 */
} srt_present_cfg;
typedef struct srt_present_result { srt_meter_result meter; srt_tone_result tone; } srt_present_result;
SRT_API int srt_present(srt_ctx *ctx, const srt_present_cfg *cfg, uint8_t *out_rgba8, size_t pitch_bytes, uint32_t image_width,
                        uint32_t image_height, srt_present_result *result);
SRT_API int srt_present_kat(srt_ctx *ctx, const srt_tone *tone, const float *xyz_mean, uint32_t w, uint32_t h, uint8_t *out_rgba8,
                            srt_tone_result *result);
SRT_API int srt_present_last_ms(srt_ctx *ctx, float *ms);

/* The firefly filter (no reference counterpart; kernel in csrc/srt_despeckle.hip): a rank-based outlier clamp on the XYZ mean, ahead of the
 * denoiser.  The path finds a light only by hitting it, so a sparse picture holds isolated pixels far above all their neighbours; the
 * a-trous filter keeps such a pixel by construction (every tap's colour weight is 0, and it returns the pixel itself).  The clamp scales a
 * pixel whose luminance exceeds a limit taken from a rank statistic of its neighbours down to that limit, keeping its chromaticity.
 * Operation by operation -- everything fp32, not contracted, evaluated left to right, with compares and selects only; the restatement is
 * tests/despeckle_reference.py, which the device equals in every integer and every bit:
 *   The input is a w x h picture of XYZ means c.  From an accumulation it is c = inv * S with inv = 1.0f / (float)n, where n is the
 *     sample total; on an adaptive kind n is the pixel's own count, and 0 counts as 1, as tone_kernel normalises.
 *   cfg is srt_despeckle { uint32_t radius, rank_ppm; float gain, floor; uint32_t reserved[4]; }.
 *   For pixel p, over the window of offsets (dx, dy) with |dx|, |dy| <= radius and the centre excluded:
 *     valid(q)  :=  q inside the rectangle  &&  (Y_q - Y_q) == 0            (Y = the second component)
 *     v_q        =  Y_q > 0 ? Y_q : +0.0f                                   (negatives and both zeros become +0)
 *     m          =  number of valid q;   u_0 <= u_1 <= .. <= u_{m-1}  the v_q in ascending order
 *     k          =  (uint64)(m - 1) * rank_ppm / 1000000;    ref = u_k      (500000: lower median; 1000000: the largest)
 *     limit      =  gain * ref;   limit = limit + floor
 *     classes, the tests in this order:
 *       1. nonfinite: (v - v) == 0 is false for a component v of c_p   ->  o = c_p, s = 1.0f
 *       2. alone:     m == 0                                           ->  o = c_p, s = 1.0f
 *       3. clamped:   Y_p > limit    ->  s = limit / Y_p;  o = (s * c_p.x, s * c_p.y, s * c_p.z)
 *       4. kept:      otherwise      ->  o = c_p (its bits), s = 1.0f
 *   ref is a rank statistic of canonical non-negative values, where equal values have equal bits: it does not depend on the order in
 *   which the window is read or sorted.  The counters clamped, nonfinite and alone are integers, added with atomics after a wave-level
 *   reduction, as the tone kernel counts.  A non-finite pixel is neither repaired nor used as a neighbour.
 *   What follows: a picture scaled by 2^k with floor scaled by 2^k (no overflow, no underflow) gives the same classes and exactly 2^k
 *   times the output; flipping or transposing the picture commutes with the filter, bit for bit; floor = +inf makes limit = +inf and the
 *   output the input, bit for bit.
 *   cfg, validated by every entry point that takes one, else SRT_ERR_INVALID: radius 1 or 2; rank_ppm <= 1000000; gain finite and >= 0;
 *     floor >= 0 and not NaN (+inf allowed: the filter is off); the reserved words 0.
 *   srt_despeckle_accum     the filter on the bound accumulation of ANY kind, streamed included.  out_xyz is o, out_lin / out_q are
 *                           xyz_mean_to_srgb(o) (three floats per pixel each), out_scale[h][w] is s; *result the three counters.  Any
 *                           output may be NULL, but not all four together with result.  Placement, clipping, synchronisation and the
 *                           read-only behaviour are srt_expose_accum's.  SRT_ERR_INVALID as srt_expose_accum's (a bad srt_despeckle in the
 *                           place of a bad srt_tone); SRT_ERR_UNSUPPORTED under a partition other than (0, 1), as the denoisers':
 *                           a pixel's neighbours must be on this context.
 *   srt_despeckle_kat       the same kernel on a caller's row-major host array xyz_mean[h][w][3]; out_xyz [h][w][3], out_scale [h][w],
 *                           either may be NULL, not both together with result.  Refusals as srt_expose_kat's.
 *   srt_despeckle_last_ms   kernel-only time in ms, from HIP events, of the context's last despeckle kernel; SRT_ERR_INVALID before one ran.
 *   srt_denoise_features_ds srt_denoise_features with one stage added between the prepass and level 0: colour[1] = Despeckle(colour[0])
 *                           on the denoiser's float4 colour image (the fourth word carried through); the levels start from colour[1], the
 *                           guides are untouched, and levels == 0 returns the despeckled mean.  Refusals are srt_denoise_features' plus a
 *                           bad srt_despeckle.  At floor = +inf it equals srt_denoise_features, bit for bit.  srt_denoise_last_ms reports
 *                           prepass, levels and epilogue as before; the stage's time is srt_despeckle_last_ms.
 *   srt_present_despeckled  srt_present with the stage in front.  SRT_PRESENT_ACCUM presents -- and, when metering, meters -- the
 *                           despeckled picture, which lies on the device as [h][w][3], as srt_meter_kat would; SRT_PRESENT_DENOISE runs
 *                           the chain of srt_denoise_features_ds.  Other sources and every partition other than (0, 1) are
 *                           SRT_ERR_UNSUPPORTED; the other refusals are srt_present's plus a bad or null srt_despeckle.  *despeckle_result,
 *                           unless NULL, receives the stage's counters.
 * Working blocks (32 bytes of counters and ten floats per pixel of the rectangle) belong to the context and are reused.  No call here
 * invalidates or alters an accumulation, the frame or the RNG state. */
typedef struct srt_despeckle { uint32_t radius, rank_ppm; float gain, floor; uint32_t reserved[4]; } srt_despeckle;
typedef struct srt_despeckle_result { uint64_t clamped, nonfinite, alone; } srt_despeckle_result;
SRT_API int srt_despeckle_accum(srt_ctx *ctx, const srt_despeckle *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_scale,
                                srt_despeckle_result *result, uint32_t image_width, uint32_t image_height);
SRT_API int srt_despeckle_kat(srt_ctx *ctx, const srt_despeckle *cfg, const float *xyz_mean, uint32_t w, uint32_t h,
                              float *out_xyz, float *out_scale, srt_despeckle_result *result);
SRT_API int srt_despeckle_last_ms(srt_ctx *ctx, float *ms);
SRT_API int srt_denoise_features_ds(srt_ctx *ctx, const srt_despeckle *despeckle_cfg, const srt_denoise *denoise_cfg,
                                    float *out_xyz, float *out_lin, float *out_q, uint32_t image_width, uint32_t image_height);
SRT_API int srt_present_despeckled(srt_ctx *ctx, const srt_present_cfg *present_cfg, const srt_despeckle *despeckle_cfg, uint8_t *out_rgba8,
                                   size_t pitch_bytes, uint32_t image_width, uint32_t image_height, srt_present_result *result,
                                   srt_despeckle_result *despeckle_result);

/* Temporal reprojection (no reference counterpart; kernel in csrc/srt_temporal.hip): the picture carried across camera moves.
 * srt_set_camera invalidates the accumulation, so a moved camera starts its picture from nothing although nearly every surface it sees was
 * seen a frame ago.  This stage finds, for every pixel, where its surface lay in the previous frame -- from the first-hit guides and the
 * two cameras, which are plain data -- gathers the previous output there, and blends the new frame into it with a weight that falls as the
 * history grows: the temporal half of an SVGF-style filter (Schied et al. 2017, section 4.1), next to the spatial and variance-guided
 * halves above.  The motion vectors fall out of the same arithmetic.  The geometry is static; lens and jitter are ignored (the centre ray).
 * Operation by operation -- everything fp32, not contracted, evaluated left to right, with only + - * /, sqrtf, floorf, float <-> int
 * conversion, compares and selects; the restatement is tests/temporal_reference.py, which the device equals in every bit and every counter:
 *   A dot product is  a.b = (a.x * b.x + a.y * b.y) + a.z * b.z;  a cross product is
 *     a x b = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x);  a vector operation is done per component.
 *   Inputs, for the w x h rectangle of the chunk at image offset (ox, oy): the current picture c_p (an XYZ mean), its guides
 *     g0_p = (N, z) and g1_p = (A, cov) as srt_denoise_features' prepass defines them (on an adaptive kind with the pixel's own count), the
 *     current camera C (du = pixel_delta_u, dv = pixel_delta_v, p00 = pixel00_loc, center = camera_center), and the HISTORY: three float4
 *     images of the same rectangle written by the previous call -- Hc = (XYZ, len), Hg0, Hg1 (that call's guides) -- and the camera C'
 *     that was current then.
 *   cfg is srt_temporal { float alpha_min, max_len, sigma_normal, sigma_albedo, sigma_depth; uint32_t reserved[3]; }.
 *   Host constants, fp32:  kn = sigma_normal * sigma_normal;  ka = sigma_albedo * sigma_albedo;  kz = sigma_depth * sigma_depth  (+inf
 *     stays +inf and switches its test off);  and of the previous camera C':
 *       n' = du' x dv';   e' = p00' - center';   k' = e'.n';
 *       cu = dv' x n';    bu' = cu / (du'.cu);       cv = n' x du';    bv' = cv / (dv'.cv)
 *     (the reciprocal basis of (du', dv') in the image plane: bu'.du' = 1, bu'.dv' = 0 and so on, also for a non-orthogonal camera).
 *   Per pixel p = (x, y):
 *     1. Class:  hit_p = cov_p >= 0.5f.
 *     2. Centre ray of C, as the render kernel forms pixel_center, without jitter and lens:
 *          fi = (float)(ox + x);  fj = (float)(oy + y);  pc = (p00 + fi * du) + fj * dv;  d = pc - center.
 *     3. Point or direction.  hit_p:  L = sqrtf(d.d);  s = z_p / L;  P = center + s * d;  v = P - center';  zexp = sqrtf(v.v).
 *          Otherwise (sky):  v = d.
 *     4. Projection into C':  den = v.n';  t = k' / den.  If (t > 0) is false there is no history for p (behind the camera, a parallel ray, or
 *          NaN), and its motion vector is (NaN, NaN).  Otherwise  q = t * v - e';  u = q.bu' - (float)ox;  w = q.bv' - (float)oy,  and the
 *          motion vector is (u - (float)x, w - (float)y).
 *     5. Bilinear gather:  x0 = floorf(u);  y0 = floorf(w);  fx = u - x0;  fy = w - y0.  The taps are (x0 + a, y0 + b) in the order
 *          (a, b) = (0, 0), (1, 0), (0, 1), (1, 1), with  wt = (a ? fx : 1.0f - fx) * (b ? fy : 1.0f - fy).  A tap q = (tx, ty) is INSIDE when
 *          tx >= 0 && tx < (float)w && ty >= 0 && ty < (float)h, tested in float: a huge or NaN coordinate is never converted, and no tap
 *          outside is read.  A tap inside is ACCEPTED when  Hc_q.len > 0,  the three colour components of Hc_q are finite ((v - v) == 0),
 *          and (Hg1_q.cov >= 0.5f) == hit_p;  for a hit pixel also
 *            (N_p.x - N_q.x)^2 + (N_p.y - N_q.y)^2 + (N_p.z - N_q.z)^2 <= kn  (N_q of Hg0_q),   the same on A (of Hg1_q) <= ka,   and
 *            m = zexp > z_q ? zexp : z_q;   r = m > 0 ? (zexp - z_q) / m : 0;   r * r <= kz      (z_q of Hg0_q).
 *          An accepted tap with wt > 0:  sw += wt;  sc += wt * Hc_q.xyz;  sl += wt * Hc_q.len.
 *     6. Result classes, the tests in this order:
 *          nonfinite: (v - v) == 0 is false for a component v of c_p  ->  o = c_p, len' = 0.  The pixel is shown as it is and leaves no history.
 *          fresh:     there is no history at all, step 4 failed, or (sw > 0) is false  ->  o = c_p, len' = 1.
 *          blended:   h = sc / sw;  lh = sl / sw;  len' = lh + 1.0f;  len' = len' < max_len ? len' : max_len;  a = 1.0f / len';
 *                     a = a > alpha_min ? a : alpha_min;   a >= 1 ? o = c_p (its bits) : o = h + a * (c_p - h).
 *     7. New history:  Hc = (o, len'), Hg0 = g0_p, Hg1 = g1_p, camera = C.  The history is double-buffered -- a call reads the old one while
 *          it writes the new --, costs 96 bytes per pixel of the rectangle and belongs to the context.
 *   Counters (integers, added with atomics after a wave-level reduction, as the tone kernel counts): blended, fresh and nonfinite are the
 *     classes; a fresh pixel is also counted as offscreen (step 4 failed or all four taps are outside) or else as rejected -- unless
 *     there is no history at all, when it is neither.  With no history at all steps 2 - 5 are not run and every motion vector is NaN.
 *   What follows: the first call after a reset returns the input picture bit for bit, with len = 1 (0 at a non-finite pixel);
 *   alpha_min = 1 returns the input picture bit for bit, whatever the history; a constant picture under any camera move stays that constant
 *   exactly where it blends (c - h = 0: h is a weighted mean of equal values only up to rounding, so this needs sc / sw to be that
 *   constant: it is for one tap, and for a constant with few mantissa bits); a non-finite value never enters the history (the nonfinite
 *   class stores len' = 0, which no later gather accepts; barring overflow in the sums) and never leaves it (a tap with non-finite colour
 *   is not accepted).
 *   cfg, validated by every entry point that takes one, else SRT_ERR_INVALID: 0 < alpha_min <= 1; max_len >= 1 and finite; every sigma > 0
 *     and not NaN (+inf allowed); the reserved words 0.
 *   srt_temporal_reset      drops the context's history: the next call is a first frame.  srt_upload_scene, srt_init_device_params and
 *                           srt_set_partition drop it too; srt_set_camera and every srt_accum_reset* do NOT -- surviving them is the point.
 *   srt_temporal_accum      the stage on the bound FEATURED accumulation of any kind the denoisers accept (plain, adaptive, spectral,
 *                           adaptive spectral): srt_denoise_features' prepass forms c and the guides, C is the context's camera.  out_xyz
 *                           is o, out_lin / out_q are xyz_mean_to_srgb(o) (three floats per pixel each), out_len[h][w] is len',
 *                           out_motion[h][w][2] the motion vector; *result the counters.  Any output may be NULL, but not all five
 *                           together with result.  Placement, clipping and synchronisation are srt_despeckle_accum's.  It reads the
 *                           accumulation and ADVANCES THE HISTORY: frame, sums, rows, sample map and RNG state are untouched.  A history
 *                           of another rectangle (w, h, ox, oy) is discarded -- history_dropped = 1 -- and the call is a first frame.
 *                           Refusals are srt_denoise_features' (SRT_ERR_UNSUPPORTED under a partition other than (0, 1)) plus a bad cfg;
 *                           a refused call leaves the history alone.
 *   srt_temporal_kat        the same kernel on a caller's row-major host arrays: xyz_mean[h][w][3], guides[h][w][8] = (N, z, A, cov),
 *                           hist_colour[h][w][4] = Hc, hist_guides[h][w][8] = (Hg0, Hg1), the rectangle's offset (ox, oy), both cameras.
 *                           prev_cam == NULL or hist_colour == NULL or hist_guides == NULL: no history.  out_colour[h][w][4] the new Hc,
 *                           out_guides[h][w][8] the new guides, out_motion[h][w][2]; any may be NULL, not all three together with result.
 *                           It touches neither the context's history nor any accumulation.  SRT_ERR_INVALID for a null ctx / cfg /
 *                           cur_cam / xyz_mean / guides, a bad cfg, an empty image, w x h >= 2^31, or ox + w or oy + h above 2^24 (where
 *                           fi and fj stop being exact).  history_frames is 1 without a history and 2 with one.
 *   srt_denoise_features_temporal  srt_denoise_features -- with despeckle_cfg not NULL: srt_denoise_features_ds -- with the stage between
 *                           the prepass (and the despeckle) and level 0, on the denoiser's own images.  The history is the stage's output,
 *                           not the filtered picture, and it is the history srt_temporal_accum keeps: the two calls may alternate.  With
 *                           no history it equals srt_denoise_features / _ds bit for bit.  Refusals are theirs plus a bad srt_temporal.
 *   srt_present_temporal    srt_present with the stage (behind the despeckle when despeckle_cfg is not NULL) in front, structured as
 *                           srt_present_despeckled is: SRT_PRESENT_ACCUM presents -- and, when metering, meters -- the stage's output,
 *                           which lies on the device as [h][w][3]; SRT_PRESENT_DENOISE runs the chain of srt_denoise_features_temporal.
 *                           Other sources and every partition other than (0, 1) are SRT_ERR_UNSUPPORTED; the other refusals are
 *                           srt_present's plus a null or bad srt_temporal, a bad srt_despeckle, and an accumulation that is not featured.
 *   srt_temporal_last_ms    kernel-only time in ms, from HIP events, of the context's last temporal kernel; SRT_ERR_INVALID before one ran.
 *                           srt_denoise_last_ms reports the chained call's prepass, levels and epilogue as before; srt_temporal_accum
 *                           records no denoise event, so after it srt_denoise_last_ms still reports the context's last denoise.
 * history_frames is the number of calls since the history began, this one included.  Working blocks (64 bytes of counters, the 96 bytes per
 * pixel of the history, 48 more for the outputs, and the denoiser's images) belong to the context and are reused. */
typedef struct srt_temporal { float alpha_min, max_len, sigma_normal, sigma_albedo, sigma_depth; uint32_t reserved[3]; } srt_temporal;
typedef struct srt_temporal_result {
    uint64_t blended, fresh, offscreen, rejected, nonfinite;
    uint32_t history_frames;       /* calls since the history began, this one included */
    uint32_t history_dropped;      /* 1: this call found a history of another rectangle and discarded it */
} srt_temporal_result;
SRT_API int srt_temporal_reset(srt_ctx *ctx);
SRT_API int srt_temporal_accum(srt_ctx *ctx, const srt_temporal *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_len,
                               float *out_motion, srt_temporal_result *result, uint32_t image_width, uint32_t image_height);
SRT_API int srt_temporal_kat(srt_ctx *ctx, const srt_temporal *cfg, const srt_camera_data *cur_cam, const srt_camera_data *prev_cam,
                             const float *xyz_mean, const float *guides, const float *hist_colour, const float *hist_guides,
                             uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, float *out_colour, float *out_guides, float *out_motion,
                             srt_temporal_result *result);
SRT_API int srt_denoise_features_temporal(srt_ctx *ctx, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg,
                                          const srt_denoise *denoise_cfg, float *out_xyz, float *out_lin, float *out_q,
                                          srt_temporal_result *temporal_result, uint32_t image_width, uint32_t image_height);
SRT_API int srt_present_temporal(srt_ctx *ctx, const srt_present_cfg *present_cfg, const srt_temporal *temporal_cfg,
                                 const srt_despeckle *despeckle_cfg, uint8_t *out_rgba8, size_t pitch_bytes, uint32_t image_width,
                                 uint32_t image_height, srt_present_result *result, srt_temporal_result *temporal_result);
SRT_API int srt_temporal_last_ms(srt_ctx *ctx, float *ms);

/* Surface motion (no reference counterpart; kernel in csrc/srt_motion.hip): the temporal history carried across refits.  The stage above
 * knows camera motion only, so a refit drops its history.  With TRACKING on, a context keeps the vertices its scene images were last made
 * from and the vertices at the moment the history was written; one pass finds, for every pixel, the surface point its centre ray sees and
 * moves that point back to where the same point of the same triangle lay then; the *_moving variants of the temporal calls project that
 * point in the place of the one they would reconstruct from the distance guide.  The same pass is a primary-visibility buffer (triangle,
 * barycentrics, distance per pixel) for picking and compositing.  Tracking is opt-in and off by default: with it off nothing of this
 * state exists and every call above behaves as stated above.
 * Operation by operation -- fp32, not contracted, left to right, dot products as the temporal section defines them; the restatement is
 * tests/surface_motion_reference.py, which the device equals in every bit and every counter -- for pixel (x, y) of the w x h rectangle at
 * image offset (ox, oy), camera C, the vertex blocks V_cur and V_prev (n_tris x 9 floats, row k = triangle k = the index srt_trace_rays
 * reports = srt_refit_vertices' row k):
 *     1. Centre ray, as temporal step 2:  fi = (float)(ox + x);  fj = (float)(oy + y);  pc = (p00 + fi * du) + fj * dv;  d = pc - center;
 *          origin center.
 *     2. Closest hit:  (t, k) as srt_trace_rays answers the ray (center, d): the same traversal on the same records.  t is in units of
 *          the unnormalised d; k = -1 is a miss.
 *     3. Miss:  point = (0, 0, 0, 0), tri = -1, bary = (0, 0, 0).  No vertex row is read.
 *     4. Hit:  P = center + t * d;  (a, b, c) = row k of V_cur, (a', b', c') = row k of V_prev;
 *          e1 = b - a;  e2 = c - a;  r = P - a;  d11 = e1.e1;  d12 = e1.e2;  d22 = e2.e2;  r1 = r.e1;  r2 = r.e2;
 *          den = d11 * d22 - d12 * d12;  beta = (d22 * r1 - d12 * r2) / den;  gamma = (d11 * r2 - d12 * r1) / den;
 *          Da = a' - a;  Db = b' - b;  Dc = c' - c;  moved = one of their nine components is != 0.
 *          Not moved:  Pprev = P (its bits), valid = 1.
 *          Moved:  disp = (Da + beta * (Db - Da)) + gamma * (Dc - Da);  Pprev = P + disp;  valid = den > 0 and beta, gamma and the three
 *            components of Pprev are finite ((v - v) == 0).
 *          point = (Pprev, valid ? 1.0f : 0.0f), the three coordinates +0 when not valid;  tri = k;  bary = (t, beta, gamma).
 *   Counters (integers: a wave sum, the workgroup's word in LDS, one atomic per workgroup and non-zero counter): hit, miss, moved (hit
 *   pixels whose triangle moved), degenerate (moved and not valid).  A triangle that is degenerate in V_prev alone stays valid: den is
 *   V_cur's.
 * The vertex state of a tracking context, always in the order of the context's calls on the NULL stream:
 *   srt_temporal_track_motion(on)  switches tracking (default 0).  Switching on or off drops the temporal history and forgets both blocks:
 *                           until the next srt_upload_scene or successful refit the vertices are UNKNOWN, and srt_surface_motion and the
 *                           three bound *_moving calls refuse with SRT_ERR_INVALID.  Setting the value it already has changes nothing.
 *   srt_temporal_tracking   reports the switch and refits_pending, the successful refits since the history was last written.
 *   srt_upload_scene        V_cur = the scene's vertices, kept on the host until first use (an upload enqueues and allocates nothing for
 *                           this, as for the refit's tables); V_hist = none; the history is dropped, as always.
 *   a successful refit      V_cur = the new vertices (a device-to-device copy from srt_refit_vertices_dev, host-to-device otherwise); if
 *                           V_hist was none and a history exists, V_hist first becomes the old V_cur; refits_pending += 1; THE TEMPORAL
 *                           HISTORY IS KEPT -- the one thing tracking changes about a refit; everything else is invalidated as stated at
 *                           srt_refit_vertices.  A refused refit changes nothing.
 *   a *_moving call that advances the history  uses V_prev = V_hist, or V_cur when V_hist is none; afterwards V_hist = none ("equal to
 *                           V_cur": no copy) and refits_pending = 0.
 *   srt_temporal_accum, srt_denoise_features_temporal, srt_present_temporal with refits_pending > 0  discard the history, which shows
 *                           geometry that has moved, and are a first frame (history_frames == 1) -- what they are after a refit without
 *                           tracking; afterwards V_hist = none and refits_pending = 0.
 *   srt_temporal_reset, srt_init_device_params, srt_set_partition  drop the history as always; V_hist = none, refits_pending = 0.
 * Entry points:
 *   srt_surface_motion      the pass on the context's camera, the uploaded scene and V_prev as defined above, for any rectangle and under
 *                           any partition (a query, not a render: tiles of other ranks are traced like the rest).  out_point[h][w][4],
 *                           out_tri[h][w] (int32), out_bary[h][w][3], *result; any may be NULL, not all three together with result.  Needs
 *                           tracking on, known vertices and a camera.  Synchronises.  It only reads: neither history nor refits_pending
 *                           nor any image, sum or RNG state moves.
 *   srt_surface_motion_kat  the same kernel on the uploaded scene, the camera cam and the caller's vertex arrays: prev_verts_host (NULL:
 *                           nothing moved) and cur_verts_host, n_tris x 9 floats each.  cur_verts_host must be the vertices the uploaded
 *                           scene images were made from: THE CALLER'S PROMISE, which nothing checks.  Works with tracking off and touches
 *                           no context state.  SRT_ERR_INVALID: no scene uploaded, a null ctx / cam / cur_verts_host, n_tris not the
 *                           scene's, a coordinate that is not finite, an empty rectangle, no output, ox + w or oy + h above 2^24,
 *                           w x h >= 2^31.
 *   srt_motion_last_ms      kernel-only time in ms, from HIP events, of the context's last motion kernel; SRT_ERR_INVALID before one ran.
 *   srt_temporal_moving_kat srt_temporal_kat plus prev_point[h][w][4] (not NULL): the moving stage.  It is srt_temporal_accum's stage in
 *                           every operation except that step 3 of a hit pixel (cov_p >= 0.5f) reads M = prev_point[p]:
 *                             M.w == 1:  v = M.xyz - center';  zexp = sqrtf(v.v).
 *                             Otherwise step 4 counts as failed: no history for p, motion vector (NaN, NaN), fresh and offscreen.
 *                           Sky pixels take v = d as before.  Fed the point the static stage reconstructs it equals srt_temporal_kat bit
 *                           for bit.  The normal and albedo tests still compare the current guides with the history's: a surface that
 *                           turns by more than sigma_normal between two frames is rejected and starts fresh -- safe, and a stated
 *                           limitation (no expected-normal correction).
 *   srt_temporal_accum_moving, srt_denoise_features_temporal_moving, srt_present_temporal_moving  their siblings with the motion pass on
 *                           the accumulation's rectangle in front of the moving stage; *motion_result (may be NULL) receives the pass's
 *                           counters.  They advance the history and the vertex state as stated above.  Refusals are their siblings' plus
 *                           tracking off or vertices unknown (SRT_ERR_INVALID); a refused call leaves history and vertex state alone.
 * Working blocks (two vertex blocks of 36 bytes per triangle, 64 bytes of counters, 32 bytes per pixel of the rectangle) belong to the
 * context and are reused.  Out of scope: an expected-normal correction, lens- and jitter-aware reprojection, motion of materials, topology
 * changes, a gathered (multi-rank) temporal stage. */
typedef struct srt_motion_result { uint64_t hit, miss, moved, degenerate; } srt_motion_result;
SRT_API int srt_temporal_track_motion(srt_ctx *ctx, int on);
SRT_API int srt_temporal_tracking(const srt_ctx *ctx, int *on, uint32_t *refits_pending);
SRT_API int srt_surface_motion(srt_ctx *ctx, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, float *out_point, int32_t *out_tri,
                               float *out_bary, srt_motion_result *result);
SRT_API int srt_surface_motion_kat(srt_ctx *ctx, const srt_camera_data *cam, const float *prev_verts_host, const float *cur_verts_host,
                                   size_t n_tris, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, float *out_point, int32_t *out_tri,
                                   float *out_bary, srt_motion_result *result);
SRT_API int srt_motion_last_ms(srt_ctx *ctx, float *ms);
SRT_API int srt_temporal_accum_moving(srt_ctx *ctx, const srt_temporal *cfg, float *out_xyz, float *out_lin, float *out_q, float *out_len,
                                      float *out_motion, srt_temporal_result *result, uint32_t image_width, uint32_t image_height,
                                      srt_motion_result *motion_result);
SRT_API int srt_temporal_moving_kat(srt_ctx *ctx, const srt_temporal *cfg, const srt_camera_data *cur_cam, const srt_camera_data *prev_cam,
                                    const float *xyz_mean, const float *guides, const float *hist_colour, const float *hist_guides,
                                    uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, float *out_colour, float *out_guides,
                                    float *out_motion, srt_temporal_result *result, const float *prev_point);
SRT_API int srt_denoise_features_temporal_moving(srt_ctx *ctx, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg,
                                                 const srt_denoise *denoise_cfg, float *out_xyz, float *out_lin, float *out_q,
                                                 srt_temporal_result *temporal_result, uint32_t image_width, uint32_t image_height,
                                                 srt_motion_result *motion_result);
SRT_API int srt_present_temporal_moving(srt_ctx *ctx, const srt_present_cfg *present_cfg, const srt_temporal *temporal_cfg,
                                        const srt_despeckle *despeckle_cfg, uint8_t *out_rgba8, size_t pitch_bytes, uint32_t image_width,
                                        uint32_t image_height, srt_present_result *result, srt_temporal_result *temporal_result,
                                        srt_motion_result *motion_result);

/* Variance measured across frames (no reference counterpart; kernels in csrc/srt_temporal.hip): the two halves of the SVGF-style filter
 * joined.  The temporal stage above carries colour and length; the variance-guided filter has only a spatial guess of the noise, a 7x7
 * window of one frame.  Here the stage also carries the first and second LUMINANCE MOMENTS through the same reprojection (Schied et al.
 * 2017, section 4.2), and the a-trous levels are guided by the variance those moments measure wherever the history is long enough, by the
 * spatial estimate elsewhere: a pixel with a long history is filtered gently, a disoccluded one hard.  Opt-in: every call above keeps
 * its results, its history bytes and its refusals.
 * The moments history Hm: a second, optional, double-buffered image of the history's rectangle, one float4 per pixel, (m1, m2, mlen, 0) --
 * 32 bytes per pixel more, allocated by the first call that asks for it.  mlen is the moments' own length: it lets a colour history that
 * moment-less calls advanced be joined later.
 * The moments ride on the stage of srt_temporal_accum (the moving variant: of srt_temporal_moving_kat) exactly: taps, acceptance tests,
 * weights wt, classes, alpha_min and max_len are unchanged, and the colour, the length, the guides, the motion vectors and the counters
 * are that stage's, bit for bit.  Everything fp32, not contracted, left to right, compares and selects only; the restatement is
 * tests/temporal_vg_reference.py.  Y = c_p.y and Q = Y * Y, c_p the stage's input picture (in the chained call: behind the firefly clamp).
 *     Step 5, for every tap the colour takes (accepted, wt > 0), when a moments history exists:
 *          s1 += wt * Hm_q.x;  s2 += wt * Hm_q.y;  sm += wt * Hm_q.z.
 *     Step 6:
 *          nonfinite:  Hm' = (0, 0, 0, 0).
 *          fresh, or blended with no moments history:  Hm' = (Y, Q, 1, 0).
 *          blended with a moments history:  g1 = s1 / sw;  g2 = s2 / sw;  lm = sm / sw;  ml = lm + 1.0f;  ml = ml < max_len ? ml : max_len;
 *                     b = 1.0f / ml;  b = b > alpha_min ? b : alpha_min;
 *                     b >= 1 ? (m1', m2') = (Y, Q) : (m1', m2') = (g1 + b * (Y - g1), g2 + b * (Q - g2));   Hm' = (m1', m2', ml, 0).
 *   Rules of the moments history: any of the moment-less temporal calls above advances Hc / Hg as always and marks Hm ABSENT; the next
 *   moments call then seeds Hm' = (Y, Q, 1, 0) at every finite pixel, so the two families may alternate; whatever drops the colour
 *   history (srt_temporal_reset, an upload, another rectangle, ...) drops the moments with it.
 * The choice of the variance, a small elementwise kernel of its own.  Per pixel, from Hm' and len' of the stage, vs_p of the spatial
 * estimator of srt_denoise_features_vg run on the stage's output o (and its guides), and ml_min = (float)min_len:
 *          d = m2' - m1' * m1';  d = d > 0 ? d : 0;  vt = d / len';
 *          use = (mlen' >= ml_min) && (len' > 0) && ((vt - vt) == 0);   v_p = use ? vt : vs_p.
 *   d / len' is the variance of a mean of len' frames: exact while the blend weight is a = 1 / len', an approximation once alpha_min or
 *   max_len holds a up -- the mean then forgets old frames and its variance stops falling; sigma_variance absorbs the constant.  v_p goes
 *   where the estimator's result goes: the colour image's fourth word and out_var[..][0].  n_temporal, the number of pixels with `use`, is
 *   an integer counter reduced per wave, then per workgroup, as the stage's counters are.
 * typedef struct srt_temporal_vg { uint32_t min_len; uint32_t moving; uint32_t reserved[2]; }: valid when 2 <= min_len <= 2^24, moving is 0
 *   or 1 and the reserved words are 0, else SRT_ERR_INVALID.  min_len > max_len: the variance is always the spatial one (n_temporal = 0).
 *   moving = 1 needs what srt_denoise_features_temporal_moving needs and is refused as that call refuses.  min_len = 4 and
 *   sigma_variance = 2 are starting values, untuned.
 *   srt_denoise_features_temporal_vg  the chain: srt_denoise_features' prepass, the firefly filter when despeckle_cfg is not NULL, the
 *                           moments stage (moving = 1: the surface-motion pass and the moving variant), the spatial estimator on o, the
 *                           choice, the levels of srt_denoise_features_vg from (o, v), the epilogue.  out_xyz / out_lin / out_q as
 *                           srt_denoise_features_vg's; out_var[h][w][2] is laid out as that call's: [0] the variance chosen, [1] the
 *                           variance behind the last level.  *temporal_result the stage's counters, *n_temporal (uint64_t, may be NULL)
 *                           the choice's, *motion_result (may be NULL) the motion pass's when moving.  The history stays the stage's
 *                           output, not the filtered picture.  Refusals are the union of the chained calls' (srt_denoise_features_vg,
 *                           srt_denoise_features_temporal(_moving), a bad srt_despeckle) plus a null or bad srt_temporal_vg; a refused call
 *                           leaves both histories alone.  srt_temporal_result does not grow: that is why n_temporal is a parameter.
 *   srt_present_temporal_vg srt_present_temporal with the chain above for the source SRT_PRESENT_DENOISE_VG (cfg->denoise_vg); every other
 *                           source is SRT_ERR_UNSUPPORTED.
 *   srt_temporal_moments_kat  srt_temporal_kat plus prev_point[h][w][4] (NULL: the static stage, else srt_temporal_moving_kat's),
 *                           hist_moments[h][w][4] (NULL: no moments history; not read without a colour history) and out_moments[h][w][4],
 *                           the new Hm.  It touches no context history.
 *   srt_temporal_variance_kat  the choice kernel alone on host arrays: moments[h][w][4] = Hm', len[h][w] = len', spatial_var[h][w] = vs;
 *                           out_var[h][w] = v and *n_temporal; either may be NULL, not both.  SRT_ERR_INVALID for a null input, an empty
 *                           image, w x h >= 2^31, min_len outside 2 .. 2^24.
 *   srt_read_temporal_moments  the context's current Hm as out[h][w][4], placed and clipped as srt_temporal_accum's outputs are.
 *                           SRT_ERR_INVALID when Hm is absent.
 *   srt_temporal_variance_last_ms  kernel-only time in ms of the context's last choice kernel; SRT_ERR_INVALID before one ran.
 *                           srt_temporal_last_ms, srt_denoise_last_ms and srt_denoise_estimate_last_ms keep reporting their kernels
 *                           after the new calls. */
typedef struct srt_temporal_vg { uint32_t min_len; uint32_t moving; uint32_t reserved[2]; } srt_temporal_vg;
SRT_API int srt_denoise_features_temporal_vg(srt_ctx *ctx, const srt_temporal *temporal_cfg, const srt_despeckle *despeckle_cfg,
                                             const srt_denoise_vg *vg_cfg, const srt_temporal_vg *tv_cfg, float *out_xyz, float *out_lin,
                                             float *out_q, float *out_var, srt_temporal_result *temporal_result, uint64_t *n_temporal,
                                             srt_motion_result *motion_result, uint32_t image_width, uint32_t image_height);
SRT_API int srt_present_temporal_vg(srt_ctx *ctx, const srt_present_cfg *present_cfg, const srt_temporal *temporal_cfg,
                                    const srt_despeckle *despeckle_cfg, const srt_temporal_vg *tv_cfg, uint8_t *out_rgba8,
                                    size_t pitch_bytes, uint32_t image_width, uint32_t image_height, srt_present_result *result,
                                    srt_temporal_result *temporal_result, uint64_t *n_temporal, srt_motion_result *motion_result);
SRT_API int srt_temporal_moments_kat(srt_ctx *ctx, const srt_temporal *cfg, const srt_camera_data *cur_cam, const srt_camera_data *prev_cam,
                                     const float *xyz_mean, const float *guides, const float *hist_colour, const float *hist_guides,
                                     uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, float *out_colour, float *out_guides,
                                     float *out_motion, srt_temporal_result *result, const float *prev_point, const float *hist_moments,
                                     float *out_moments);
SRT_API int srt_temporal_variance_kat(srt_ctx *ctx, const float *moments, const float *len, const float *spatial_var, uint32_t min_len,
                                      uint32_t w, uint32_t h, float *out_var, uint64_t *n_temporal);
SRT_API int srt_read_temporal_moments(srt_ctx *ctx, float *out, uint32_t image_width, uint32_t image_height);
SRT_API int srt_temporal_variance_last_ms(srt_ctx *ctx, float *ms);

/* Sample-parallel pixels (no reference counterpart; a deliberate departure from its one RNG stream per pixel, so opt-in).  A STREAMED
 * accumulation gives every pixel K independent RNG streams, each with its own state and its own XYZ sum, so that any lane of any wave
 * can render a stream while others render the pixel's other streams: the longest sequential chain of a pass is spp_add / K samples.
 * Streams.  With n_lanes = tx * bx * ty * by of srt_init_device_params, stream k of lane idx is XORWOW(seed + k * n_lanes + idx): exactly
 *   the state that lane has in a context initialised with seed_k = seed + k * n_lanes.  Stream 0 is the context's own RNG state.  Streams
 *   1 .. K-1 are kept by the context (stream-major planes of K * n_lanes words), seeded from the seed of the last srt_init_device_params at
 *   the first streamed reset after it, and they continue across resets and accumulations until the next srt_init_device_params, as
 *   stream 0 does: stream k behaves as the RNG state of a context initialised with seed_k that has rendered the same launches.  (A reset
 *   with ANOTHER K re-lays the planes and seeds streams 1 .. K-1 afresh from seed_k; stream 0 continues.)
 * Passes.  srt_render_chunk_accum on a streamed accumulation needs spp_add % K == 0; every stream of every pixel of the chunk draws
 *   spp_add / K samples.  srt_accum_samples reports the total over the streams, and the 65535 limit applies to that total.
 * Result after passes totalling n samples.  S_k = the XYZ sum a plain accumulation (srt_accum_reset) of a context seeded seed_k holds
 *   after n / K samples, same bits.  The pixel's sum is ((S_0 + S_1) + S_2) + ... + S_{K-1}, per component, fp32, not contracted: the XYZ
 *   parity group, srt_read_accum_stats' sum_y and everything derived from them use it.  The unquantised and quantised sRGB planes are the
 *   plain conversion of (1.0f / (float)n) * sum, the one every render launch applies.  So a K-stream frame is, bit for bit, a fixed-order
 *   fp32 sum of K plain frames, and K = 1 equals srt_accum_reset in every output.  The result does not depend on partition, world size,
 *   launch shape, queue order or the split into passes.  A plain srt_render_chunk after a streamed accumulation continues stream 0.
 * Queue.  A pass runs the cost probe's queue with every row repeated K times, one copy per stream, the copies adjacent, so that the K
 *   streams of an expensive tile start on K different workgroups (render_kernel MODE 6); a kernel after the pass adds the K sums of
 *   every pixel in stream order and writes the tile buffer.  The probe itself walks a copy of stream 0, as ever.
 *   srt_accum_reset_streams   srt_accum_reset + zeroed per-stream sum planes (12 B x K per lane of the grid) and the per-stream RNG states
 *                             (24 B x K per lane), allocated on first use and when K or n_lanes grows.  1 <= K <= SRT_MAX_STREAMS.
 *                             Refused with the previous accumulation unchanged: K == 0 or K > 16, device parameters not set, K x n_lanes
 *                             >= 2^31 (SRT_ERR_INVALID); an instrumented context (SRT_ERR_UNSUPPORTED); a failed allocation (SRT_ERR_HIP).
 *                             srt_accum_reset, srt_accum_reset_adaptive and srt_accum_reset_spectral make the next accumulation
 *                             non-streamed again.  Streams combined with adaptive sampling or with the spectral film are NOT supported
 *                             (adaptive streams are the obvious next step).  Invalidation and the chunk binding are those of
 *                             srt_accum_reset.  A pass is refused with nothing changed on the device (SRT_ERR_INVALID) when spp_add is
 *                             no multiple of K, the total would pass 65535, the chunk or offset is another one, or local tiles x K x 64
 *                             reaches 2^32 (the queue's slot counter); srt_get_stats after a pass: paths = pixels x spp_add.
 *   srt_accum_streams         K of the context's streamed accumulation; 0 when its accumulation is not streamed (or there is none). */
#define SRT_MAX_STREAMS 16
SRT_API int srt_accum_reset_streams(srt_ctx *ctx, uint32_t streams);
SRT_API int srt_accum_streams(const srt_ctx *ctx, uint32_t *streams);

/* Compact tile buffer of this rank (device memory): three plane GROUPS of tiles_padded * 3 * 64 floats each,
 * [group][tile][plane][lane] -- group 0 = quantised r,g,b (the reference's frame_buffer values, 12 B / pixel), group 1 =
 * unquantised sRGB r,g,b, group 2 = XYZ sums (parity planes).  tiles_padded = ceil(n_tiles/world), so every rank's buffer has
 * the same size.  `planes` = 3 (default): the render kernel writes group 0 only, and group 0 is what a scatter / the multi-GPU
 * gather moves -- what the reference's framebuffer holds; `planes` = 9: the kernel also writes the two parity groups
 * and scatter / gather move all three (parity tests that compare unquantised sRGB or XYZ sums; srt_read_fb_aux needs it).  Set it
 * before srt_render_chunk.  srt_tile_buffer reports n_floats = tiles_padded * planes * 64. */
SRT_API int srt_set_gather_planes(srt_ctx *ctx, uint32_t planes);
SRT_API int srt_tile_buffer(srt_ctx *ctx, void **dev_ptr, size_t *n_floats, uint32_t *tiles_local, uint32_t *tiles_padded);
/* Stream-ordered device-to-device copy of the exchange unit into caller-owned device memory (e.g. the tensor that is
 * handed to the RCCL gather): n_floats as reported by srt_tile_buffer. */
SRT_API int srt_copy_tile_buffer(srt_ctx *ctx, void *dst_dev, void *stream);
/* Scatter gathered exchange units (device pointer, world * tiles_padded * planes * 64 floats, rank-major) into this
 * context's block-linear planar framebuffer (rendering.cu:146-148 layout); with planes == 3 only the quantised planes are
 * written.  With world == 1 pass NULL: the context's own tile buffer (its first `planes` planes) is scattered. */
SRT_API int srt_scatter_tiles(srt_ctx *ctx, const void *dev_gathered, void *stream);

/* Gathering an accumulation (no reference counterpart).  The tile buffer above carries the finished picture of a partition; the
 * accumulation itself -- XYZ sums, sample map and S2, feature rows, film -- stays in the block-linear buffers of the context that
 * rendered it, and a pixel another rank owns reads +0 there.  Every such buffer is indexed by the lane of the WHOLE grid on every rank,
 * and a pass touches only its own tiles, so the records of the other ranks' tiles can be copied into a context's own buffers: it then
 * holds exactly the accumulation a partition (0, 1) context would hold after the same passes, and every stage runs on it unchanged.
 * These three calls mirror srt_tile_buffer / srt_copy_tile_buffer / srt_scatter_tiles for a caller with a transport of its own;
 * srt_comm_gather_accum is the same over RCCL.
 *   parts                   SRT_GATHER_*: what travels.  The sums always do (SRT_GATHER_SUMS is implied); COUNTS is the per-pixel state
 *                           word (samples held | converged flag) and S2 of an adaptive accumulation, FEATURES the first-hit rows of a
 *                           featured one, FILM the film of a spectral one (384 B per pixel: it moves only when it is asked for).
 *                           parts == 0 stands for everything the accumulation's kind holds except the film.  A streamed accumulation
 *                           holds -- and moves -- its combined sums only: the per-stream sums and RNG states stay where they are.
 *   srt_accum_exchange_size *n_floats = the exchange unit for `parts`: tiles_padded * 64 * (3 + 2 a + 8 f + 96 s) floats, a, f, s = 1
 *                           where COUNTS, FEATURES, FILM travel; the same on every rank of the partition.
 *   srt_pack_accum          this rank's own tiles, out of the accumulation buffers into dst_dev (device memory, n_floats floats; 16-byte
 *                           aligned memory takes the wide path).  Slots outside the chunk and tile records past the rank's last tile
 *                           are +0: the unit is a function of the accumulation alone.  Words that are not floats travel as their bit
 *                           patterns in float slots (hand a transport ncclFloat).
 *   srt_unpack_accum        dev_gathered = `world` units, rank-major (what ncclGather leaves at its root), into this context's
 *                           accumulation buffers, for every tile the context does not own.  Its own records are neither read nor
 *                           written, and its RNG state is untouched: its next pass continues as if nothing had happened.  With
 *                           world == 1 it succeeds and enqueues nothing.
 *   srt_accum_gathered      *parts = what the last unpack since the last pass brought (0: nothing).
 *   srt_accum_whole         *whole = 1 when the context is whole (below) for a stage that reads `parts` -- FEATURES and FILM as the
 *                           stage needs them; the sums, and the counts of an adaptive accumulation, are implied -- else 0.
 *   srt_gather_last_ms      the kernel times of the context's last pack and last unpack (0 where there was none).
 * Pack and unpack are asynchronous on `hip_stream` (a hipStream_t passed as void*, NULL = default stream, as srt_render_chunk's `stream`)
 * and belong to the calls that take a stream ("Order of a context's calls").
 * A context is WHOLE for a stage when its partition is (0, 1), or when the last unpack since its last pass brought every part that
 * stage reads (the sums; COUNTS for an adaptive accumulation; FEATURES for the denoisers and the temporal stage; FILM and FEATURES for
 * srt_denoise_developed).  The stages that refuse a partition -- srt_despeckle_accum, srt_denoise_features*, srt_denoise_developed,
 * srt_temporal_accum*, the chained srt_present_* calls -- run on a whole context, and the per-rank counters of srt_meter_accum,
 * srt_expose_accum and srt_present* then count every pixel, as under partition (0, 1): results and counters equal that context's.
 * The mark is cleared by every pass on the context, by every srt_accum_reset* and by everything that invalidates the accumulation.
 * After a later pass the pixels of the other ranks are STALE until the next gather: the stages that need the whole chunk refuse again,
 * and the stages that accept a partition see the stale records where they used to see +0.  Gather before you look.
 * The temporal history belongs to the context and survives all of this, as it survives srt_set_camera.
 * Refused with nothing changed: no accumulation with a pass, a part the kind does not hold, an unknown bit, a null pointer
 * (SRT_ERR_INVALID); an instrumented context (SRT_ERR_UNSUPPORTED). */
#define SRT_GATHER_SUMS 1u
#define SRT_GATHER_COUNTS 2u
#define SRT_GATHER_FEATURES 4u
#define SRT_GATHER_FILM 8u
SRT_API int srt_accum_exchange_size(srt_ctx *ctx, uint32_t parts, size_t *n_floats);
SRT_API int srt_pack_accum(srt_ctx *ctx, uint32_t parts, void *dst_dev, void *hip_stream);
SRT_API int srt_unpack_accum(srt_ctx *ctx, uint32_t parts, const void *dev_gathered, void *hip_stream);
SRT_API int srt_accum_gathered(const srt_ctx *ctx, uint32_t *parts);
SRT_API int srt_accum_whole(const srt_ctx *ctx, uint32_t parts, int *whole);
SRT_API int srt_gather_last_ms(srt_ctx *ctx, float *pack_ms, float *unpack_ms);

/* renderer::getDevFBr/g/b (rendering.cuh:87-97): device pointers to the block-linear planes (tx*bx*ty*by floats). */
SRT_API int srt_dev_fb(srt_ctx *ctx, void **r, void **g, void **b, size_t *n_floats);
/* The three cudaMemcpyAsync D2H of render_manager::step (render_manager.cu:41-45): block-linear, grid sized. */
SRT_API int srt_read_fb(srt_ctx *ctx, float *r, float *g, float *b);
/* D2H + the un-swizzle of render_manager::update_fb (render_manager.cuh:68-142) done on the device:
 * writes the last rendered chunk into row-major image planes of width image_width at (offx, offy). */
SRT_API int srt_read_fb_rowmajor(srt_ctx *ctx, float *r, float *g, float *b, uint32_t image_width, uint32_t image_height);
/* Parity planes, block-linear: which = 1 unquantised sRGB in [0,1] (value before expand_sRGB), 2 = XYZ sums.  ANY context -- single
 * GPU included -- writes them only when srt_set_gather_planes(ctx, 9) was called before srt_render_chunk: with the default 3 planes
 * the kernel and the scatter move the quantised framebuffer alone and this call returns SRT_ERR_UNSUPPORTED. */
SRT_API int srt_read_fb_aux(srt_ctx *ctx, int which, float *p0, float *p1, float *p2);

/* Scheduling introspection: per-local-tile traversal cost measured by the probe of the last ordered launch (n = tiles_local; n = 2 *
 * tiles_local: followed by the cost of every tile's most expensive pixel -- one pixel is one sequential chain). */
SRT_API int srt_get_tile_costs(srt_ctx *ctx, uint32_t *out, size_t n);
/* Child order of a built tree from a profile of the real rays (no reference counterpart: the reference's bvh::hit, bvh/bvh.cu:98-166,
 * always descends left first, so the order is a property of the tree it is given).  Renders ONE instrumented probe frame of the
 * context's camera (width x height, spp, bounce_limit; srt_set_camera first) in which every closest-hit query notes, at each
 * ancestor of the triangle it found, whether the other child's box lay on the ray beyond the hit -- the rays for which the visiting
 * order decides whether that subtree is pruned -- and swaps the children of every node where the right child won more often (at
 * least min_samples such rays; other nodes keep their order).  The scene is left re-ordered AND uploaded to ctx; topology, boxes,
 * depth unchanged; results can only differ where two triangles tie exactly in t.  Call srt_init_device_params afterwards (the
 * probe used the context's RNG state).  n_swapped may be NULL. */
SRT_API int srt_order_children_by_profile(srt_ctx *ctx, srt_scene *scene, uint32_t width, uint32_t height, uint32_t spp,
                                          uint32_t bounce_limit, uint32_t min_samples, uint32_t *n_swapped);
/* Pixels of a width x height frame per persistent lane of one of `world` ranks' launches of the uploaded scene on ctx: below about 6 a
 * launch is bound by its longest pixel chain, above by total work. */
SRT_API int srt_pixels_per_lane(const srt_ctx *ctx, uint32_t width, uint32_t height, uint32_t world, double *out);
/* What srt_tune_tree_for_throughput found and did. */
typedef struct srt_tree_tuning {
    double   pixels_per_lane;      /* width*height / world / (CUs * waves per CU * 64) of the scene's launch on ctx */
    uint32_t throughput_bound;     /* pixels_per_lane >= 6 */
    uint32_t reinsertion;          /* 0 not tried (more than 8192 triangles, or not tuned), 1 kept (3 passes against box areas), 2 undone:
                                    * tree restored (it would leave LDS, or its objective rose), 3 kept (3 passes against the frame's sampled
                                    * queries), 4 vetoed: the sampled frame's work counters did not fall on the new tree, the tree is as it
                                    * walked in, 5 no usable segment in the sample: the topology is as it walked in */
    uint32_t probe_width, probe_height, probe_spp;   /* 0 when no probe frame ran */
    uint32_t nodes_swapped;
    int32_t  order_status;         /* SRT_OK, or what srt_order_children_by_profile returned (its message in srt_last_error) */
    uint32_t segments;             /* usable segments the ray-weighted passes counted (0 when they did not run) */
} srt_tree_tuning;
/* Tree tuning for a THROUGHPUT-bound render of a width x height frame on `world` ranks (no reference counterpart: the tree is an
 * input of bvh::hit, bvh/bvh.cu:98-166) -- the one recipe of every front end, so that they traverse the same tree for
 * the same workload.  When a rank's launch has at least 6 pixels per persistent lane, a tree of up to 8 192 triangles is post-optimised
 * against the frame's own rays: one instrumented frame of the scene's default camera at a twelfth of the frame's size (at least 32 x 32),
 * 1 sample per pixel, records every closest-hit query (srt_collect_ray_segments, stride 1), 2 048 of them, taken evenly through their
 * canonical order, drive 3 reinsertion passes (srt_scene_optimise_bvh_for_rays; put back exactly as it was if the deeper tree would no
 * longer be LDS resident), and the same frame is rendered again on the new tree: unless its work counters (node records + 2 x triangle
 * tests) fell, the tree that walked in is put back (out->reinsertion tells).  A launch with fewer pixels per lane that is tuned all the
 * same (only_if_throughput_bound == 0) gets the 3 passes against box areas it always got (srt_scene_optimise_bvh, same LDS rule).  Then
 * the child order is measured on one instrumented probe frame of the scene's default camera at a quarter of the frame's size (at least
 * 32 x 32), 8 samples per pixel, nodes with at least 16 deciding rays (srt_order_children_by_profile, which undoes itself when the
 * probe frame did not get cheaper).  Launches with fewer pixels per lane are bound by their longest pixel, which a tree with less total
 * work does not shorten: with only_if_throughput_bound != 0 they keep the tree untouched (out->throughput_bound == 0).  Deterministic.
 * A failing profile call is reported in out->order_status; the return value covers the arguments and the first upload.
 * Side effects on ctx are srt_order_children_by_profile's: the scene is left uploaded, the camera is replaced by the probe's, any
 * accumulation is invalidated, and srt_init_device_params comes next. */
SRT_API int srt_tune_tree_for_throughput(srt_ctx *ctx, srt_scene *scene, uint32_t width, uint32_t height, uint32_t world,
                                         uint32_t bounce_limit, int only_if_throughput_bound, srt_tree_tuning *out);
/* The same recipe with the caller's sample in place of the recorded one (segments[n_segments][7] as srt_collect_ray_segments returns them;
 * thinned to 2 048 like the recorded sample): what the recipe does with a sample can be checked without depending on what a frame casts.
 * The two frames that decide the veto are rendered as ever. */
SRT_API int srt_tune_tree_with_segments(srt_ctx *ctx, srt_scene *scene, uint32_t width, uint32_t height, uint32_t world, uint32_t bounce_limit,
                                        int only_if_throughput_bound, const float *segments, size_t n_segments, srt_tree_tuning *out);
/* A sample of a frame's closest-hit queries (no reference counterpart; instrumented kernel).  Renders ONE instrumented frame of the
 * context's camera and uploaded scene (width x height, spp, bounce_limit; the grid and seed of srt_order_children_by_profile's probe
 * frames) in which every finished closest-hit query whose direction is not NaN -- those never walk the tree -- takes a ticket 0, 1, 2 ..
 * from one counter; ticket t is recorded when (t + seed % stride) % stride == 0, as origin xyz, direction xyz (not normalised) and t_end:
 * the closest hit, FLT_MAX for a miss.  *n_queries (optional) = tickets taken = srt_stats.rays - srt_stats.util[2] of the frame;
 * *n_segments = the recorded ones, at most `capacity` (the later ones are dropped), written to segments[*n_segments][7] in ascending
 * order of their bit patterns.  With stride 1 every query is recorded and the array is the same in every run; with a larger stride WHICH
 * queries hold the sampled tickets depends on the order in which the waves finish them.  The production kernels are not involved; the
 * context's frame buffer, RNG state and grid are the frame's afterwards: srt_init_device_params comes next. */
SRT_API int srt_collect_ray_segments(srt_ctx *ctx, uint32_t width, uint32_t height, uint32_t spp, uint32_t bounce_limit, uint32_t stride,
                                     uint64_t seed, float *segments, size_t capacity, size_t *n_segments, uint64_t *n_queries);
SRT_API int srt_get_stats(srt_ctx *ctx, srt_stats *out);       /* counters of the last srt_render_chunk (or _accum pass) */
SRT_API int srt_set_count_traversal(srt_ctx *ctx, int on);     /* 1: instrumented kernel also counts V / T */
/* Instrumented launches only (diagnostics of the tail of a launch): 4 words per persistent wave -- [0] its life time and [1] the
 * moment the pixel queue first came back empty for it (both in units of 256 shader cycles since the wave started; [1] = 2^32-1 if
 * never), [2] its closest-hit queries, [3] the queries of its most expensive pixel.  n_waves <= srt_stats.waves[0]. */
SRT_API int srt_get_wave_debug(srt_ctx *ctx, uint32_t *out, size_t n_waves);
/* Kernel-only time of the last srt_render_chunk in ms, measured with HIP events on its stream. */
SRT_API int srt_last_kernel_ms(srt_ctx *ctx, float *ms);
/* Closest-hit query for explicit rays (bvh::hit, bvh/bvh.cu:98-166) -- KAT entry point.
 * rays: n * 6 floats (origin, direction); out: n * 4 floats (t, tri_index or -1, front_face, mat_index). */
SRT_API int srt_trace_rays(srt_ctx *ctx, const float *rays, size_t n, float *out);
/* Ray queries (no reference counterpart): batched closest-hit and any-hit queries over an interval of t, in one persistent kernel
 * (srt_query.hip) in the shape of the scene's render launch plan -- the inner records the plan caches in LDS, 16- or 32-bit references,
 * the PAIRED variant where srt_launch_paired says so; the test knobs apply.
 *   Ray row.  rays[n][8] = ox, oy, oz, tmin, dx, dy, dz, tmax (float32; t in units of |d|, as everywhere).
 *   The query is bvh::hit of srt_trace_rays with the interval as arguments, operation by operation (c = closest so far, m = min(t1x, t1y,
 * t1z) and t0x .. t0z the slab entries of a child box, t and inside exactly what srt_trace_rays computes for a triangle):
 *     start            c = fminf(tmax, FLT_MAX): tmax = +inf is answered exactly as FLT_MAX.
 *     box passes       !(fminf(c, m) <= max(tmin, t0x, t0y, t0z)).
 *     triangle accepted  !(|n.d| < 1e-8) && tmin <= t && t <= c && inside; c = t.
 *     visit order      left child, then right with the updated c; push right when both pass -- as srt_trace_rays.  A tree whose root is a
 *                      leaf tests that triangle with the same interval.
 *     closest query    runs to the end: with [0, FLT_MAX] (or [0, +inf]) its answer is srt_trace_rays' word for word.
 *     any query        stops after the first traversal step that accepted a triangle.  Up to that step it made the closest query's visits,
 *                      so occluded == (the closest query's tri >= 0) for every ray and every interval.
 *     special inputs   a direction with a NaN component is a miss (as srt_trace_rays); a NaN tmin or tmax, or tmin > tmax, accepts
 *                      nothing: a miss.  A negative tmin lets the query accept crossings behind the origin.
 *   A ray's answer depends on the ray and the tree alone, never on the order in which the kernel's lanes and waves take the rays.
 *   srt_intersect_rays      host arrays; hits[n][4] in srt_trace_rays' layout: t (0 on a miss), tri or -1, front_face, mat_index.
 *   srt_occluded_rays       host arrays; occluded[n] = 1 when the interval holds a hit, else 0.  Both host entries copy through a staging
 *                           block of the context on the NULL stream and synchronise.
 *   srt_intersect_rays_dev / srt_occluded_rays_dev  device pointers and a hipStream_t passed as void* (NULL = the NULL stream), under the
 *                           order of a context's calls (srt_render_chunk): the counter reset and the kernel are enqueued on that stream,
 *                           nothing synchronises.  rays_dev must stay valid and unchanged, and the answers are complete, once that stream
 *                           reaches them.
 *   Refused with SRT_ERR_INVALID, nothing enqueued or written: a null ctx, no scene uploaded (srt_set_test_knobs ends an upload too), a null
 *   rays or output pointer with n > 0, a device rays / hits pointer that is not 16-byte aligned, n > SRT_QUERY_MAX_RAYS (the kernel's
 *   32-bit ray counter).  n = 0 succeeds and touches nothing.  A failed allocation: SRT_ERR_HIP.  After srt_refit_vertices* the queries see
 *   the refitted images.
 *   srt_query_last          the last query launch of the context: kernel-only ms from HIP events (waits for that kernel alone), the
 *                           persistent waves launched, the inner records cached in LDS, the variant (narrow_refs, all_cached, paired) and
 *                           whether it was the any query.  SRT_ERR_INVALID before one ran.
 *   srt_set_query_test_grid TEST HOOK (tests and tools only, like srt_set_test_knobs): at most max_waves persistent waves per launch (whole
 *                           workgroups of at most the plan's size); 0 = fill the device (the default). */
#define SRT_QUERY_MAX_RAYS 0x7fffffffu
typedef struct srt_query_info { float ms; uint32_t waves, n_cached, narrow_refs, all_cached, paired, any, reserved; } srt_query_info;
SRT_API int srt_intersect_rays(srt_ctx *ctx, const float *rays, size_t n, float *hits);
SRT_API int srt_occluded_rays(srt_ctx *ctx, const float *rays, size_t n, uint8_t *occluded);
SRT_API int srt_intersect_rays_dev(srt_ctx *ctx, const float *rays_dev, size_t n, float *hits_dev, void *query_stream);
SRT_API int srt_occluded_rays_dev(srt_ctx *ctx, const float *rays_dev, size_t n, uint8_t *occluded_dev, void *query_stream);
SRT_API int srt_query_last(srt_ctx *ctx, srt_query_info *info);
SRT_API int srt_set_query_test_grid(srt_ctx *ctx, uint32_t max_waves);
/* Direct lighting (no reference counterpart: material::scatter has no next-event estimation): a deferred pass over a rectangle of the
 * image, built from a light sampler and the ray queries above (srt_light.hip).  Per sample: camera ray -> closest hit -> one shadow
 * segment to a sampled light and one cosine-distributed sky ray -> any-hit occlusion -> a sum.  In expectation the picture is what the
 * path tracer computes at bounce_limit = 2 on pixels whose first hit is not specular.  render_kernel is not involved.
 *
 *   Spectra collapse on the host.  A two-segment path camera -> Lambertian ms -> end e contributes, in expectation, the integral over
 *   [360, 830] nm of cmf(l) rho_ms(l) L_e(l), all three linear interpolants on the 5 nm grid (srt_color_tables' cmf rows x, y, z; the
 *   materials' spectral_distribution and the background as uploaded, a bake included; emission_power is not read).  Per 5 nm cell
 *   [a, b] Simpson's rule, exact for the cubic: 5/6 (f(a) + 4 f(m) + f(b)), f(m) the product of the factors' means (p(a) + p(b)) / 2;
 *   cells added in ascending order, all in double, the result rounded to float32 once.  At the first use after srt_upload_scene (the
 *   upload itself enqueues nothing and allocates nothing on the device for this):
 *     T_light[ms][ml][3]  surface material x emissive material    T_sky[ms][3]  surface material x background
 *     T_emit[m][3]        a material alone                         T_bg[3]       the background alone
 *   (on the device T_light is stored per emissive material that owns a light: its "slot").  The device part carries XYZ triples only.
 *
 *   Light table.  Every triangle, in scene order, with an EMISSIVE material, area > 0 and T_emit[mat].y > 0; both faces emit.  e1 = v1 - v0,
 *   e2 = v2 - v0 in float32; area = float32(0.5 sqrt(cx^2 + cy^2 + cz^2)), c = e1 x e2, evaluated in double from the float32 edges; n_l
 *   the triangle's unit normal of srt_scene_get_tri_records.  Weight g_l = double(area) x double(T_emit.y).  Integer thresholds
 *   c_0 = 0 <= ... <= c_L = N = 2^24 by largest remainder with every light at least 1 wide: start with all lights "free" and repeat
 *   { G = sum of g over the free lights in table order; B = N - (number of pinned lights); a free light with g / G * B < 1 becomes
 *   pinned (width 1) } until no light changes; a free light's width is floor(g / G * B), and the B - sum of these that remain go, one
 *   each, to the free lights with the largest remainders g / G * B - floor(.), ties to the lower index.  A 24-bit draw k picks the
 *   light with c_l <= k < c_l+1 (binary search: a = 0, b = L; while b - a > 1 { m = (a + b) >> 1; c_m <= k ? a = m : b = m }); its
 *   probability is exactly p_l = (c_l+1 - c_l) 2^-24, float32 exactly.  More than 2^20 lights: SRT_ERR_UNSUPPORTED.
 *
 *   Random numbers.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC11): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments
 *   0x9E3779B9, 0xBB67AE85; ten rounds of (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the
 *   key incremented between rounds.  The all-zero counter and key give 6627e8d5 e169c58d bc57ac4c 9b00dbd8.  Key = (seed low word,
 *   seed high word); counter = (pixel = global y * image width + global x, first_sample + s, purpose, try).  A sample's numbers depend
 *   on these and on nothing else: not on lane, wave, rectangle, round or which parts are on.  u(x) = (x >> 8) 2^-24; s(x) = 2 u(x) - 1.
 *   Purposes: 0 pixel jitter (try 0; words 0, 1), 1 lens disk (try t; words 0, 1), 2 light (try 0; word 0 >> 8 is the draw k, words 1,
 *   2 the point), 3 sky sphere (try t; words 0, 1, 2).
 *
 *   One sample, float32 throughout: + - x / sqrtf, conversions, compares, selects and integer operations only, not contracted, left to
 *   right; vectors componentwise; a . b = (a.x b.x + a.y b.y) + a.z b.z.
 *     Camera ray (renderer::get_ray as render_kernel states it).  px = -0.5 + u, py = -0.5 + u: jitter in [-0.5, 0.5)^2;
 *       pc = (pixel00_loc + float(X) pixel_delta_u) + float(Y) pixel_delta_v; ps = pc + (px pixel_delta_u + py pixel_delta_v); origin =
 *       camera_center, or when !(defocus_angle <= 0): (camera_center + dx defocus_disk_u) + dy defocus_disk_v with (dx, dy) = (s, s) of
 *       the first try t < 16 with dx dx + dy dy < 1, and (0, 0) when all 16 fail (probability (1 - pi/4)^16 = 2.0e-11: a bias bound,
 *       not tested).  Row (origin, 0, ps - origin, FLT_MAX).
 *     Closest hit: srt_intersect_rays_dev's kernel on the camera rows.
 *       miss                                      add T_bg (part EMITTED)
 *       EMISSIVE first hit                        add T_emit[mat] (part EMITTED)
 *       METALLIC or DIELECTRIC first hit          nothing; the sample counts as specular
 *       every other material type                 p = o + t d; n = the triangle's unit normal n_g (the shading record's) when d . n_g < 0,
 *                                                 else -n_g; o' = p + 0.0001 n (kEpsilon); then
 *         LIGHTS (the table is not empty)  pick l; (u1, u2) = (u, u); if u1 + u2 > 1: u1 = 1 - u1, u2 = 1 - u2; q = (v0 + u1 e1) + u2 e2;
 *                    dl = q - o'; nd = n . dl; r2 = dl . dl; cl = |n_l . dl|; the row is (o', 0, dl, 1 - 2^-10) and
 *                    w = ((nd cl) / ((r2 r2) pi)) (area / p_l), pi = 0x40490fdb, when nd > 0 and r2 > 0; else it is not traced and
 *                    w = 0.  Unoccluded: add w T_light[ms][ml].
 *         SKY        (x, y, z) = (s, s, s) of the first try t < 32 with 0 < len2 = (x x + y y) + z z < 1; v = (1 / sqrtf(len2)) (x, y,
 *                    z); when all 32 fail v = n (probability (1 - pi/6)^32 = 5.0e-11: a bias bound, not tested; 16 tries would leave
 *                    7.0e-6).  dir = n + v, and dir = n when all three |components| < 1e-8 (lambertian_scatter).  Row (o', 0, dir,
 *                    FLT_MAX).  Unoccluded: add T_sky[ms].
 *     A row that is not traced is written (.., tmin = 1, .., tmax = 0): the query answers it as a miss without a walk, and its
 *     contribution is masked.  Occlusion: srt_occluded_rays_dev's kernel on each buffer of shadow rows.
 *     Per pixel, samples in ascending order: with e, l, k the EMITTED, LIGHTS and SKY terms (0 where they do not apply),
 *     sum[c] = ((sum[c] + e[c]) + l[c]) + k[c]; t[c] = (e[c] + l[c]) + k[c]; m2[c] = m2[c] + t[c] t[c].  sum and m2 are SUMS over the
 *     call's samples, like the accumulation's.
 *   Rounds.  The work runs in rounds of a whole number of samples of the whole rectangle, sized so that the context's working buffers
 *   (130 bytes per row) stay under 320 MiB, one sample at least; sums carry over in sample order, so no answer depends on the round size.
 *
 *   srt_direct_light         on the context's camera and uploaded scene, any rectangle inside the camera's image, any partition; a query
 *                            like srt_surface_motion: NULL stream, synchronises, and only reads -- no frame, sum, history or RNG state moves.
 *                            out_sum[h][w][3], out_m2[h][w][3] (or NULL) row-major; result: the counters over all samples (light_rows and
 *                            sky_rows count traced rows) and the lights in the table.
 *   srt_direct_light_kat     the same for cfg->samples = 1 (one round of the sample index first_sample); also copies out, each when not
 *                            NULL and n = w h: cam_rows[n][8], hit_rows[n][4], light_rows[n][8], sky_rows[n][8] (zero when the part is
 *                            off), records[n][4] = bits(w), surface material (the first hit's), light index, kind (0 miss, 1 emitted,
 *                            2 specular, 3 shaded) | 4 light row traced | 8 sky row traced, and occ_light[n], occ_sky[n].
 *   srt_read_light_table     *n_lights; thresholds[L + 1] and records[L][16] = v0 area | e1 bits(mat) | e2 bits(tri) | n_l bits(slot)
 *                            when not NULL and cap >= L (else SRT_ERR_INVALID).  Host only once the table exists.
 *   srt_direct_light_last    kernel-only ms of the last call, summed over its rounds: camera, shade, gather kernels, the query launches;
 *                            and its rounds.
 *   srt_set_light_test_batch TEST HOOK: rounds of at most max_rows rows (one sample at least); 0 = the budget.
 *   Refused, nothing changed or written: SRT_ERR_INVALID for a null argument, no scene or no camera, samples outside 1 .. 65536, parts 0
 *   or with unknown bits, first_sample + samples > 2^32, an empty rectangle, one that sticks out of the camera's image or has more than
 *   2^28 pixels, (kat) samples != 1; SRT_ERR_UNSUPPORTED for more than 2^20 lights, and for LIGHTS on a context whose scene was refitted
 *   since its upload (the table's areas are stale; EMITTED and SKY work on refitted trees). */
#define SRT_LIGHT_EMITTED 1u
#define SRT_LIGHT_LIGHTS 2u
#define SRT_LIGHT_SKY 4u
#define SRT_LIGHT_MAX_SAMPLES 65536u
#define SRT_LIGHT_MAX_LIGHTS (1u << 20)
typedef struct srt_light { uint32_t samples, first_sample, parts, reserved; uint64_t seed; } srt_light;
typedef struct srt_light_result {
    uint64_t miss, emitted, specular, shaded, light_rows, light_unoccluded, sky_rows, sky_unoccluded;
    uint32_t lights, reserved;
} srt_light_result;
typedef struct srt_light_info { float camera_ms, shade_ms, gather_ms, query_ms; uint32_t rounds, rows_per_round, query_launches, reserved; } srt_light_info;
SRT_API int srt_direct_light(srt_ctx *ctx, const srt_light *cfg, float *out_sum, float *out_m2, srt_light_result *result,
                             uint32_t w, uint32_t h, uint32_t ox, uint32_t oy);
SRT_API int srt_direct_light_kat(srt_ctx *ctx, const srt_light *cfg, float *out_sum, float *out_m2, srt_light_result *result,
                                 uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, float *cam_rows, float *hit_rows, float *light_rows,
                                 float *sky_rows, uint32_t *records, uint8_t *occ_light, uint8_t *occ_sky);
SRT_API int srt_read_light_table(srt_ctx *ctx, uint32_t *n_lights, uint32_t *thresholds, float *records, size_t cap);
SRT_API int srt_direct_light_last(srt_ctx *ctx, srt_light_info *info);
SRT_API int srt_set_light_test_batch(srt_ctx *ctx, uint32_t max_rows);
/* Device arithmetic self-test: evaluates op `which` on n operand pairs on the GPU (see DESIGN.md "primitive-op
 * sweep"); used to prove the device's + - * / sqrt fmin cast and srt_powf bits equal the host's. */
SRT_API int srt_device_op_sweep(srt_ctx *ctx, int which, const float *a, const float *b, size_t n, float *out);
/* The tile scheduler on explicit costs -- KAT entry point (no reference counterpart: the pixel queue is scheduling only).  Runs the
 * kernel that builds a launch's pixel queue on cost[2 * n] (per-tile cost, then the cost of each tile's most expensive pixel) for a
 * machine of n_waves waves, in buffers of its own: the context's schedule is not touched.  rows_out receives rows_cap words of a row
 * buffer that held 0xffffffff in every word before the kernel ran (row = local tile | part << 22 | level << 28), sorted_out the n
 * tile numbers in queue order, info_out 4 words: [0] the number of rows, [1] the largest tile cost.  SRT_ERR_INVALID, with nothing
 * enqueued, for n == 0, n > 2^20 (beyond that the scheduler never splits; left out here) and rows_cap < 64 * n + 64 (the largest
 * possible queue and 64 guard words behind it). */
SRT_API int srt_order_tiles_kat(srt_ctx *ctx, const uint32_t *cost, uint32_t n, uint32_t n_waves, uint32_t split_load_pct,
                                uint32_t order_max_pct, uint32_t *rows_out, size_t rows_cap, uint32_t *sorted_out, uint32_t *info_out);
/* What the host knew when the cost probe built the context's current schedule (srt_read_tile_schedule). */
typedef struct srt_tile_schedule_info {
    uint32_t tiles_local;         /* local tiles the probe measured */
    uint32_t n_rows;              /* rows of the queue that was read (filled in from the device) */
    uint32_t cost_max;            /* the largest tile cost, as the render kernel's wave priorities see it (from the device) */
    uint32_t n_waves_plan;        /* waves of the machine the split policy planned for (a streamed pass: divided by its streams) */
    uint32_t split_load_pct;      /* as passed to the scheduler: 0 when the launch may not split */
    uint32_t order_max_pct;       /* as passed to the scheduler */
    uint32_t streams;             /* RNG streams per pixel of the pass that ran the probe (1 unless streamed) */
    uint32_t reserved;
} srt_tile_schedule_info;
/* The pixel queue a launch ran -- tests and diagnostics, like srt_get_tile_costs; synchronises.  which = 0: the queue the cost probe
 * built for the last launch (or for the accumulation that launch belongs to); which = 1: the compacted queue the last adaptive pass
 * left for the next one.  Copies info->n_rows rows to rows_out.  SRT_ERR_INVALID when the last launch has no such queue or rows_cap
 * is smaller than its row count. */
SRT_API int srt_read_tile_schedule(srt_ctx *ctx, int which, uint32_t *rows_out, size_t rows_cap, srt_tile_schedule_info *info);

SRT_API int srt_ctx_device(const srt_ctx *ctx);                 /* HIP device index of the context */
/* compute units of the context's GPU (a render launch keeps srt_launch_plan's waves_per_cu x 64 pixels in flight on each) */
SRT_API int srt_ctx_cu_count(const srt_ctx *ctx);

/* ---------------------------------------------------------------------------------------------------
 * Multi-GPU.  The reference's caller renders chunk after chunk on ONE GPU
 * (render_manager::step, rendering/render_manager.cu:3-66); a communicator fans one chunk out over W GPUs:
 * rank r renders the 8x8-pixel tiles t with t % W == r, ONE RCCL gather (xGMI inside a node) brings the
 * compact tile buffers to rank 0, which scatters them into its block-linear framebuffer.  The image is
 * bit-identical for every W (per-pixel seeds, rendering.cu:137).  RCCL is loaded (dlopen) on first use.
 * ------------------------------------------------------------------------------------------------- */
#define SRT_COMM_ID_BYTES 128
typedef struct srt_comm srt_comm;
/* One process drives n GPUs: creates one context per device (rank i = devices[i]) and an RCCL communicator
 * over them (ncclCommInitAll), one HIP stream per device. */
SRT_API int srt_comm_init_all(const int *devices, int n, srt_comm **out);
/* One process per GPU (torch.distributed.run, mpirun): rank 0 calls srt_comm_unique_id and hands the 128 bytes
 * to the other ranks by any channel; every rank then wraps its own context.  Sets the context's partition. */
SRT_API int srt_comm_unique_id(unsigned char id[SRT_COMM_ID_BYTES]);
SRT_API int srt_comm_init_rank(srt_ctx *ctx, const unsigned char id[SRT_COMM_ID_BYTES], uint32_t rank, uint32_t world, srt_comm **out);
/* SRT_OK when an RCCL can be loaded in this process, SRT_ERR_UNSUPPORTED (with a message) otherwise.  Cheap and local: a
 * launcher lets every rank call it and agrees on the exchange path BEFORE any rank enters the collective srt_comm_init_rank.
 * An RCCL the host process already mapped (PyTorch's) is re-used; SRT_RCCL_LIB names an explicit library. */
SRT_API int srt_comm_available(void);
/* Planes the gather moves: 3 (default) = the quantised framebuffer, 12 B / pixel; 9 = + the parity planes (72 B / pixel).
 * With one process per GPU EVERY rank must set the same value: every srt_render_frame_multi of such a communicator starts with a
 * 4-byte all-gather of the count each rank's context will really use (whichever call set it, srt_set_gather_planes on the wrapped
 * context included) and fails with SRT_ERR_INVALID on EVERY rank when they differ -- all ranks make the same collective calls, so a
 * disagreement is an error, never a hang in ncclGather.  After a 3-plane frame rank 0's parity planes are not this frame's: srt_read_fb_aux returns
 * SRT_ERR_UNSUPPORTED until a 9-plane frame (or a single-GPU scatter) has written them. */
SRT_API int srt_comm_set_gather_planes(srt_comm *comm, uint32_t planes);
SRT_API void srt_comm_destroy(srt_comm *comm);                 /* destroys the contexts srt_comm_init_all created */
SRT_API const char *srt_comm_last_error(const srt_comm *comm);
SRT_API uint32_t srt_comm_world(const srt_comm *comm);
SRT_API uint32_t srt_comm_local_count(const srt_comm *comm);   /* contexts this process drives */
SRT_API srt_ctx *srt_comm_ctx(srt_comm *comm, uint32_t local_index);
SRT_API srt_ctx *srt_comm_root_ctx(srt_comm *comm);            /* rank 0's context (holds the assembled framebuffer) or NULL */
/* srt_upload_scene / srt_set_camera / srt_init_device_params on every local context (the scene is replicated). */
SRT_API int srt_comm_upload_scene(srt_comm *comm, const srt_scene *s);
SRT_API int srt_comm_set_camera(srt_comm *comm, const srt_camera_data *cam);
/* srt_refit_vertices on every local context, as srt_comm_upload_scene uploads to them. */
SRT_API int srt_comm_refit_vertices(srt_comm *comm, const float *verts_host, size_t n_tris);
SRT_API int srt_comm_init_device_params(srt_comm *comm, uint32_t tx, uint32_t ty, uint32_t bx, uint32_t by, uint32_t chunk_w,
                                        uint32_t chunk_h, uint32_t spp, uint32_t bounce_limit, uint64_t seed);
/* renderer::render(w,h,offx,offy) on W GPUs: render kernels on every local rank's stream, one ncclGather of the tile
 * buffers to rank 0, one scatter kernel there.  Asynchronous; srt_comm_synchronize waits for the local streams.
 * Afterwards rank 0's context answers srt_read_fb / srt_read_fb_rowmajor / srt_dev_fb as after srt_render_chunk. */
SRT_API int srt_render_frame_multi(srt_comm *comm, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy);
/* Progressive rendering on W GPUs: srt_accum_reset on every local context; then srt_render_frame_multi with an accumulating pass
 * (srt_render_chunk_accum, spp_add samples) on every rank's own tiles.  The gather moves the tile buffers exactly as for a plain frame. */
SRT_API int srt_comm_accum_reset(srt_comm *comm);
SRT_API int srt_render_frame_multi_accum(srt_comm *comm, uint32_t width, uint32_t height, uint32_t offx, uint32_t offy, uint32_t spp_add);
/* Adaptive sampling on W GPUs: srt_accum_reset_adaptive on every local context (then srt_render_frame_multi_accum as above), and the
 * active pixels summed over the local contexts.  A process-per-GPU communicator (srt_comm_init_rank) returns SRT_ERR_UNSUPPORTED: a
 * stop decision there would need a reduction across processes. */
SRT_API int srt_comm_accum_reset_adaptive(srt_comm *comm, const srt_adaptive *cfg);
SRT_API int srt_comm_accum_active(srt_comm *comm, uint64_t *active);
/* Spectral film on W GPUs: srt_accum_reset_spectral on every local context; srt_render_frame_multi_accum then runs MODE 5 on each rank.
 * The films stay with their ranks (srt_read_spectral per context; each pixel is owned by one rank and reads +0 on the others) until
 * srt_comm_gather_accum(comm, SRT_GATHER_FILM | ..) brings them to rank 0. */
SRT_API int srt_comm_accum_reset_spectral(srt_comm *comm);
/* First-hit features on W GPUs: srt_accum_reset_features on every local context; srt_render_frame_multi_accum then runs MODE 7 on each
 * rank.  The rows stay with their ranks (srt_read_features per context; each pixel is owned by one rank and reads +0 on the others) until
 * srt_comm_gather_accum brings them to rank 0.  On process-per-GPU communicators too: no decision crosses ranks. */
SRT_API int srt_comm_accum_reset_features(srt_comm *comm);
/* srt_accum_reset_adaptive_features on every local rank; like srt_comm_accum_reset_adaptive, SRT_ERR_UNSUPPORTED on a process-per-GPU
 * communicator.  The rows stay with their ranks until srt_comm_gather_accum, as for srt_comm_accum_reset_features. */
SRT_API int srt_comm_accum_reset_adaptive_features(srt_comm *comm, const srt_adaptive *cfg);
/* srt_accum_reset_spectral_features on every local rank (any communicator: no decision crosses ranks); film and rows stay with their
 * ranks, as for srt_comm_accum_reset_spectral and srt_comm_accum_reset_features.  A denoise of the whole frame: srt_comm_gather_accum, then the
 * stage on srt_comm_root_ctx. */
SRT_API int srt_comm_accum_reset_spectral_features(srt_comm *comm);
/* srt_accum_reset_adaptive_spectral / _features on every local rank; like srt_comm_accum_reset_adaptive, SRT_ERR_UNSUPPORTED on a
 * process-per-GPU communicator.  Film and rows stay with their ranks until srt_comm_gather_accum; srt_comm_accum_active sums the active pixels. */
SRT_API int srt_comm_accum_reset_adaptive_spectral(srt_comm *comm, const srt_adaptive *cfg);
SRT_API int srt_comm_accum_reset_adaptive_spectral_features(srt_comm *comm, const srt_adaptive *cfg);
/* Sample-parallel pixels on W GPUs: srt_accum_reset_streams on every local context; srt_render_frame_multi_accum then runs MODE 6 on each
 * rank.  On process-per-GPU communicators too: no decision crosses ranks (every rank resets with the same K). */
SRT_API int srt_comm_accum_reset_streams(srt_comm *comm, uint32_t streams);
SRT_API int srt_comm_synchronize(srt_comm *comm);
/* Closest-hit queries / paths of the last frame summed over the local ranks, and the slowest local render kernel. */
SRT_API int srt_comm_stats(srt_comm *comm, uint64_t *rays, uint64_t *paths, float *max_kernel_ms);
/* Time between the end of a local rank's render kernel and the end of the exchange of the last frame (gather + waiting for
 * the slowest rank + the scatter on rank 0), max over the local ranks, ms; 0 in a 1-rank world. */
SRT_API int srt_comm_last_gather_ms(srt_comm *comm, float *ms);
/* The accumulations of the ranks gathered on rank 0 (srt_pack_accum on every local rank's stream, ONE ncclGather of the units into a
 * buffer of their own, srt_unpack_accum on rank 0): afterwards srt_comm_root_ctx is whole for every stage that reads `parts` -- the
 * denoisers, the temporal stage, srt_present_* -- and computes what a single context would compute, bit for bit.  parts: SRT_GATHER_*
 * as for srt_pack_accum (0: everything the kind holds except the film).  Asynchronous like srt_render_frame_multi, and to be repeated
 * after every further pass: callers gather before they look.  With world == 1 it succeeds and does nothing.
 * Before anything is enqueued the ranks must agree on kind, sample total, streams, chunk and offset, and parts (srt_comm_init_all
 * compares its contexts; srt_comm_init_rank all-gathers a 32-byte descriptor, the same collective on every rank): a mismatch -- or a
 * rank whose context would refuse the pack -- returns SRT_ERR_INVALID on EVERY rank, and no rank enters the gather alone. */
SRT_API int srt_comm_gather_accum(srt_comm *comm, uint32_t parts);
/* Of the last srt_comm_gather_accum, ms: the slowest local pack kernel, the exchange (end of a local pack to the end of the gather,
 * waiting for the slowest rank included; max over the local ranks) and rank 0's unpack kernel (0 where rank 0 is not local).
 * All 0 in a 1-rank world. */
SRT_API int srt_comm_last_accum_gather_ms(srt_comm *comm, float *pack_ms, float *exchange_ms, float *unpack_ms);

/* Issue-rate calibration (no reference counterpart: measurement support for bench.py's roofline).  Runs microkernel
 * `kind` (csrc/srt_calib.hip: 0 v_add_f32, 1 v_pk_mul_f32, 2 v_fma_f32, 3 dependent v_add_f32 chain, 4 s_add_u32,
 * 5 v_add_f32 + s_add_u32 interleaved, 6 v_cmp + v_cndmask, 7 / 8 ds_read_b64 linear / random, 9 v_max3_f32,
 * 10 v_add_f32 with 26 of 64 lanes enabled) with one workgroup of waves_per_simd * 256 threads on every CU. */
typedef struct {
    double wave_cycles_mean, wave_cycles_max;   /* s_memtime ticks (shader cycles) a wave spent in its loop */
    double wall_ms;                             /* HIP events around the launch */
    uint64_t instr_per_wave;                    /* instructions of the measured loop body per wave (loop control excluded) */
    uint32_t n_waves, n_cu, waves_per_simd;
    uint32_t reserved;
    double wave_cycles_min;                     /* the SIMD arbitrates by age: with 4 resident waves the oldest finish first, so the
                                                   rate of a SIMD is instructions / wave_cycles_max (or wall x clock), never / mean */
} srt_calibration;
SRT_API int srt_calibrate(srt_ctx *ctx, int kind, uint32_t waves_per_simd, uint32_t iters, srt_calibration *out);

#ifdef __cplusplus
}
#endif
#endif /* SRT_C_API_H */
