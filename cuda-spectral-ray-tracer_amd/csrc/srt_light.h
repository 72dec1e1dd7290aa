// srt_light.h -- the deferred direct-light pass (srt_light.hip; stated operation by operation in srt_c_api.h at "Direct lighting").
// A header of its own, so that no other translation unit sees a change: only srt_light.hip and srt_capi.cpp include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srt {

constexpr uint32_t kLightDiskTries = 16;        // unit-disk rejection: (1 - pi/4)^16 = 2.0e-11
constexpr uint32_t kLightSphereTries = 32;      // unit-sphere rejection: (1 - pi/6)^32 = 5.0e-11 (16 tries would leave 7.0e-6)
constexpr uint32_t kLightCounters = 8;          // miss, emitted, specular, shaded, light_rows, light_unoccluded, sky_rows, sky_unoccluded
// the record's kind word
constexpr uint32_t kLightKindMiss = 0, kLightKindEmitted = 1, kLightKindSpecular = 2, kLightKindShaded = 3;
constexpr uint32_t kLightKindMask = 3u, kLightRowLight = 4u, kLightRowSky = 8u;

// One round: n_samples samples of every pixel of the w x h rectangle at (ox, oy) of an image image_w wide.  Row i = s * (w * h) + y * w + x
// belongs to sample first_sample + s of pixel (ox + x, oy + y).
struct LightRound {
    uint32_t w, h, ox, oy, image_w;
    uint32_t n_samples, first_sample;
    uint32_t seed_lo, seed_hi;
    uint32_t parts;                 // SRT_LIGHT_* bits
};

struct LightCamera { float du[3], dv[3], p00[3], center[3], disk_u[3], disk_v[3], defocus_angle; };

struct LightShadeParams {
    LightRound r;
    const float4 *cam_rows;         // [n][2]
    const float4 *hits;             // [n]: (t, tri or -1, front_face, mat), the closest query's rows
    const float4 *shade;            // the scene's shading records, 3 float4 per triangle
    uint32_t n_tris;
    const uint32_t *thresholds;     // [n_lights + 1]
    const float4 *lights;           // [n_lights][4]: (v0, area) (e1, bits(mat)) (e2, bits(tri)) (n, bits(slot))
    uint32_t n_lights;
    float4 *light_rows, *sky_rows;  // [n][2] each (null when the part is off)
    uint4 *records;                 // [n]: bits(w), surface material, light index, kind | row flags
};

struct LightGatherParams {
    LightRound r;
    const uint4 *records;
    const uint8_t *occ_light, *occ_sky;      // null when the part is off
    const float4 *lights;
    const float *t_light;           // [n_materials][n_slots][3]
    const float *t_sky;             // [n_materials][3]
    const float *t_emit;            // [n_materials][3]
    float t_bg[3];
    uint32_t n_materials, n_slots;
    float *sum, *m2;                // [h][w][3], read and written: the sums carry over the rounds of a call
    unsigned long long *counters;   // [kLightCounters]
};

hipError_t launch_light_camera(const LightRound &r, const LightCamera &cam, float4 *cam_rows, hipStream_t st);
hipError_t launch_light_shade(const LightShadeParams &p, hipStream_t st);
hipError_t launch_light_gather(const LightGatherParams &p, hipStream_t st);

}  // namespace srt
