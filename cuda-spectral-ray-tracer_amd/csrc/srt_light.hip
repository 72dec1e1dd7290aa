// srt_light.hip -- the deferred direct-light pass: camera rows, shade rows and the gather around the two query launches of srt_query.hip
// (srt_direct_light, srt_direct_light_kat; include/srt_c_api.h states every operation at "Direct lighting", tests/direct_light_reference.py
// restates them in numpy float32).
//
// A translation unit of its own, like the ray queries': no render, denoise, develop, expose, present, despeckle, temporal, refit, motion or
// query kernel is touched and their machine code stays what it was.  Built with the exactness flags of the other units (-ffp-contract=off,
// no fast-math, correctly rounded division and square root): every product, quotient and root below is rounded once, in the order written.
//
// Three streaming kernels, one lane per row (camera, shade) or per pixel (gather), 256 lanes per workgroup:
//   light_camera_kernel   row i = sample s of pixel (x, y): the camera ray (o, 0) (d, FLT_MAX), two 16-byte stores.
//   light_shade_kernel    reads the camera row and the closest query's hit row, writes the light's and the sky's shadow rows (two 16-byte
//                         stores each; a row that must not be traced has tmin = 1 > tmax = 0) and the 16-byte record.
//   light_gather_kernel   one lane per pixel walks the round's samples in order and adds into sum / m2, which carry over the rounds of a
//                         call, so the sums do not depend on the round size.  The integer counters are summed over a wave, then over the
//                         workgroup in LDS, then one atomic per workgroup and non-zero counter.
// Random numbers: Philox4x32-10 on the counter (pixel, sample, purpose, try) under the key (seed): no state, no dependence on lane or round.
// No scratch, no float atomics, no inline assembly, no LDS beyond the counters.
#include "srt_light.h"

#include "../../include/srt_c_api.h"

namespace srt {

namespace {

constexpr uint32_t kLtThreads = 256;
constexpr float kLtFltMax = 3.402823466e+38f;
constexpr float kLtEpsilon = 0.0001f;            // kEpsilon of the render kernel (materials/material.cuh:14)
constexpr float kLtPi = 3.14159265358979f;       // 0x40490fdb
constexpr float kLtShadowEnd = 0.9990234375f;    // 1 - 2^-10

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 f3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ F3 ld3(const float *a) { return f3(a[0], a[1], a[2]); }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ F3 operator-(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ F3 operator*(float t, F3 v) { return f3(t * v.x, t * v.y, t * v.z); }
// (a.x * b.x + a.y * b.y) + a.z * b.z, as srt_c_api.h defines a dot product
__device__ __forceinline__ float dot3(F3 a, F3 b) { const float s = a.x * b.x + a.y * b.y; return s + a.z * b.z; }

struct U4 { uint32_t x, y, z, w; };
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11), restated in srt_c_api.h
__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    U4 o; o.x = c0; o.y = c1; o.z = c2; o.w = c3;
    return o;
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-08f; }      // (x >> 8) 2^-24: exact
__device__ __forceinline__ float pm1(uint32_t x) { return 2.0f * u01(x) - 1.0f; }                             // exact as well

// row i of a round -> sample offset and pixel; false beyond the round
__device__ __forceinline__ bool row_of(const LightRound &r, uint32_t &i, uint32_t &pid, uint32_t &si, uint32_t &gx, uint32_t &gy) {
    const uint32_t npix = r.w * r.h;
    i = blockIdx.x * kLtThreads + threadIdx.x;
    if (i >= npix * r.n_samples) return false;
    const uint32_t s = i / npix, pix = i - s * npix;
    const uint32_t y = pix / r.w, x = pix - y * r.w;
    gx = r.ox + x; gy = r.oy + y;
    pid = gy * r.image_w + gx;
    si = r.first_sample + s;
    return true;
}

__global__ __launch_bounds__(kLtThreads) void light_camera_kernel(const LightRound R, const LightCamera cam, float4 *__restrict__ rows) {
    uint32_t i, pid, si, gx, gy;
    if (!row_of(R, i, pid, si, gx, gy)) return;
    const U4 j = philox(pid, si, 0u, 0u, R.seed_lo, R.seed_hi);
    const float px = -0.5f + u01(j.x), py = -0.5f + u01(j.y);
    const F3 du = ld3(cam.du), dv = ld3(cam.dv), centre = ld3(cam.center);
    const F3 pixel_center = (ld3(cam.p00) + (float)gx * du) + (float)gy * dv;
    const F3 pixel_sample = pixel_center + (px * du + py * dv);
    F3 origin = centre;
    if (!(cam.defocus_angle <= 0.0f)) {
        float dx = 0.0f, dy = 0.0f;      // (the fallback after kLightDiskTries rejections: the lens centre)
        for (uint32_t t = 0; t < kLightDiskTries; t++) {
            const U4 q = philox(pid, si, 1u, t, R.seed_lo, R.seed_hi);
            const float a = pm1(q.x), b = pm1(q.y);
            if (a * a + b * b < 1.0f) { dx = a; dy = b; break; }
        }
        origin = (centre + dx * ld3(cam.disk_u)) + dy * ld3(cam.disk_v);
    }
    const F3 d = pixel_sample - origin;
    rows[2 * (size_t)i + 0] = make_float4(origin.x, origin.y, origin.z, 0.0f);
    rows[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, kLtFltMax);
}

__device__ __forceinline__ void put_row(float4 *rows, uint32_t i, F3 o, float tmin, F3 d, float tmax) {
    rows[2 * (size_t)i + 0] = make_float4(o.x, o.y, o.z, tmin);
    rows[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, tmax);
}

__global__ __launch_bounds__(kLtThreads) void light_shade_kernel(const LightShadeParams P) {
    uint32_t i, pid, si, gx, gy;
    if (!row_of(P.r, i, pid, si, gx, gy)) return;
    const float4 hit = P.hits[i];
    const int tri = (int)hit.y;
    uint32_t kind = kLightKindMiss, mat = 0u, light = 0u;
    float w = 0.0f;
    // the rows of a sample that traces nothing: an empty interval, which the query answers as a miss without a walk
    F3 lo = f3(0.f, 0.f, 0.f), ld = f3(0.f, 0.f, 1.f), so = lo, sd = ld;
    bool l_traced = false, s_traced = false;
    if (tri >= 0 && (uint32_t)tri < P.n_tris) {
        const float4 s0 = P.shade[3 * (size_t)tri + 0], s1 = P.shade[3 * (size_t)tri + 1];
        mat = __float_as_uint(s0.w);
        const uint32_t mtype = __float_as_uint(s1.x);
        if (mtype == (uint32_t)SRT_MAT_EMISSIVE) kind = kLightKindEmitted;
        else if (mtype == (uint32_t)SRT_MAT_METALLIC || mtype == (uint32_t)SRT_MAT_DIELECTRIC) kind = kLightKindSpecular;
        else {
            kind = kLightKindShaded;
            const float4 c0 = P.cam_rows[2 * (size_t)i + 0], c1 = P.cam_rows[2 * (size_t)i + 1];
            const F3 o = f3(c0.x, c0.y, c0.z), d = f3(c1.x, c1.y, c1.z);
            const F3 n_geo = f3(s0.x, s0.y, s0.z);
            const F3 p = o + hit.x * d;
            const bool front_face = dot3(d, n_geo) < 0.0f;
            const F3 n = front_face ? n_geo : f3(-n_geo.x, -n_geo.y, -n_geo.z);
            const F3 o2 = p + kLtEpsilon * n;
            lo = o2; so = o2;
            if ((P.r.parts & SRT_LIGHT_LIGHTS) && P.n_lights > 0u) {
                const U4 q = philox(pid, si, 2u, 0u, P.r.seed_lo, P.r.seed_hi);
                const uint32_t k = q.x >> 8;
                uint32_t a = 0u, b = P.n_lights;      // thresholds[a] <= k < thresholds[b]
                while (b - a > 1u) {
                    const uint32_t m = (a + b) >> 1;
                    if (P.thresholds[m] <= k) a = m; else b = m;
                }
                light = a;
                const float pl = (float)(P.thresholds[a + 1] - P.thresholds[a]) * 5.9604644775390625e-08f;
                const float4 l0 = P.lights[4 * (size_t)a + 0], l1 = P.lights[4 * (size_t)a + 1], l2 = P.lights[4 * (size_t)a + 2], l3 = P.lights[4 * (size_t)a + 3];
                float u1 = u01(q.y), u2 = u01(q.z);
                if (u1 + u2 > 1.0f) { u1 = 1.0f - u1; u2 = 1.0f - u2; }
                const F3 point = (f3(l0.x, l0.y, l0.z) + u1 * f3(l1.x, l1.y, l1.z)) + u2 * f3(l2.x, l2.y, l2.z);
                const F3 dl = point - o2;
                const float nd = dot3(n, dl), r2 = dot3(dl, dl);
                const float cl = fabsf(dot3(f3(l3.x, l3.y, l3.z), dl));
                ld = dl;
                if (nd > 0.0f && r2 > 0.0f) {
                    l_traced = true;
                    w = ((nd * cl) / ((r2 * r2) * kLtPi)) * (l0.w / pl);
                }
            }
            if (P.r.parts & SRT_LIGHT_SKY) {
                F3 ruv = n;      // (the fallback after kLightSphereTries rejections: the normal itself)
                for (uint32_t t = 0; t < kLightSphereTries; t++) {
                    const U4 q = philox(pid, si, 3u, t, P.r.seed_lo, P.r.seed_hi);
                    const float a = pm1(q.x), b = pm1(q.y), c = pm1(q.z);
                    const float len2 = (a * a + b * b) + c * c;
                    if (len2 < 1.0f && len2 > 0.0f) {
                        const float kk = 1.0f / sqrtf(len2);
                        ruv = kk * f3(a, b, c);
                        break;
                    }
                }
                F3 dir = n + ruv;
                if (fabsf(dir.x) < 1e-8f && fabsf(dir.y) < 1e-8f && fabsf(dir.z) < 1e-8f) dir = n;
                sd = dir;
                s_traced = true;
            }
        }
    }
    if (P.light_rows) put_row(P.light_rows, i, lo, l_traced ? 0.0f : 1.0f, ld, l_traced ? kLtShadowEnd : 0.0f);
    if (P.sky_rows) put_row(P.sky_rows, i, so, s_traced ? 0.0f : 1.0f, sd, s_traced ? kLtFltMax : 0.0f);
    P.records[i] = make_uint4(__float_as_uint(w), mat, light, kind | (l_traced ? kLightRowLight : 0u) | (s_traced ? kLightRowSky : 0u));
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kLtThreads) void light_gather_kernel(const LightGatherParams P) {
    __shared__ uint32_t wg_counts[kLightCounters];
    if (threadIdx.x < kLightCounters) wg_counts[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t npix = P.r.w * P.r.h;
    const uint32_t pix = blockIdx.x * kLtThreads + threadIdx.x;
    uint32_t n[kLightCounters] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (pix < npix) {
        float s0 = P.sum[3 * (size_t)pix + 0], s1 = P.sum[3 * (size_t)pix + 1], s2 = P.sum[3 * (size_t)pix + 2];
        float q0 = 0.f, q1 = 0.f, q2 = 0.f;
        if (P.m2) { q0 = P.m2[3 * (size_t)pix + 0]; q1 = P.m2[3 * (size_t)pix + 1]; q2 = P.m2[3 * (size_t)pix + 2]; }
        for (uint32_t s = 0; s < P.r.n_samples; s++) {
            const size_t i = (size_t)s * npix + pix;
            const uint4 rec = P.records[i];
            const uint32_t kind = rec.w & kLightKindMask;
            float e0 = 0.f, e1 = 0.f, e2 = 0.f, l0 = 0.f, l1 = 0.f, l2 = 0.f, k0 = 0.f, k1 = 0.f, k2 = 0.f;
            const bool mat_ok = rec.y < P.n_materials;
            if (kind == kLightKindMiss) {
                n[0]++;
                if (P.r.parts & SRT_LIGHT_EMITTED) { e0 = P.t_bg[0]; e1 = P.t_bg[1]; e2 = P.t_bg[2]; }
            } else if (kind == kLightKindEmitted) {
                n[1]++;
                if ((P.r.parts & SRT_LIGHT_EMITTED) && mat_ok) { const float *t = P.t_emit + 3 * (size_t)rec.y; e0 = t[0]; e1 = t[1]; e2 = t[2]; }
            } else if (kind == kLightKindSpecular) {
                n[2]++;
            } else {
                n[3]++;
                if (rec.w & kLightRowLight) {
                    n[4]++;
                    if (P.occ_light[i] == 0) {
                        n[5]++;
                        if (mat_ok) {
                            const uint32_t slot = __float_as_uint(P.lights[4 * (size_t)rec.z + 3].w);
                            const float *t = P.t_light + 3 * ((size_t)rec.y * P.n_slots + slot);
                            const float w = __uint_as_float(rec.x);
                            l0 = w * t[0]; l1 = w * t[1]; l2 = w * t[2];
                        }
                    }
                }
                if (rec.w & kLightRowSky) {
                    n[6]++;
                    if (P.occ_sky[i] == 0) {
                        n[7]++;
                        if (mat_ok) { const float *t = P.t_sky + 3 * (size_t)rec.y; k0 = t[0]; k1 = t[1]; k2 = t[2]; }
                    }
                }
            }
            // sum: EMITTED, then LIGHTS, then SKY; m2: the square of the sample's total (e + l) + k
            s0 = ((s0 + e0) + l0) + k0; s1 = ((s1 + e1) + l1) + k1; s2 = ((s2 + e2) + l2) + k2;
            const float c0 = (e0 + l0) + k0, c1 = (e1 + l1) + k1, c2 = (e2 + l2) + k2;
            q0 = q0 + c0 * c0; q1 = q1 + c1 * c1; q2 = q2 + c2 * c2;
        }
        P.sum[3 * (size_t)pix + 0] = s0; P.sum[3 * (size_t)pix + 1] = s1; P.sum[3 * (size_t)pix + 2] = s2;
        if (P.m2) { P.m2[3 * (size_t)pix + 0] = q0; P.m2[3 * (size_t)pix + 1] = q1; P.m2[3 * (size_t)pix + 2] = q2; }
    }
    // every lane of the workgroup arrives here
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t k = 0; k < kLightCounters; k++) {
        const uint32_t s = wave_sum_u32(n[k]);
        if (lane == 0u && s) atomicAdd(&wg_counts[k], s);
    }
    __syncthreads();
    if (threadIdx.x < kLightCounters && wg_counts[threadIdx.x]) atomicAdd(&P.counters[threadIdx.x], (unsigned long long)wg_counts[threadIdx.x]);
}

bool round_ok(const LightRound &r, uint64_t &rows) {
    if (r.w == 0 || r.h == 0 || r.n_samples == 0) return false;
    rows = (uint64_t)r.w * r.h * r.n_samples;
    return (uint64_t)r.w * r.h <= 0x7fffffffull && rows <= (uint64_t)SRT_QUERY_MAX_RAYS;
}

}  // namespace

hipError_t launch_light_camera(const LightRound &r, const LightCamera &cam, float4 *cam_rows, hipStream_t st) {
    uint64_t rows;
    if (!round_ok(r, rows) || !cam_rows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(light_camera_kernel, dim3((uint32_t)((rows + kLtThreads - 1) / kLtThreads)), dim3(kLtThreads), 0, st, r, cam, cam_rows);
    return hipGetLastError();
}

hipError_t launch_light_shade(const LightShadeParams &p, hipStream_t st) {
    uint64_t rows;
    if (!round_ok(p.r, rows) || !p.cam_rows || !p.hits || !p.shade || !p.records) return hipErrorInvalidValue;
    if (p.n_lights > 0 && (!p.thresholds || !p.lights)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(light_shade_kernel, dim3((uint32_t)((rows + kLtThreads - 1) / kLtThreads)), dim3(kLtThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_light_gather(const LightGatherParams &p, hipStream_t st) {
    uint64_t rows;
    if (!round_ok(p.r, rows) || !p.records || !p.sum || !p.counters || !p.t_sky || !p.t_emit) return hipErrorInvalidValue;
    if (p.n_slots > 0 && (!p.t_light || !p.lights)) return hipErrorInvalidValue;
    const uint64_t npix = (uint64_t)p.r.w * p.r.h;
    hipLaunchKernelGGL(light_gather_kernel, dim3((uint32_t)((npix + kLtThreads - 1) / kLtThreads)), dim3(kLtThreads), 0, st, p);
    return hipGetLastError();
}

}  // namespace srt
