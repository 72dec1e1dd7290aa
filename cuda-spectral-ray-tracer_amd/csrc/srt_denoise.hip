// srt_denoise.hip -- the edge-avoiding a-trous denoiser over the first-hit feature buffers (srt_denoise_features / srt_denoise_kat,
// include/srt_c_api.h states the filter operation by operation; tests/denoise_reference.py restates it in numpy float32).
//
// A translation unit of its own: the render kernels (srt_kernels.hip) are not touched, and their machine code stays what it was.
// Built with the exactness flags of the render unit (-ffp-contract=off, correctly rounded divide, no fast-math): every expression
// below is evaluated as written, so the device result is predicted bit for bit by the restatement.
//
// Three kernels, all on row-major w x h images of the chunk's rectangle:
//   denoise_prepass_kernel   block-linear lane -> row-major (the mapping of features_unswizzle_kernel), normalises, packs the guides as two
//                            float4 per pixel (N.xyz, z | A.xyz, coverage) and the colour as one float4 (c.xyz, 0)
//   denoise_level_kernel     one level of the 5x5 B3-spline stencil at step s: 25 taps of 48 B per pixel.  A workgroup filters a 32 x 8
//                            tile (a wave = two rows of 32 pixels: its loads are two 512-B runs per float4 array).  TILED (steps 1 and 2):
//                            the tile and its halo of 2 s pixels are staged in LDS once (36 x 12 or 40 x 16 pixels x 48 B <= 30 KiB:
//                            1.7 or 2.5 pixels fetched per pixel filtered instead of 25) and the taps are ds_read_b128 of neighbouring
//                            lanes' neighbouring 16-byte slots (conflict free).  From step 4 on the halo outgrows the tile (48 x 24 pixels
//                            for 256), so the taps come straight from L2 / HBM: the lanes of a row read contiguous 16-byte runs.
//   denoise_epilogue_kernel  the filtered XYZ mean -> unquantised and quantised sRGB through xyz_mean_to_srgb (srt_device.h), three
//                            row-major [h][w][3] outputs
// The variance-guided path (srt_denoise_features_vg) adds three kernels and leaves the three above as they are:
//   denoise_variance_kernel  the spatial estimator: the guide-weighted variance of Y over a 7x7 window at distance 1.  The 32 x 8 tile and
//                            its halo of 3 pixels are staged in LDS -- 38 x 14 pixels of the two guide float4 and Y, 19 152 B -- so a
//                            pixel's 49 taps are two ds_read_b128 (a row's lanes read neighbouring 16-byte slots: the 16 lanes of a
//                            ds_read_b128 group cover 16 distinct slots of the 256-B bank row) and one ds_read_b32 (32 consecutive
//                            dwords per half wave) each: conflict free at any row pitch, so the rows are not padded.  Reads Y and
//                            writes v as 4-byte accesses of the colour image's second and fourth lane: no block reads a word that
//                            another writes.
//   denoise_level_vg_kernel  the sibling of denoise_level_kernel, tiled and direct, both through denoise_vg_tap: the colour float4
//                            carries the variance in .w, the luminance term's width comes from a 3x3 blur of it (tiled: nine more
//                            LDS reads inside the halo of 2 s >= 2; direct: nine 4-byte loads of .w)
//   denoise_prepass_counts_kernel / denoise_measured_kernel: an accumulation whose pixels hold different sample counts (adaptive +
//                            features) -- the prepass with the pixel's own count, and the per-pixel estimator of srt_denoise_features_mv
//                            (the variance of the mean from the pixel's measured S1 and S2); one thread per pixel, no neighbours
//   denoise_var_out_kernel   the variance after the last level -> channel 1 of the [h][w][2] variance output
// The developed payload (srt_denoise_developed) adds three kernels behind all of the above and leaves them as they are:
//   denoise_payload_prepass_kernel  the developed planes [h][w][K] -> d = inv * D as G = KC / 4 float4 groups, [group][pixel], KC the
//                            smallest of {4, 8, 16} that holds K, the padding +0: the lanes of a row read contiguous 16-byte runs
//   denoise_level_dev_kernel the plain level with the payload riding along.  The 25 weights of a pixel are computed ONCE, through
//                            denoise_tap's arithmetic (which also filters the colour), and kept in 25 registers -- the tap loops are
//                            fully unrolled -- then the groups are streamed one after the other: per group the same 25 taps, each read
//                            only where its weight is > 0.  TILED (steps 1 and 2): guides and colour are staged as in
//                            denoise_level_kernel<true> (30 720 B) and each group's tile and halo goes through a fourth 10 240-B array
//                            between two barriers -- 40 960 B static, so four workgroups a CU whatever G is, where staging all groups
//                            at once would need 71 680 B at G = 4.  From step 4 on the taps come from L2 / HBM.
//   denoise_dev_out_kernel   the payload after the last level -> the row-major [h][w][K] output
// An adaptive spectral featured accumulation (pixels with different sample counts) adds one more, behind all of the above:
//   denoise_payload_prepass_counts_kernel  denoise_payload_prepass_kernel with the pixel's own count n_p = counts[idx] & ~kAdaptConverged
//                            in the place of the total (idx: the pixel's block-linear lane, as in denoise_prepass_counts_kernel)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kDnTileW = 32, kDnTileH = 8;                                   // pixels a workgroup of 256 lanes filters
constexpr uint32_t kDnTiledMaxStep = 2;                                           // the LDS tile pays at steps 1 and 2
constexpr uint32_t kDnHaloMax = 2 * kDnTiledMaxStep;
constexpr uint32_t kDnLdsPixels = (kDnTileW + 2 * kDnHaloMax) * (kDnTileH + 2 * kDnHaloMax);      // 40 x 16 = 640 -> 30 KiB

// B3-spline tap weight h[k], k = d + 2: {1/16, 1/4, 3/8, 1/4, 1/16}
__device__ __forceinline__ constexpr float b3_tap(int k) { return (k == 0 || k == 4) ? 0.0625f : (k == 2 ? 0.375f : 0.25f); }

// e(d2, k): 1 at no difference, 0 from d2 >= k on; NaN gives 0, an infinite k gives 1
__device__ __forceinline__ float edge_term(float d2, float k) {
    float t = 1.0f - d2 / k;
    t = (t > 0.0f) ? t : 0.0f;
    return t * t;
}
__device__ __forceinline__ float dist2(float4 a, float4 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}

struct TapSums { float sw, sx, sy, sz; };
// one tap q of pixel p (srt_c_api.h, "For tap q"): g0 = (N.xyz, z), g1 = (A.xyz, coverage), c = the current level's colour
__device__ __forceinline__ void denoise_tap(TapSums &s, float h2, float4 p_g0, float4 p_g1, float4 p_c, float4 q_g0, float4 q_g1, float4 q_c,
                                            float kn, float ka, float kz, float kc) {
    const float dn = dist2(p_g0, q_g0);
    const float da = dist2(p_g1, q_g1);
    const float dc = dist2(p_c, q_c);
    const float zp = p_g0.w, zq = q_g0.w;
    const float m = (zp > zq) ? zp : zq;      // max(z_p, z_q) as a select (the restatement's np.where)
    const float r = (m > 0.0f) ? (zp - zq) / m : 0.0f;
    const float dz = r * r;
    float wt = h2;
    wt = wt * edge_term(dn, kn);
    wt = wt * edge_term(da, ka);
    wt = wt * edge_term(dz, kz);
    wt = wt * edge_term(dc, kc);
    if (wt > 0.0f) {
        s.sw += wt;
        s.sx += wt * q_c.x; s.sy += wt * q_c.y; s.sz += wt * q_c.z;
    }
}

__global__ __launch_bounds__(256) void denoise_prepass_kernel(const DenoisePrepassParams P) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)P.w * P.h) return;
    const uint32_t y = (uint32_t)(pix / P.w), x = (uint32_t)(pix - (size_t)y * P.w);
    const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
    const float *s = P.sums + idx * P.sum_pixel_stride;
    const float4 f0 = P.rows[idx * (kFeatureStride / 4u) + 0], f1 = P.rows[idx * (kFeatureStride / 4u) + 1];
    const float inv = 1.0f / (float)P.samples;
    const float z = (f1.w > 0.0f) ? f1.z / f1.w : 0.0f;
    P.colour[pix] = make_float4(inv * s[0], inv * s[P.sum_comp_stride], inv * s[2 * P.sum_comp_stride], 0.0f);
    P.guides[2 * pix + 0] = make_float4(inv * f0.x, inv * f0.y, inv * f0.z, z);
    P.guides[2 * pix + 1] = make_float4(inv * f0.w, inv * f1.x, inv * f1.y, inv * f1.w);
}

// the prepass of an accumulation whose pixels hold different sample counts (adaptive + features, srt_denoise_mv_kat): the kernel above
// with the pixel's own count n_p = counts[idx] & ~kAdaptConverged in the place of the global total, and nothing else changed
__global__ __launch_bounds__(256) void denoise_prepass_counts_kernel(const DenoisePrepassParams P) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)P.w * P.h) return;
    const uint32_t y = (uint32_t)(pix / P.w), x = (uint32_t)(pix - (size_t)y * P.w);
    const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
    const float *s = P.sums + idx * P.sum_pixel_stride;
    const float4 f0 = P.rows[idx * (kFeatureStride / 4u) + 0], f1 = P.rows[idx * (kFeatureStride / 4u) + 1];
    const uint32_t n_p = P.counts[idx] & ~kAdaptConverged;
    const float inv = 1.0f / (float)n_p;
    const float z = (f1.w > 0.0f) ? f1.z / f1.w : 0.0f;
    P.colour[pix] = make_float4(inv * s[0], inv * s[P.sum_comp_stride], inv * s[2 * P.sum_comp_stride], 0.0f);
    P.guides[2 * pix + 0] = make_float4(inv * f0.x, inv * f0.y, inv * f0.z, z);
    P.guides[2 * pix + 1] = make_float4(inv * f0.w, inv * f1.x, inv * f1.y, inv * f1.w);
}

// the measured estimator (srt_c_api.h, srt_denoise_features_mv): the variance of the pixel's mean luminance from its own S1, S2 and count
// -- the first four operations of the stopping rule (adaptive_converged, srt_kernels.hip), in that order; no neighbour is read
__global__ __launch_bounds__(256) void denoise_measured_kernel(const DenoiseMeasuredParams P) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)P.w * P.h) return;
    const uint32_t y = (uint32_t)(pix / P.w), x = (uint32_t)(pix - (size_t)y * P.w);
    const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
    const uint32_t n_p = P.counts[idx] & ~kAdaptConverged;
    const float s1 = P.sum_y[idx * P.sum_pixel_stride], s2 = P.sum_y2[idx];
    const float n = (float)n_p;
    const float mean = s1 / n;
    const float mm = mean * mean;
    float v = s2 / n - mm;
    v = v > 0.0f ? v : 0.0f;
    const float vm = v / (n - 1.0f);
    const float o = (n_p >= 2u && (vm - vm) == 0.0f) ? vm : 0.0f;
    P.colour[4 * pix + 3] = o;
    P.out_var[2 * pix + 0] = o;
}

template <bool TILED>
__global__ __launch_bounds__(256) void denoise_level_kernel(const DenoiseLevelParams P) {
    // the workgroup's tile: blocks run row-major over the tiles of the image (a 1-D grid: no 65535 limit on the rows)
    const uint32_t tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x0 = tile_x * kDnTileW, y0 = tile_y * kDnTileH;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const int step = (int)P.step;

    __shared__ float4 t_g0[TILED ? kDnLdsPixels : 1], t_g1[TILED ? kDnLdsPixels : 1], t_c[TILED ? kDnLdsPixels : 1];
    const uint32_t halo = 2u * P.step, lw = kDnTileW + 2u * halo, lh = kDnTileH + 2u * halo;      // (TILED: step <= 2, lw * lh <= kDnLdsPixels)
    if constexpr (TILED) {
        for (uint32_t i = threadIdx.x; i < lw * lh; i += 256u) {
            const uint32_t ty = i / lw, tx = i - ty * lw;
            const long long gx = (long long)x0 + tx - halo, gy = (long long)y0 + ty - halo;
            float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, c = g0;      // outside the rectangle: never read as a tap
            if (gx >= 0 && gx < (long long)P.w && gy >= 0 && gy < (long long)P.h) {
                const size_t q = (size_t)gy * P.w + (size_t)gx;
                g0 = P.guides[2 * q + 0]; g1 = P.guides[2 * q + 1]; c = P.src[q];
            }
            t_g0[i] = g0; t_g1[i] = g1; t_c[i] = c;
        }
        __syncthreads();
    }
    if (x >= P.w || y >= P.h) return;

    const size_t p = (size_t)y * P.w + x;
    float4 p_g0, p_g1, p_c;
    if constexpr (TILED) {
        const uint32_t i = (ly + halo) * lw + lx + halo;
        p_g0 = t_g0[i]; p_g1 = t_g1[i]; p_c = t_c[i];
    } else {
        p_g0 = P.guides[2 * p + 0]; p_g1 = P.guides[2 * p + 1]; p_c = P.src[p];
    }
    TapSums s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const long long qy = (long long)y + dy * step;
        if (qy < 0 || qy >= (long long)P.h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const long long qx = (long long)x + dx * step;
            if (qx < 0 || qx >= (long long)P.w) continue;
            float4 q_g0, q_g1, q_c;
            if constexpr (TILED) {
                const uint32_t i = (uint32_t)((int)(ly + halo) + dy * step) * lw + (uint32_t)((int)(lx + halo) + dx * step);
                q_g0 = t_g0[i]; q_g1 = t_g1[i]; q_c = t_c[i];
            } else {
                const size_t q = (size_t)qy * P.w + (size_t)qx;
                q_g0 = P.guides[2 * q + 0]; q_g1 = P.guides[2 * q + 1]; q_c = P.src[q];
            }
            denoise_tap(s, b3_tap(dy + 2) * b3_tap(dx + 2), p_g0, p_g1, p_c, q_g0, q_g1, q_c, P.kn, P.ka, P.kz, P.kc);
        }
    }
    float4 o = p_c;
    if (s.sw > 0.0f) o = make_float4(s.sx / s.sw, s.sy / s.sw, s.sz / s.sw, 0.0f);
    P.dst[p] = o;
}

// ---- the variance-guided path --------------------------------------------------------------------------------------------------------
constexpr uint32_t kDnVarHalo = 3;                                                // the estimator's 7x7 window
constexpr uint32_t kDnVarLdsW = kDnTileW + 2 * kDnVarHalo, kDnVarLdsH = kDnTileH + 2 * kDnVarHalo;      // 38 x 14 = 532 pixels x 36 B
constexpr uint32_t kDnVarLdsPixels = kDnVarLdsW * kDnVarLdsH;

// the variance blur's tap weight b[k], k = d + 1: {1/4, 1/2, 1/4}
__device__ __forceinline__ constexpr float blur_tap(int k) { return k == 1 ? 0.5f : 0.25f; }

// e(dn, kn), e(da, ka), e(dz, kz) of a tap, multiplied into w0 left to right (dn, da, dz as in denoise_tap)
__device__ __forceinline__ float guide_weight(float w0, float4 p_g0, float4 p_g1, float4 q_g0, float4 q_g1, float kn, float ka, float kz) {
    const float dn = dist2(p_g0, q_g0);
    const float da = dist2(p_g1, q_g1);
    const float zp = p_g0.w, zq = q_g0.w;
    const float m = (zp > zq) ? zp : zq;
    const float r = (m > 0.0f) ? (zp - zq) / m : 0.0f;
    const float dz = r * r;
    float wt = w0;
    wt = wt * edge_term(dn, kn);
    wt = wt * edge_term(da, ka);
    wt = wt * edge_term(dz, kz);
    return wt;
}

struct VarSums { float s0, s1, s2; };
// one tap of the estimator (srt_c_api.h, "Estimator"): counted only with a finite Y_q
__device__ __forceinline__ void variance_tap(VarSums &s, float4 p_g0, float4 p_g1, float4 q_g0, float4 q_g1, float yq, float kn, float ka, float kz) {
    const float g = guide_weight(1.0f, p_g0, p_g1, q_g0, q_g1, kn, ka, kz);      // (1 * e is e: the first product is exact)
    if (g > 0.0f && (yq - yq) == 0.0f) {
        s.s0 += g;
        s.s1 += g * yq;
        s.s2 += g * (yq * yq);
    }
}

struct VgTapSums { float sw, sx, sy, sz, sv; };
// one tap q of pixel p of a variance-guided level (srt_c_api.h, "Variance-guided level"): c = (colour.xyz, variance)
__device__ __forceinline__ void denoise_vg_tap(VgTapSums &s, float h2, float4 p_g0, float4 p_g1, float4 p_c, float4 q_g0, float4 q_g1, float4 q_c,
                                               float kn, float ka, float kz, float kc) {
    const float dc = dist2(p_c, q_c);
    const float d = p_c.y - q_c.y;
    const float dl = d * d;
    float wt = guide_weight(h2, p_g0, p_g1, q_g0, q_g1, kn, ka, kz);
    wt = wt * edge_term(dl, kc);
    if (wt > 0.0f && (dc - dc) == 0.0f) {
        s.sw += wt;
        s.sx += wt * q_c.x; s.sy += wt * q_c.y; s.sz += wt * q_c.z;
        s.sv += (wt * wt) * q_c.w;
    }
}

__global__ __launch_bounds__(256) void denoise_variance_kernel(const DenoiseVarianceParams P) {
    const uint32_t tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x0 = tile_x * kDnTileW, y0 = tile_y * kDnTileH;
    const uint32_t x = x0 + lx, y = y0 + ly;

    __shared__ float4 t_g0[kDnVarLdsPixels], t_g1[kDnVarLdsPixels];
    __shared__ float t_y[kDnVarLdsPixels];
    for (uint32_t i = threadIdx.x; i < kDnVarLdsPixels; i += 256u) {
        const uint32_t ty = i / kDnVarLdsW, tx = i - ty * kDnVarLdsW;
        const long long gx = (long long)x0 + tx - kDnVarHalo, gy = (long long)y0 + ty - kDnVarHalo;
        float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0;      // outside the rectangle: never read as a tap
        float yv = 0.0f;
        if (gx >= 0 && gx < (long long)P.w && gy >= 0 && gy < (long long)P.h) {
            const size_t q = (size_t)gy * P.w + (size_t)gx;
            g0 = P.guides[2 * q + 0]; g1 = P.guides[2 * q + 1]; yv = P.colour[4 * q + 1];
        }
        t_g0[i] = g0; t_g1[i] = g1; t_y[i] = yv;
    }
    __syncthreads();
    if (x >= P.w || y >= P.h) return;

    const uint32_t ip = (ly + kDnVarHalo) * kDnVarLdsW + lx + kDnVarHalo;
    const float4 p_g0 = t_g0[ip], p_g1 = t_g1[ip];
    VarSums s = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -3; dy <= 3; dy++) {
        const long long qy = (long long)y + dy;
        if (qy < 0 || qy >= (long long)P.h) continue;
#pragma unroll
        for (int dx = -3; dx <= 3; dx++) {
            const long long qx = (long long)x + dx;
            if (qx < 0 || qx >= (long long)P.w) continue;
            const uint32_t i = (uint32_t)((int)ip + dy * (int)kDnVarLdsW + dx);
            variance_tap(s, p_g0, p_g1, t_g0[i], t_g1[i], t_y[i], P.kn, P.ka, P.kz);
        }
    }
    const float mu = s.s1 / s.s0, m2 = s.s2 / s.s0;
    const float v = m2 - mu * mu;
    const float o = (s.s0 > 0.0f && v > 0.0f) ? v : 0.0f;
    const size_t p = (size_t)y * P.w + x;
    P.colour[4 * p + 3] = o;
    P.out_var[2 * p + 0] = o;
}

template <bool TILED>
__global__ __launch_bounds__(256) void denoise_level_vg_kernel(const DenoiseLevelVgParams P) {
    const uint32_t tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x0 = tile_x * kDnTileW, y0 = tile_y * kDnTileH;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const int step = (int)P.step;

    __shared__ float4 t_g0[TILED ? kDnLdsPixels : 1], t_g1[TILED ? kDnLdsPixels : 1], t_c[TILED ? kDnLdsPixels : 1];
    const uint32_t halo = 2u * P.step, lw = kDnTileW + 2u * halo, lh = kDnTileH + 2u * halo;      // (TILED: step <= 2, lw * lh <= kDnLdsPixels)
    if constexpr (TILED) {
        for (uint32_t i = threadIdx.x; i < lw * lh; i += 256u) {
            const uint32_t ty = i / lw, tx = i - ty * lw;
            const long long gx = (long long)x0 + tx - halo, gy = (long long)y0 + ty - halo;
            float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, c = g0;      // outside the rectangle: never read as a tap
            if (gx >= 0 && gx < (long long)P.w && gy >= 0 && gy < (long long)P.h) {
                const size_t q = (size_t)gy * P.w + (size_t)gx;
                g0 = P.guides[2 * q + 0]; g1 = P.guides[2 * q + 1]; c = P.src[q];
            }
            t_g0[i] = g0; t_g1[i] = g1; t_c[i] = c;
        }
        __syncthreads();
    }
    if (x >= P.w || y >= P.h) return;

    const size_t p = (size_t)y * P.w + x;
    const uint32_t ip = (ly + halo) * lw + lx + halo;      // (TILED only)
    float4 p_g0, p_g1, p_c;
    if constexpr (TILED) {
        p_g0 = t_g0[ip]; p_g1 = t_g1[ip]; p_c = t_c[ip];
    } else {
        p_g0 = P.guides[2 * p + 0]; p_g1 = P.guides[2 * p + 1]; p_c = P.src[p];
    }
    // the luminance term's width: the 3x3 blur of the input variance at distance 1 (the halo is 2 s >= 2 pixels wide)
    float bk = 0.0f, bv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const long long qy = (long long)y + dy;
        if (qy < 0 || qy >= (long long)P.h) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const long long qx = (long long)x + dx;
            if (qx < 0 || qx >= (long long)P.w) continue;
            float vq;
            if constexpr (TILED) vq = t_c[(uint32_t)((int)ip + dy * (int)lw + dx)].w;
            else vq = reinterpret_cast<const float *>(P.src)[4 * ((size_t)qy * P.w + (size_t)qx) + 3];
            const float k = blur_tap(dy + 1) * blur_tap(dx + 1);
            bk += k;
            bv += k * vq;
        }
    }
    const float vb = bv / bk;
    const float kc = P.ks * vb + P.floor;

    VgTapSums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const long long qy = (long long)y + dy * step;
        if (qy < 0 || qy >= (long long)P.h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const long long qx = (long long)x + dx * step;
            if (qx < 0 || qx >= (long long)P.w) continue;
            float4 q_g0, q_g1, q_c;
            if constexpr (TILED) {
                const uint32_t i = (uint32_t)((int)(ly + halo) + dy * step) * lw + (uint32_t)((int)(lx + halo) + dx * step);
                q_g0 = t_g0[i]; q_g1 = t_g1[i]; q_c = t_c[i];
            } else {
                const size_t q = (size_t)qy * P.w + (size_t)qx;
                q_g0 = P.guides[2 * q + 0]; q_g1 = P.guides[2 * q + 1]; q_c = P.src[q];
            }
            denoise_vg_tap(s, b3_tap(dy + 2) * b3_tap(dx + 2), p_g0, p_g1, p_c, q_g0, q_g1, q_c, P.kn, P.ka, P.kz, kc);
        }
    }
    float4 o = p_c;
    if (s.sw > 0.0f) o = make_float4(s.sx / s.sw, s.sy / s.sw, s.sz / s.sw, s.sv / (s.sw * s.sw));
    P.dst[p] = o;
}

__global__ __launch_bounds__(256) void denoise_var_out_kernel(const float4 *colour, float *out_var, size_t n) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n) return;
    out_var[2 * pix + 1] = colour[pix].w;
}

__global__ __launch_bounds__(256) void denoise_epilogue_kernel(const float4 *colour, float *out_xyz, float *out_lin, float *out_q, size_t n) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n) return;
    const float4 c = colour[pix];
    const SrgbPixel o = xyz_mean_to_srgb(mk(c.x, c.y, c.z));
    out_xyz[3 * pix + 0] = c.x; out_xyz[3 * pix + 1] = c.y; out_xyz[3 * pix + 2] = c.z;
    out_lin[3 * pix + 0] = o.lin.x; out_lin[3 * pix + 1] = o.lin.y; out_lin[3 * pix + 2] = o.lin.z;
    out_q[3 * pix + 0] = o.q.x; out_q[3 * pix + 1] = o.q.y; out_q[3 * pix + 2] = o.q.z;
}

// ---- the developed payload (srt_denoise_developed) -----------------------------------------------------------------------------------
// one tap q of pixel p with the weight handed back: denoise_tap's operations in denoise_tap's order (the colour sums are its bits), and
// the tap's weight where it counts, +0 where it does not -- the payload of such a tap is never multiplied
__device__ __forceinline__ float denoise_tap_weight(TapSums &s, float h2, float4 p_g0, float4 p_g1, float4 p_c, float4 q_g0, float4 q_g1, float4 q_c,
                                                    float kn, float ka, float kz, float kc) {
    const float dn = dist2(p_g0, q_g0);
    const float da = dist2(p_g1, q_g1);
    const float dc = dist2(p_c, q_c);
    const float zp = p_g0.w, zq = q_g0.w;
    const float m = (zp > zq) ? zp : zq;
    const float r = (m > 0.0f) ? (zp - zq) / m : 0.0f;
    const float dz = r * r;
    float wt = h2;
    wt = wt * edge_term(dn, kn);
    wt = wt * edge_term(da, ka);
    wt = wt * edge_term(dz, kz);
    wt = wt * edge_term(dc, kc);
    if (wt > 0.0f) {
        s.sw += wt;
        s.sx += wt * q_c.x; s.sy += wt * q_c.y; s.sz += wt * q_c.z;
        return wt;
    }
    return 0.0f;
}

__global__ __launch_bounds__(256) void denoise_payload_prepass_kernel(const DenoisePayloadPrepassParams P) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= P.pixels) return;
    const float inv = 1.0f / (float)P.samples;
    const float *d = P.developed + pix * P.channels;
    for (uint32_t g = 0; g < P.groups; g++) {
        float v[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            const uint32_t k = 4u * g + e;
            v[e] = (k < P.channels) ? inv * d[k] : 0.0f;
        }
        P.payload[(size_t)g * P.pixels + pix] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

template <bool TILED>
__global__ __launch_bounds__(256) void denoise_level_dev_kernel(const DenoiseLevelDevParams P) {
    const uint32_t tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const uint32_t x0 = tile_x * kDnTileW, y0 = tile_y * kDnTileH;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const int step = (int)P.step;
    const size_t pixels = (size_t)P.w * P.h;

    __shared__ float4 t_g0[TILED ? kDnLdsPixels : 1], t_g1[TILED ? kDnLdsPixels : 1], t_c[TILED ? kDnLdsPixels : 1], t_d[TILED ? kDnLdsPixels : 1];
    const uint32_t halo = 2u * P.step, lw = kDnTileW + 2u * halo, lh = kDnTileH + 2u * halo;      // (TILED: step <= 2, lw * lh <= kDnLdsPixels)
    if constexpr (TILED) {
        for (uint32_t i = threadIdx.x; i < lw * lh; i += 256u) {
            const uint32_t ty = i / lw, tx = i - ty * lw;
            const long long gx = (long long)x0 + tx - halo, gy = (long long)y0 + ty - halo;
            float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, c = g0;      // outside the rectangle: never read as a tap
            if (gx >= 0 && gx < (long long)P.w && gy >= 0 && gy < (long long)P.h) {
                const size_t q = (size_t)gy * P.w + (size_t)gx;
                g0 = P.guides[2 * q + 0]; g1 = P.guides[2 * q + 1]; c = P.src[q];
            }
            t_g0[i] = g0; t_g1[i] = g1; t_c[i] = c;
        }
        __syncthreads();
    }
    // (no early return: the lanes outside the rectangle stay for the barriers of the group loop, with 25 zero weights)
    const bool mine = x < P.w && y < P.h;
    const size_t p = mine ? (size_t)y * P.w + x : 0;
    const uint32_t ip = (ly + halo) * lw + lx + halo;      // (TILED only)

    float wts[25];
    TapSums s = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 p_c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (mine) {
        float4 p_g0, p_g1;
        if constexpr (TILED) {
            p_g0 = t_g0[ip]; p_g1 = t_g1[ip]; p_c = t_c[ip];
        } else {
            p_g0 = P.guides[2 * p + 0]; p_g1 = P.guides[2 * p + 1]; p_c = P.src[p];
        }
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const long long qy = (long long)y + dy * step;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const long long qx = (long long)x + dx * step;
                float wt = 0.0f;
                if (qy >= 0 && qy < (long long)P.h && qx >= 0 && qx < (long long)P.w) {
                    float4 q_g0, q_g1, q_c;
                    if constexpr (TILED) {
                        const uint32_t i = (uint32_t)((int)ip + (dy * step) * (int)lw + dx * step);
                        q_g0 = t_g0[i]; q_g1 = t_g1[i]; q_c = t_c[i];
                    } else {
                        const size_t q = (size_t)qy * P.w + (size_t)qx;
                        q_g0 = P.guides[2 * q + 0]; q_g1 = P.guides[2 * q + 1]; q_c = P.src[q];
                    }
                    wt = denoise_tap_weight(s, b3_tap(dy + 2) * b3_tap(dx + 2), p_g0, p_g1, p_c, q_g0, q_g1, q_c, P.kn, P.ka, P.kz, P.kc);
                }
                wts[(dy + 2) * 5 + (dx + 2)] = wt;
            }
        }
        float4 o = p_c;
        if (s.sw > 0.0f) o = make_float4(s.sx / s.sw, s.sy / s.sw, s.sz / s.sw, 0.0f);
        P.dst[p] = o;
    } else {
#pragma unroll
        for (int i = 0; i < 25; i++) wts[i] = 0.0f;
    }

    // the payload: group after group through the same 25 weights; a tap whose weight is not > 0 is not read (it may lie outside the rectangle)
    for (uint32_t g = 0; g < P.groups; g++) {
        const float4 *psrc = P.psrc + (size_t)g * pixels;
        if constexpr (TILED) {
            if (g) __syncthreads();      // (the previous group's taps have been read)
            for (uint32_t i = threadIdx.x; i < lw * lh; i += 256u) {
                const uint32_t ty = i / lw, tx = i - ty * lw;
                const long long gx = (long long)x0 + tx - halo, gy = (long long)y0 + ty - halo;
                float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gx >= 0 && gx < (long long)P.w && gy >= 0 && gy < (long long)P.h) d = psrc[(size_t)gy * P.w + (size_t)gx];
                t_d[i] = d;
            }
            __syncthreads();
        }
        if (!mine) continue;
        float4 sd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const float wt = wts[(dy + 2) * 5 + (dx + 2)];
                if (wt > 0.0f) {
                    float4 d;
                    if constexpr (TILED) d = t_d[(uint32_t)((int)ip + (dy * step) * (int)lw + dx * step)];
                    else d = psrc[(size_t)((long long)y + dy * step) * P.w + (size_t)((long long)x + dx * step)];
                    sd.x += wt * d.x; sd.y += wt * d.y; sd.z += wt * d.z; sd.w += wt * d.w;
                }
            }
        }
        float4 o;
        if (s.sw > 0.0f) o = make_float4(sd.x / s.sw, sd.y / s.sw, sd.z / s.sw, sd.w / s.sw);
        else if constexpr (TILED) o = t_d[ip];
        else o = psrc[p];
        P.pdst[(size_t)g * pixels + p] = o;
    }
}

__global__ __launch_bounds__(256) void denoise_dev_out_kernel(const float4 *payload, float *out_dev, uint32_t channels, uint32_t groups, size_t n) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n) return;
    float *o = out_dev + pix * channels;
    for (uint32_t g = 0; g < groups; g++) {
        const float4 d = payload[(size_t)g * n + pix];
        const uint32_t k = 4u * g;
        if (k + 0u < channels) o[k + 0u] = d.x;
        if (k + 1u < channels) o[k + 1u] = d.y;
        if (k + 2u < channels) o[k + 2u] = d.z;
        if (k + 3u < channels) o[k + 3u] = d.w;
    }
}

// the payload prepass of an accumulation whose pixels hold different sample counts (adaptive + spectral + features,
// srt_denoise_developed_counts_kat): denoise_payload_prepass_kernel with the pixel's own count, read as denoise_prepass_counts_kernel
// reads it, in the place of the global total, and nothing else changed
__global__ __launch_bounds__(256) void denoise_payload_prepass_counts_kernel(const DenoisePayloadPrepassCountsParams P) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)P.w * P.h) return;
    const size_t pixels = (size_t)P.w * P.h;
    const uint32_t y = (uint32_t)(pix / P.w), x = (uint32_t)(pix - (size_t)y * P.w);
    const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
    const uint32_t n_p = P.counts[idx] & ~kAdaptConverged;
    const float inv = 1.0f / (float)n_p;
    const float *d = P.developed + pix * P.channels;
    for (uint32_t g = 0; g < P.groups; g++) {
        float v[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            const uint32_t k = 4u * g + e;
            v[e] = (k < P.channels) ? inv * d[k] : 0.0f;
        }
        P.payload[(size_t)g * pixels + pix] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

}  // namespace

hipError_t launch_denoise_prepass(const DenoisePrepassParams &p, hipStream_t st) {
    const size_t n = (size_t)p.w * p.h;
    if (n == 0) return hipSuccess;
    if (p.counts) hipLaunchKernelGGL(denoise_prepass_counts_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(denoise_prepass_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_measured(const DenoiseMeasuredParams &p, hipStream_t st) {
    const size_t n = (size_t)p.w * p.h;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_measured_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_level(const DenoiseLevelParams &p_in, hipStream_t st) {
    DenoiseLevelParams p = p_in;
    if (p.w == 0 || p.h == 0) return hipSuccess;
    p.tiles_x = (p.w + kDnTileW - 1u) / kDnTileW;
    const uint64_t blocks = (uint64_t)p.tiles_x * ((p.h + kDnTileH - 1u) / kDnTileH);
    if (blocks > 0x7fffffffull || p.step == 0 || p.step > 128u) return hipErrorInvalidValue;
    if (p.step <= kDnTiledMaxStep) hipLaunchKernelGGL(denoise_level_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(denoise_level_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_epilogue(const float *colour, float *out_xyz, float *out_lin, float *out_q, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_epilogue_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4 *>(colour), out_xyz,
                       out_lin, out_q, n);
    return hipGetLastError();
}

hipError_t launch_denoise_variance(const DenoiseVarianceParams &p_in, hipStream_t st) {
    DenoiseVarianceParams p = p_in;
    if (p.w == 0 || p.h == 0) return hipSuccess;
    p.tiles_x = (p.w + kDnTileW - 1u) / kDnTileW;
    const uint64_t blocks = (uint64_t)p.tiles_x * ((p.h + kDnTileH - 1u) / kDnTileH);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(denoise_variance_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_level_vg(const DenoiseLevelVgParams &p_in, hipStream_t st) {
    DenoiseLevelVgParams p = p_in;
    if (p.w == 0 || p.h == 0) return hipSuccess;
    p.tiles_x = (p.w + kDnTileW - 1u) / kDnTileW;
    const uint64_t blocks = (uint64_t)p.tiles_x * ((p.h + kDnTileH - 1u) / kDnTileH);
    if (blocks > 0x7fffffffull || p.step == 0 || p.step > 128u) return hipErrorInvalidValue;
    if (p.step <= kDnTiledMaxStep) hipLaunchKernelGGL(denoise_level_vg_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(denoise_level_vg_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_var_out(const float *colour, float *out_var, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_var_out_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4 *>(colour), out_var, n);
    return hipGetLastError();
}

uint32_t denoise_payload_groups(uint32_t channels) {
    for (const uint32_t kc : {4u, 8u, 16u})
        if (channels <= kc) return kc / 4u;
    return 0;
}

hipError_t launch_denoise_payload_prepass(const DenoisePayloadPrepassParams &p, hipStream_t st) {
    if (p.channels == 0 || p.channels > kMaxDevelopChannels || p.groups != denoise_payload_groups(p.channels) || p.samples == 0) return hipErrorInvalidValue;
    if (p.pixels == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_payload_prepass_kernel, dim3((uint32_t)((p.pixels + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_payload_prepass_counts(const DenoisePayloadPrepassCountsParams &p, hipStream_t st) {
    if (p.channels == 0 || p.channels > kMaxDevelopChannels || p.groups != denoise_payload_groups(p.channels) || !p.counts || p.tx == 0 || p.ty == 0 || p.bx == 0)
        return hipErrorInvalidValue;
    const size_t n = (size_t)p.w * p.h;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_payload_prepass_counts_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_level_dev(const DenoiseLevelDevParams &p_in, hipStream_t st) {
    DenoiseLevelDevParams p = p_in;
    if (p.w == 0 || p.h == 0) return hipSuccess;
    p.tiles_x = (p.w + kDnTileW - 1u) / kDnTileW;
    const uint64_t blocks = (uint64_t)p.tiles_x * ((p.h + kDnTileH - 1u) / kDnTileH);
    if (blocks > 0x7fffffffull || p.step == 0 || p.step > 128u || p.groups == 0 || p.groups > kMaxDevelopChannels / 4u) return hipErrorInvalidValue;
    if (p.step <= kDnTiledMaxStep) hipLaunchKernelGGL(denoise_level_dev_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(denoise_level_dev_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_denoise_dev_out(const float4 *payload, float *out_dev, uint32_t channels, uint32_t groups, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_dev_out_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, payload, out_dev, channels, groups, n);
    return hipGetLastError();
}

}  // namespace srt
