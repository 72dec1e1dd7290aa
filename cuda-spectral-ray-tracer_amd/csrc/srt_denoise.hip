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

__global__ __launch_bounds__(256) void denoise_epilogue_kernel(const float4 *colour, float *out_xyz, float *out_lin, float *out_q, size_t n) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n) return;
    const float4 c = colour[pix];
    const SrgbPixel o = xyz_mean_to_srgb(mk(c.x, c.y, c.z));
    out_xyz[3 * pix + 0] = c.x; out_xyz[3 * pix + 1] = c.y; out_xyz[3 * pix + 2] = c.z;
    out_lin[3 * pix + 0] = o.lin.x; out_lin[3 * pix + 1] = o.lin.y; out_lin[3 * pix + 2] = o.lin.z;
    out_q[3 * pix + 0] = o.q.x; out_q[3 * pix + 1] = o.q.y; out_q[3 * pix + 2] = o.q.z;
}

}  // namespace

hipError_t launch_denoise_prepass(const DenoisePrepassParams &p, hipStream_t st) {
    const size_t n = (size_t)p.w * p.h;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_prepass_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
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

}  // namespace srt
