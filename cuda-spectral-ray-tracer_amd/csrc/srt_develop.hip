// srt_develop.hip -- the spectral film developed on the device (srt_develop_spectral / srt_develop_spectral_srgb / srt_develop_kat;
// include/srt_c_api.h states the contraction operation by operation, tests/develop_reference.py restates it in numpy float32).
//
// A translation unit of its own, like the denoiser: the render and denoise kernels are not touched and their machine code stays what it
// was.  Built with the exactness flags of the render unit (-ffp-contract=off, no fast-math): every product and every sum below is
// rounded once, in the order written, so the restatement predicts the device's bits.
//
// Two kernels:
//   develop_kernel<KC>    out_k = (sum over j = 0 .. 94, ascending, of F_j * R[k][j]) * scale for up to KC channels of every pixel.
//                         Bandwidth work -- 384 B in per pixel, at most 64 B out -- so the film is read as whole 128-B lines: a workgroup
//                         is ONE wave and owns the 64 consecutive block-linear lanes [64 b, 64 b + 64), whose rows are one contiguous
//                         24 576-B run of the film.  The wave fetches it as 24 global_load_dwordx4 per lane, neighbouring lanes on
//                         neighbouring 16-byte slots, all 24 in flight at once (96 registers: LDS, not registers, bounds the occupancy), and writes it to an LDS tile with a row pitch of
//                         97 dwords; after that lane l walks row l in ascending j with one ds_read_b32 per sample: bank
//                         (97 l + j) mod 32 = (l + j) mod 32, distinct over the 32 lanes of a half wave -- conflict free.  The tile is
//                         64 x 97 x 4 = 24 832 B, the only LDS of the kernel: six workgroups fit in a CU's 160 KiB.
//                         The responses are uniform over the lanes: the host hands them over transposed and padded, [95][KC], and the
//                         loop reads them with wave-uniform addresses, i.e. through the scalar cache into scalar registers; a product
//                         takes its response straight from there.  KC is the smallest of {1, 2, 3, 4, 8, 16} that holds the call's
//                         channels (the padding's responses are +0 and its results are not stored): KC accumulators are KC registers,
//                         so sixteen channels fit in one walk over the tile and no channel groups are needed.
//                         The result goes to the row-major rectangle through the inverse of block_linear_idx (a KAT call makes the map
//                         the identity with tx = n, ty = 1, bx = 1).  A tile without a pixel of the rectangle is skipped before it loads
//                         anything.  No atomics, no scratch.
//   develop_srgb_kernel   three developed channels taken as XYZ sums of `samples` samples -> unquantised and quantised sRGB: the render
//                         kernel's normalisation (inv = 1.0f / (float)samples; c = inv * sum) and xyz_mean_to_srgb (srt_device.h)
// An adaptive spectral accumulation, whose pixels hold different sample counts, adds a third behind them and leaves them as they are:
//   develop_srgb_counts_kernel  develop_srgb_kernel with the pixel's own count n_p = counts[idx] & ~kAdaptConverged in the place of the
//                         total, idx the pixel's block-linear lane (the state words are indexed like the film), and nothing else changed
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kDevTilePixels = 64;                                  // one wave, one lane per pixel
constexpr uint32_t kDevPitch = kFilmStride + 1u;                         // 97 dwords: odd, so a lane's walk over its row never shares a bank
constexpr uint32_t kDevRowF4 = kFilmStride / 4u;                         // 24 sixteen-byte slots per film row
constexpr uint32_t kDevTileF4 = kDevTilePixels * kDevRowF4;              // 1536 slots per tile: 24 per lane
constexpr uint32_t kDevBatch = 24;                                       // loads in flight per lane: the whole tile
static_assert(kDevTileF4 % (kDevTilePixels * kDevBatch) == 0, "the tile is a whole number of load batches");
static_assert(kFilmStride % 4u == 0, "a 16-byte slot never straddles two film rows");

template <int KC>
__global__ __launch_bounds__(64) void develop_kernel(const DevelopParams P) {
    __shared__ float tile[kDevTilePixels * kDevPitch];
    const uint32_t lane = threadIdx.x;
    const uint32_t idx0 = blockIdx.x * kDevTilePixels, idx = idx0 + lane;
    const PixelIJ px = block_linear_pixel(idx, P.tx, P.ty, P.bx);
    const bool mine = idx < P.n_lanes && px.i < P.w && px.j < P.h;
    if (__ballot(mine) == 0ull) return;      // (the workgroup is this one wave: the whole tile lies outside the rectangle)

    // stage: the tile's rows are contiguous in the film; slots of lanes beyond the grid (the last tile of a KAT film) read as +0
    const float4 *src = reinterpret_cast<const float4 *>(P.film) + (size_t)idx0 * kDevRowF4;
    const uint32_t rows_here = (P.n_lanes - idx0 < kDevTilePixels) ? P.n_lanes - idx0 : kDevTilePixels;
    const uint32_t valid_f4 = rows_here * kDevRowF4;
    for (uint32_t b = 0; b < kDevTileF4 / kDevTilePixels; b += kDevBatch) {
        float4 v[kDevBatch];
#pragma unroll
        for (uint32_t u = 0; u < kDevBatch; u++) {
            const uint32_t e = (b + u) * kDevTilePixels + lane;
            v[u] = (e < valid_f4) ? src[e] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (uint32_t u = 0; u < kDevBatch; u++) {
            const uint32_t e = (b + u) * kDevTilePixels + lane;
            const uint32_t r = e / kDevRowF4, s = e - r * kDevRowF4;
            float *d = tile + r * kDevPitch + 4u * s;
            d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
        }
    }
    __syncthreads();

    // contract: a_k = +0; for j ascending: t = F_j * R[k][j]; a_k = a_k + t (the row's 96th word is never read)
    const float *row = tile + lane * kDevPitch;
    const float *__restrict__ R = P.response;      // [95][KC], wave-uniform addresses
    float a[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) a[k] = 0.0f;
#pragma unroll 5
    for (uint32_t j = 0; j < kFilmSamples; j++) {
        const float f = row[j];
#pragma unroll
        for (int k = 0; k < KC; k++) {
            const float t = f * R[j * KC + k];
            a[k] = a[k] + t;
        }
    }
    if (!mine) return;
    float *o = P.out + ((size_t)px.j * P.w + px.i) * P.channels;
#pragma unroll
    for (int k = 0; k < KC; k++)
        if ((uint32_t)k < P.channels) o[k] = a[k] * P.scale;
}

__global__ __launch_bounds__(256) void develop_srgb_kernel(const float *xyz, float *out_lin, float *out_q, uint32_t samples, size_t n) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n) return;
    const float inv = 1.0f / (float)samples;
    const SrgbPixel o = xyz_mean_to_srgb(mk(inv * xyz[3 * pix + 0], inv * xyz[3 * pix + 1], inv * xyz[3 * pix + 2]));
    if (out_lin) { out_lin[3 * pix + 0] = o.lin.x; out_lin[3 * pix + 1] = o.lin.y; out_lin[3 * pix + 2] = o.lin.z; }
    if (out_q) { out_q[3 * pix + 0] = o.q.x; out_q[3 * pix + 1] = o.q.y; out_q[3 * pix + 2] = o.q.z; }
}

// the epilogue of an accumulation whose pixels hold different sample counts (adaptive + spectral): the kernel above over the row-major
// w x h rectangle with the pixel's own count in the place of the total.  A pixel that holds no sample (n_p == 0: a pixel of another
// rank) has +0 sums and is normalised by 1: the 0 * inf of 1 / 0 never forms.
__global__ __launch_bounds__(256) void develop_srgb_counts_kernel(const DevelopSrgbCountsParams P) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)P.w * P.h) return;
    const uint32_t y = (uint32_t)(pix / P.w), x = (uint32_t)(pix - (size_t)y * P.w);
    const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
    const uint32_t n_p = P.counts[idx] & ~kAdaptConverged;
    const float inv = 1.0f / (float)(n_p ? n_p : 1u);
    const SrgbPixel o = xyz_mean_to_srgb(mk(inv * P.xyz[3 * pix + 0], inv * P.xyz[3 * pix + 1], inv * P.xyz[3 * pix + 2]));
    if (P.out_lin) { P.out_lin[3 * pix + 0] = o.lin.x; P.out_lin[3 * pix + 1] = o.lin.y; P.out_lin[3 * pix + 2] = o.lin.z; }
    if (P.out_q) { P.out_q[3 * pix + 0] = o.q.x; P.out_q[3 * pix + 1] = o.q.y; P.out_q[3 * pix + 2] = o.q.z; }
}

}  // namespace

uint32_t develop_padded_channels(uint32_t channels) {
    for (const uint32_t kc : {1u, 2u, 3u, 4u, 8u, 16u})
        if (channels <= kc) return kc;
    return 0;
}

hipError_t launch_develop(const DevelopParams &p, hipStream_t st) {
    if (p.channels == 0 || p.channels > kMaxDevelopChannels || p.n_lanes > 0x7fffffffu || p.tx == 0 || p.ty == 0 || p.bx == 0) return hipErrorInvalidValue;
    if (p.n_lanes == 0 || p.w == 0 || p.h == 0) return hipSuccess;
    const dim3 grid((p.n_lanes + kDevTilePixels - 1u) / kDevTilePixels), block(kDevTilePixels);
    switch (develop_padded_channels(p.channels)) {
    case 1: hipLaunchKernelGGL(develop_kernel<1>, grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL(develop_kernel<2>, grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL(develop_kernel<3>, grid, block, 0, st, p); break;
    case 4: hipLaunchKernelGGL(develop_kernel<4>, grid, block, 0, st, p); break;
    case 8: hipLaunchKernelGGL(develop_kernel<8>, grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL(develop_kernel<16>, grid, block, 0, st, p); break;
    }
    return hipGetLastError();
}

hipError_t launch_develop_srgb(const float *xyz, float *out_lin, float *out_q, uint32_t samples, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(develop_srgb_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, xyz, out_lin, out_q, samples, n);
    return hipGetLastError();
}

hipError_t launch_develop_srgb_counts(const DevelopSrgbCountsParams &p, hipStream_t st) {
    const size_t n = (size_t)p.w * p.h;
    if (n == 0) return hipSuccess;
    if (!p.counts || p.tx == 0 || p.ty == 0 || p.bx == 0 || (n + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(develop_srgb_counts_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace srt
