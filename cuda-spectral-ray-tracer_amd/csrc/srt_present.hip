// srt_present.hip -- the end of the pipe on the device (srt_present / srt_present_kat; include/srt_c_api.h states every operation,
// tests/present_reference.py restates the packing in numpy): an XYZ picture through the tone curve and the usual conversion to sRGB into
// one packed RGBA8 word per pixel, the only thing of a presented picture that crosses the bus.
//
// A translation unit of its own, like the denoiser, the develop and the exposure: no existing kernel is touched and their machine code
// stays what it was.  Built with the exactness flags of the render unit (-ffp-contract=off, no fast-math): every product and quotient
// below is rounded once, in the order written -- tone_kernel's order (srt_expose.hip), so the bytes are its out_q, cast.
//
// Two kernels:
//   present_kernel            over the row-major w x h rectangle, one thread per group of four consecutive pixels of a row (columns
//                             4 g .. 4 g + 3).  The pixel's XYZ mean comes from the accumulation's three block-linear sum planes and the
//                             sample total or the pixel's own count (form a), or from a row-major [h][w][3] array (form b); times the
//                             gain, through the tone curve, through xyz_mean_to_srgb (srt_device.h); the three quantised channels -- whole
//                             numbers in 0 .. 255 always: a NaN channel fails every compare of correct_channel and comes out 255 -- and
//                             A = 255 are packed R | G << 8 | B << 16 | A << 24.
//                             A group that is whole (4 g + 4 <= w) and whose first pixel's row-major index is a multiple of four takes
//                             the vector path when the launcher found the bases 16-byte aligned (and, form a, tx and the plane stride
//                             multiples of four -- then the four pixels are four consecutive lanes of one block row): three 16-byte loads
//                             (form a: one per plane, and one of the state plane) and one 16-byte store.  At 12 B in and 4 B out per
//                             pixel the kernel is pure streaming: the wide accesses quarter the VMEM instructions per byte and a wave's
//                             store is 1 KiB contiguous.  Every other group -- the last columns of a width that is no multiple of four,
//                             rows that start off the 16-byte grid, misaligned bases -- walks its pixels one by one with 4-byte
//                             accesses.  Both paths run the same per-pixel function: the same bytes.
//                             The four columns of a group lie in one 8 x 8 tile, so ownership is decided once per group.  Blown /
//                             crushed / non-finite pixels of this rank's tiles are counted as tone_kernel counts them: a wave-level
//                             reduction, an LDS word per counter, one integer atomic per workgroup and counter (the grid is capped and
//                             grid-strided, so those atomics do not grow with the frame).
//   present_normalise_kernel  m = inv * D per component of a [h][w][3] array of developed sums, inv = 1.0f / (float)n with n the sample
//                             total or the pixel's own count (0 counts as 1): the mean develop_srgb_kernel / develop_srgb_counts_kernel
//                             form internally, materialised for the meter and for present_kernel's form b.
// No scratch, no LDS beyond the three counters, no float atomics, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kPresentThreads = 256;
constexpr uint32_t kPresentMaxBlocks = 4096;      // the grid's cap: at most this many workgroups add their counters

struct PresentCounts { uint32_t blown, crushed, nonfinite; };

// one pixel: XYZ mean -> packed word; tone_kernel's arithmetic, operation by operation
__device__ __forceinline__ uint32_t present_pixel(const PresentParams &P, V3 c, bool mine, PresentCounts &n) {
    const float cx = P.gain * c.x, cy = P.gain * c.y, cz = P.gain * c.z;
    V3 o = mk(cx, cy, cz);
    if (P.curve == 1u) {
        const float t = cy / P.kw;
        const float num = 1.0f + t;
        const float den = 1.0f + cy;
        float s = num / den;
        s = (cy > 0.0f) ? s : 1.0f;
        o = mk(s * cx, s * cy, s * cz);
    }
    const SrgbPixel srgb = xyz_mean_to_srgb(o);
    if (mine) {      // a pixel of another rank's tile is written (its sums are +0) and counted nowhere
        const bool finite = ((o.x - o.x) == 0.0f) & ((o.y - o.y) == 0.0f) & ((o.z - o.z) == 0.0f);
        n.nonfinite += finite ? 0u : 1u;
        n.blown += (srgb.q.x == 255.0f) | (srgb.q.y == 255.0f) | (srgb.q.z == 255.0f) ? 1u : 0u;
        n.crushed += (srgb.q.x == 0.0f) & (srgb.q.y == 0.0f) & (srgb.q.z == 0.0f) ? 1u : 0u;
    }
    return (uint32_t)srgb.q.x | ((uint32_t)srgb.q.y << 8) | ((uint32_t)srgb.q.z << 16) | 0xff000000u;
}

// the normalisation of a pixel's sums: tone_kernel's
__device__ __forceinline__ float present_inv(const PresentParams &P, uint32_t state_word) {
    uint32_t ns = P.samples;
    if (P.state) { ns = state_word & ~kAdaptConverged; ns = ns ? ns : 1u; }
    return 1.0f / (float)ns;
}

__global__ __launch_bounds__(kPresentThreads) void present_kernel(const PresentParams P) {
    __shared__ uint32_t wg_counts[3];
    if (threadIdx.x < 3u) wg_counts[threadIdx.x] = 0u;
    __syncthreads();
    PresentCounts n = {0u, 0u, 0u};      // (a thread sees fewer than 2^32 pixels)
    const uint32_t per_row = (P.w + 3u) / 4u;
    const uint32_t groups = per_row * P.h;      // (the launcher: below 2^31)
    const uint32_t stride = gridDim.x * kPresentThreads;
    for (uint32_t q = blockIdx.x * kPresentThreads + threadIdx.x; q < groups; q += stride) {      // (q < 2^31 + 2^20: no wrap)
        const uint32_t y = q / per_row, x0 = (q - y * per_row) * 4u;
        const size_t pix0 = (size_t)y * P.w + x0;
        const uint32_t tile = (y >> 3) * P.tiles_x + (x0 >> 3);      // x0 is a multiple of four: the group's columns share the tile
        const bool mine = tile % P.world == P.rank;
        if (P.vec && x0 + 4u <= P.w && (pix0 & 3u) == 0u) {
            V3 c[4];
            if (P.sums) {
                const size_t idx = block_linear_idx(x0, y, P.tx, P.ty, P.bx);      // tx is a multiple of four: lanes idx .. idx + 3 are the group
                const float4 X = *reinterpret_cast<const float4 *>(P.sums + idx);
                const float4 Y = *reinterpret_cast<const float4 *>(P.sums + idx + P.comp_stride);
                const float4 Z = *reinterpret_cast<const float4 *>(P.sums + idx + 2 * P.comp_stride);
                const uint4 s = P.state ? *reinterpret_cast<const uint4 *>(P.state + idx) : make_uint4(0u, 0u, 0u, 0u);
                const float i0 = present_inv(P, s.x), i1 = present_inv(P, s.y), i2 = present_inv(P, s.z), i3 = present_inv(P, s.w);
                c[0] = mk(i0 * X.x, i0 * Y.x, i0 * Z.x);
                c[1] = mk(i1 * X.y, i1 * Y.y, i1 * Z.y);
                c[2] = mk(i2 * X.z, i2 * Y.z, i2 * Z.z);
                c[3] = mk(i3 * X.w, i3 * Y.w, i3 * Z.w);
            } else {
                const float4 *src = reinterpret_cast<const float4 *>(P.xyz + 3 * pix0);      // 48 bytes: four pixels of three floats
                const float4 a = src[0], b = src[1], d = src[2];
                c[0] = mk(a.x, a.y, a.z);
                c[1] = mk(a.w, b.x, b.y);
                c[2] = mk(b.z, b.w, d.x);
                c[3] = mk(d.y, d.z, d.w);
            }
            uint4 o;
            o.x = present_pixel(P, c[0], mine, n);
            o.y = present_pixel(P, c[1], mine, n);
            o.z = present_pixel(P, c[2], mine, n);
            o.w = present_pixel(P, c[3], mine, n);
            *reinterpret_cast<uint4 *>(P.out + pix0) = o;
        } else {
            const uint32_t count = min(4u, P.w - x0);
            for (uint32_t e = 0; e < count; e++) {
                const size_t pix = pix0 + e;
                V3 c;
                if (P.sums) {
                    const size_t idx = block_linear_idx(x0 + e, y, P.tx, P.ty, P.bx);
                    const float inv = present_inv(P, P.state ? P.state[idx] : 0u);
                    c = mk(inv * P.sums[idx], inv * P.sums[idx + P.comp_stride], inv * P.sums[idx + 2 * P.comp_stride]);
                } else {
                    c = mk(P.xyz[3 * pix + 0], P.xyz[3 * pix + 1], P.xyz[3 * pix + 2]);
                }
                P.out[pix] = present_pixel(P, c, mine, n);
            }
        }
    }
    // the workgroup's three counters: every wave adds its lanes' sum to the LDS word, one thread per counter adds the word to global memory
    const uint32_t a = wave_sum(n.blown), b = wave_sum(n.crushed), d = wave_sum(n.nonfinite);
    if ((threadIdx.x & 63u) == 0u) {
        if (a) atomicAdd(&wg_counts[0], a);
        if (b) atomicAdd(&wg_counts[1], b);
        if (d) atomicAdd(&wg_counts[2], d);
    }
    __syncthreads();
    if (threadIdx.x < 3u && wg_counts[threadIdx.x]) atomicAdd(&P.counts[threadIdx.x], (unsigned long long)wg_counts[threadIdx.x]);
}

__global__ __launch_bounds__(256) void present_normalise_kernel(const PresentNormaliseParams P) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (size_t)P.w * P.h) return;
    uint32_t ns = P.samples;
    if (P.counts) {
        const uint32_t y = (uint32_t)(pix / P.w), x = (uint32_t)(pix - (size_t)y * P.w);
        ns = P.counts[block_linear_idx(x, y, P.tx, P.ty, P.bx)] & ~kAdaptConverged;
        ns = ns ? ns : 1u;
    }
    const float inv = 1.0f / (float)ns;
    P.mean[3 * pix + 0] = inv * P.developed[3 * pix + 0];
    P.mean[3 * pix + 1] = inv * P.developed[3 * pix + 1];
    P.mean[3 * pix + 2] = inv * P.developed[3 * pix + 2];
}

}  // namespace

hipError_t launch_present(const PresentParams &p, uint32_t n_cu, bool allow_vector, hipStream_t st) {
    if (p.w == 0 || p.h == 0) return hipSuccess;
    if ((!p.sums && !p.xyz) || !p.out || !p.counts || p.world == 0 || p.rank >= p.world || p.tiles_x == 0) return hipErrorInvalidValue;
    if (p.sums && (p.tx == 0 || p.ty == 0 || p.bx == 0)) return hipErrorInvalidValue;
    const uint64_t groups = (uint64_t)((p.w + 3u) / 4u) * p.h;
    if (groups > 0x7fffffffull) return hipErrorInvalidValue;
    // the vector path: every 16-byte access of a whole, aligned group lands on the 16-byte grid
    auto aligned = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    PresentParams k = p;
    k.vec = allow_vector && aligned(p.out) && (p.sums ? aligned(p.sums) && aligned(p.state) && p.tx % 4u == 0 && p.comp_stride % 4u == 0 : aligned(p.xyz)) ? 1u : 0u;
    const uint64_t cap = std::min<uint64_t>(kPresentMaxBlocks, (uint64_t)std::max<uint32_t>(n_cu, 1u) * 16u);
    hipLaunchKernelGGL(present_kernel, dim3((uint32_t)std::min((groups + kPresentThreads - 1) / kPresentThreads, cap)), dim3(kPresentThreads), 0, st, k);
    return hipGetLastError();
}

hipError_t launch_present_normalise(const PresentNormaliseParams &p, hipStream_t st) {
    const size_t n = (size_t)p.w * p.h;
    if (n == 0) return hipSuccess;
    if (!p.developed || !p.mean || (p.counts && (p.tx == 0 || p.ty == 0 || p.bx == 0))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(present_normalise_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace srt
