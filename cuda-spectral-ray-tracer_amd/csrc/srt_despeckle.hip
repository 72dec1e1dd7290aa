// srt_despeckle.hip -- the firefly filter: a rank-based outlier clamp on the XYZ mean, ahead of the denoiser (srt_despeckle_accum /
// srt_despeckle_kat / srt_denoise_features_ds / srt_present_despeckled; include/srt_c_api.h states every operation at srt_despeckle_accum,
// tests/despeckle_reference.py restates them in numpy).
//
// A translation unit of its own, like the exposure's: no render, denoise, develop, expose or present kernel is touched and their machine
// code stays what it was.  Built with the exactness flags of the render unit (-ffp-contract=off, no fast-math, correctly rounded
// division): every product and quotient below is rounded once, in the order written, so the restatement predicts the device's bits.
//
// One kernel, despeckle_kernel<R, SRC>: a 256-lane workgroup filters a 32 x 8 tile of the row-major w x h rectangle, one pixel per lane.
//   Staging.   The workgroup writes the canonical luminance v_q of every pixel of the tile and of a halo of R pixels around it to LDS
//              once ((32 + 2 R) x (8 + 2 R) words: 1.7 KiB at R = 2) -- +inf for a tap outside the rectangle or a non-finite one.  A valid
//              value is never +inf, so a window's m is its count of entries below +inf.
//   Selection. A lane takes the 8 (R = 1) or 24 (R = 2) values of its window into registers and sorts them ascending with a fixed
//              compare-exchange network (Batcher's odd-even merge sort for N wires, every index a compile-time constant: no private array
//              is indexed dynamically, scratch is 0); the +inf of the missing taps sort to the end, so u_k is wire k of the network for
//              every k < m, picked with a select chain.  v_min_f32 / v_max_f32 are exact here: the values hold no NaN and no -0, equal
//              values have equal bits, and f32 denormals are kept.
//   Arithmetic. despeckle_pixel() holds everything from the window to (o, s); all three load paths call it.
//   Load paths (SRC): an accumulation's block-linear sum planes with the sample total or the pixel's own count (Sums); a row-major
//              [h][w][3] array (Rows); the denoiser's row-major float4 colour image, whose fourth word is carried through (Quads).
//   Counters.  clamped, nonfinite, alone: summed over a wave, then over the workgroup in LDS, then one integer atomic per workgroup and
//              non-zero counter, as the tone kernel counts.
// No scratch, no float atomics, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kDsTileW = 32, kDsTileH = 8, kDsThreads = kDsTileW * kDsTileH;
constexpr float kDsInf = __builtin_huge_valf();

enum DespeckleSource { Sums = 0, Rows = 1, Quads = 2 };

__device__ __forceinline__ void compare_exchange(float &a, float &b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo; b = hi;
}

// Batcher's odd-even merge sort on N wires, ascending; every loop bound is a compile-time constant and every loop is unrolled, so u[] lives
// in registers.  (The network of the next power of two with the wires >= N removed: they would hold +inf and their comparators do nothing.)
template <int N>
__device__ __forceinline__ void sort_network(float (&u)[N]) {
#pragma unroll
    for (int p = 1; p < N; p *= 2) {
#pragma unroll
        for (int k = p; k >= 1; k /= 2) {
#pragma unroll
            for (int j = k % p; j <= N - 1 - k; j += 2 * k) {
#pragma unroll
                for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); i++) {
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) compare_exchange(u[i + j], u[i + j + k]);
                }
            }
        }
    }
}

struct DespeckleOut { V3 o; float s; uint32_t clamped, nonfinite, alone; };

// The filter of one pixel with XYZ mean c from the N values of its window (canonical luminances, +inf for a missing tap), as srt_c_api.h
// states it: m, the rank k, ref = u_k, limit = gain * ref + floor, the four classes in their order.
template <int N>
__device__ __forceinline__ DespeckleOut despeckle_pixel(float (&u)[N], V3 c, uint32_t rank_ppm, float gain, float floor) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < N; i++) m += u[i] < kDsInf ? 1u : 0u;
    sort_network<N>(u);
    // (m - 1) * rank_ppm <= 23 * 1000000 < 2^32: the 64-bit quotient of the statement, in 32 bits
    const uint32_t k = ((m ? m - 1u : 0u) * rank_ppm) / 1000000u;
    float ref = u[0];
#pragma unroll
    for (int i = 1; i < N; i++) ref = (k == (uint32_t)i) ? u[i] : ref;
    float limit = gain * ref;
    limit = limit + floor;
    const bool finite = ((c.x - c.x) == 0.0f) & ((c.y - c.y) == 0.0f) & ((c.z - c.z) == 0.0f);
    const bool alone = finite & (m == 0u);
    const bool clamp = finite & (m != 0u) & (c.y > limit);
    float s = limit / c.y;
    s = clamp ? s : 1.0f;
    DespeckleOut r;
    r.o = clamp ? mk(s * c.x, s * c.y, s * c.z) : c;
    r.s = s;
    r.clamped = clamp ? 1u : 0u; r.nonfinite = finite ? 0u : 1u; r.alone = alone ? 1u : 0u;
    return r;
}

// the XYZ mean of pixel (x, y) of the rectangle, and (Quads) the fourth word of its float4
template <int SRC>
__device__ __forceinline__ V3 despeckle_mean(const DespeckleParams &P, uint32_t x, uint32_t y, float &w4) {
    const size_t pix = (size_t)y * P.w + x;
    w4 = 0.0f;
    if constexpr (SRC == Sums) {
        const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
        uint32_t ns = P.samples;
        if (P.state) { ns = P.state[idx] & ~kAdaptConverged; ns = ns ? ns : 1u; }
        const float inv = 1.0f / (float)ns;
        return mk(inv * P.sums[idx], inv * P.sums[idx + P.comp_stride], inv * P.sums[idx + 2 * P.comp_stride]);
    } else if constexpr (SRC == Rows) {
        return mk(P.xyz[3 * pix + 0], P.xyz[3 * pix + 1], P.xyz[3 * pix + 2]);
    } else {
        const float4 v = P.src4[pix];
        w4 = v.w;
        return mk(v.x, v.y, v.z);
    }
}

// the luminance of pixel (x, y) alone: what the staging reads of a neighbour
template <int SRC>
__device__ __forceinline__ float despeckle_luminance(const DespeckleParams &P, uint32_t x, uint32_t y) {
    const size_t pix = (size_t)y * P.w + x;
    if constexpr (SRC == Sums) {
        const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
        uint32_t ns = P.samples;
        if (P.state) { ns = P.state[idx] & ~kAdaptConverged; ns = ns ? ns : 1u; }
        const float inv = 1.0f / (float)ns;
        return inv * P.sums[idx + P.comp_stride];
    } else if constexpr (SRC == Rows) {
        return P.xyz[3 * pix + 1];
    } else {
        return P.src4[pix].y;
    }
}

template <int R, int SRC>
__global__ __launch_bounds__(kDsThreads) void despeckle_kernel(const DespeckleParams P) {
    constexpr uint32_t LW = kDsTileW + 2 * R, LH = kDsTileH + 2 * R;
    constexpr int N = (2 * R + 1) * (2 * R + 1) - 1;
    __shared__ float lum[LH * LW];
    __shared__ uint32_t wg_counts[3];
    const uint32_t tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
    const uint32_t x0 = tile_x * kDsTileW, y0 = tile_y * kDsTileH;
    if (threadIdx.x < 3u) wg_counts[threadIdx.x] = 0u;
    for (uint32_t e = threadIdx.x; e < LH * LW; e += kDsThreads) {
        const uint32_t ly = e / LW, lx = e - ly * LW;
        // (x0 + lx - R wraps below zero for the left and top halo of the first tiles: the unsigned compare refuses it)
        const uint32_t gx = x0 + lx - (uint32_t)R, gy = y0 + ly - (uint32_t)R;
        float v = kDsInf;
        if (gx < P.w && gy < P.h) {
            const float Y = despeckle_luminance<SRC>(P, gx, gy);
            const bool valid = (Y - Y) == 0.0f;
            const float canon = Y > 0.0f ? Y : 0.0f;
            v = valid ? canon : kDsInf;
        }
        lum[e] = v;
    }
    __syncthreads();

    const uint32_t lx = threadIdx.x % kDsTileW, ly = threadIdx.x / kDsTileW;
    const uint32_t x = x0 + lx, y = y0 + ly;
    uint32_t clamped = 0, nonfinite = 0, alone = 0;
    if (x < P.w && y < P.h) {
        float u[N];
#pragma unroll
        for (int t = 0; t < N; t++) {      // the window's taps in row-major order, the centre (tap N / 2) left out
            const int tap = t < N / 2 ? t : t + 1, dy = tap / (2 * R + 1), dx = tap - dy * (2 * R + 1);
            u[t] = lum[(ly + (uint32_t)dy) * LW + lx + (uint32_t)dx];
        }
        float w4;
        const V3 c = despeckle_mean<SRC>(P, x, y, w4);
        const DespeckleOut r = despeckle_pixel<N>(u, c, P.rank_ppm, P.gain, P.floor);
        clamped = r.clamped; nonfinite = r.nonfinite; alone = r.alone;
        const size_t pix = (size_t)y * P.w + x;
        if (P.dst4) P.dst4[pix] = make_float4(r.o.x, r.o.y, r.o.z, w4);
        if (P.out_xyz) { P.out_xyz[3 * pix + 0] = r.o.x; P.out_xyz[3 * pix + 1] = r.o.y; P.out_xyz[3 * pix + 2] = r.o.z; }
        if (P.out_scale) P.out_scale[pix] = r.s;
        if (P.out_lin || P.out_q) {
            const SrgbPixel srgb = xyz_mean_to_srgb(r.o);
            if (P.out_lin) { P.out_lin[3 * pix + 0] = srgb.lin.x; P.out_lin[3 * pix + 1] = srgb.lin.y; P.out_lin[3 * pix + 2] = srgb.lin.z; }
            if (P.out_q) { P.out_q[3 * pix + 0] = srgb.q.x; P.out_q[3 * pix + 1] = srgb.q.y; P.out_q[3 * pix + 2] = srgb.q.z; }
        }
    }
    // every lane of the workgroup arrives here: a wave-level sum, the workgroup's word in LDS, one atomic per counter
    clamped = wave_sum(clamped); nonfinite = wave_sum(nonfinite); alone = wave_sum(alone);
    if ((threadIdx.x & 63u) == 0u) {
        if (clamped) atomicAdd(&wg_counts[0], clamped);
        if (nonfinite) atomicAdd(&wg_counts[1], nonfinite);
        if (alone) atomicAdd(&wg_counts[2], alone);
    }
    __syncthreads();
    if (threadIdx.x < 3u && wg_counts[threadIdx.x]) atomicAdd(&P.counts[threadIdx.x], (unsigned long long)wg_counts[threadIdx.x]);
}

template <int R>
void launch_radius(const DespeckleParams &p, uint32_t blocks, hipStream_t st) {
    if (p.sums) hipLaunchKernelGGL((despeckle_kernel<R, Sums>), dim3(blocks), dim3(kDsThreads), 0, st, p);
    else if (p.xyz) hipLaunchKernelGGL((despeckle_kernel<R, Rows>), dim3(blocks), dim3(kDsThreads), 0, st, p);
    else hipLaunchKernelGGL((despeckle_kernel<R, Quads>), dim3(blocks), dim3(kDsThreads), 0, st, p);
}

}  // namespace

hipError_t launch_despeckle(const DespeckleParams &p_in, hipStream_t st) {
    DespeckleParams p = p_in;
    if (p.w == 0 || p.h == 0) return hipSuccess;
    if ((p.sums != nullptr) + (p.xyz != nullptr) + (p.src4 != nullptr) != 1 || !p.counts || (p.radius != 1u && p.radius != 2u) || p.rank_ppm > 1000000u)
        return hipErrorInvalidValue;
    if (p.sums && (p.tx == 0 || p.ty == 0 || p.bx == 0)) return hipErrorInvalidValue;
    if (p.dst4 && reinterpret_cast<const void *>(p.dst4) == reinterpret_cast<const void *>(p.src4)) return hipErrorInvalidValue;      // (neighbours are read: never in place)
    p.tiles_x = (p.w + kDsTileW - 1u) / kDsTileW;
    const uint64_t blocks = (uint64_t)p.tiles_x * ((p.h + kDsTileH - 1u) / kDsTileH);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (p.radius == 1u) launch_radius<1>(p, (uint32_t)blocks, st);
    else launch_radius<2>(p, (uint32_t)blocks, st);
    return hipGetLastError();
}

}  // namespace srt
