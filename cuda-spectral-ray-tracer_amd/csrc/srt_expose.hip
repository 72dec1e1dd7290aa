// srt_expose.hip -- exposure metering and tone mapping on the device (srt_meter_accum / srt_meter_kat / srt_expose_accum /
// srt_expose_kat; include/srt_c_api.h states every operation, tests/expose_reference.py restates them in numpy).
//
// A translation unit of its own, like the denoiser and the develop: no render, denoise or develop kernel is touched and their machine
// code stays what it was.  Built with the exactness flags of the render unit (-ffp-contract=off, no fast-math): every product and
// quotient below is rounded once, in the order written, so the restatement predicts the device's bits.
//
// Two kernels:
//   meter_kernel<V>       the luminance histogram of the metered rectangle.  It walks the block-linear lanes [0, n_lanes) of the Y plane
//                         (and, on an adaptive accumulation, of the state plane), V consecutive lanes per thread -- V = 4 reads them as
//                         one 16-byte load when the plane is contiguous and tx is a multiple of 4, so the four lanes are four pixels
//                         of one row and the inverse of block_linear_idx (three integer divisions) is paid once for them -- maps them
//                         to chunk pixels for the rectangle and ownership tests, classifies, and counts into a 4096-bin uint32
//                         histogram in LDS that is private to the workgroup (16 KiB: nine workgroups fit in a CU's 160 KiB).  The
//                         grid is capped and grid-strided: at the end a workgroup adds its non-zero bins to the global histogram
//                         with integer atomics (at most kMeterMaxBlocks x 4096 of them, whatever the frame) and its three counters,
//                         which its waves summed (a wave-level reduction, then LDS).  Integer counts: the result does not depend on
//                         the order.
//                         The hot bin -- a flat sky or a black frame sends every lane of a wave to one LDS address -- is left to
//                         plain LDS atomics: measured at 1080p against a wave-level aggregation of equal bins
//                         (profiles/expose/hot_bin.txt), they lose 5 % on a constant image and win 7 to 20 % on noise, the better
//                         worst case.
//   tone_kernel           elementwise over the row-major w x h rectangle: the pixel's XYZ mean (from the accumulation's three planes
//                         and the sample total or the pixel's own count, or from a row-major array), times the gain, through the tone
//                         curve, through xyz_mean_to_srgb (srt_device.h) -- the epilogue every other picture ends in -- and out to up
//                         to three row-major images; blown / crushed / non-finite pixels are counted with integer atomics after a
//                         wave-level reduction (the grid is capped and grid-strided, so those atomics do not grow with the frame).
// No scratch, no float atomics, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kMeterThreads = 256;
constexpr uint32_t kToneThreads = 256;
constexpr uint32_t kToneMaxBlocks = 4096;      // the grid's cap: at most this many workgroups add their counters
constexpr float kFltMin = 1.17549435e-38f;

// is chunk pixel (i, j) a pixel this rank meters: inside the rectangle, in a tile it owns
__device__ __forceinline__ bool metered_pixel(const MeterParams &P, uint32_t i, uint32_t j) {
    if (i < P.x0 || i - P.x0 >= P.w || j < P.y0 || j - P.y0 >= P.h) return false;
    const uint32_t t = (j >> 3) * P.tiles_x + (i >> 3);
    return t % P.world == P.rank;
}

// one pixel's luminance into the workgroup's histogram or one of the thread's counters
__device__ __forceinline__ void meter_count(uint32_t *hist, bool mine, float Y, uint32_t &n_metered, uint32_t &n_dark, uint32_t &n_nonfinite) {
    const bool finite = (Y - Y) == 0.0f;
    const bool bright = Y >= kFltMin;
    const bool metered = mine && finite && bright;
    n_nonfinite += (mine && !finite) ? 1u : 0u;
    n_dark += (mine && finite && !bright) ? 1u : 0u;
    n_metered += metered ? 1u : 0u;
    if (metered) atomicAdd(&hist[__float_as_uint(Y) >> 19], 1u);      // the bin: in [16, 4080)
}

// A workgroup's three counters: every wave adds its lanes' sum to the LDS word, and behind a barrier one thread per counter adds the word to
// global memory -- one integer atomic per workgroup and counter: thousands of waves adding to one address would queue up behind each other.
__device__ __forceinline__ void add_workgroup_counts(uint32_t *wg, uint32_t a, uint32_t b, uint32_t c) {
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if ((threadIdx.x & 63u) == 0u) {
        if (a) atomicAdd(&wg[0], a);
        if (b) atomicAdd(&wg[1], b);
        if (c) atomicAdd(&wg[2], c);
    }
}
__device__ __forceinline__ void flush_workgroup_counts(const uint32_t *wg, unsigned long long *counts) {
    if (threadIdx.x < 3u && wg[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)wg[threadIdx.x]);
}

template <int V>
__global__ __launch_bounds__(kMeterThreads) void meter_kernel(const MeterParams P) {
    __shared__ uint32_t hist[kMeterBins];
    __shared__ uint32_t wg_counts[3];
    for (uint32_t b = threadIdx.x; b < kMeterBins; b += kMeterThreads) hist[b] = 0u;
    if (threadIdx.x < 3u) wg_counts[threadIdx.x] = 0u;
    __syncthreads();

    uint32_t n_metered = 0, n_dark = 0, n_nonfinite = 0;
    const uint32_t groups = (P.n_lanes + (uint32_t)V - 1u) / (uint32_t)V;      // V = 4 only when n_lanes is a multiple of 4
    const uint32_t stride = gridDim.x * kMeterThreads;
    for (uint32_t q = blockIdx.x * kMeterThreads + threadIdx.x; q < groups; q += stride) {      // (q < 2^31 + 2^18: no wrap)
        const uint32_t idx = q * (uint32_t)V;
        const PixelIJ px = block_linear_pixel(idx, P.tx, P.ty, P.bx);
        float y[V];
        uint32_t st[V];
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(P.y + idx);
            y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
            const uint4 s = P.state ? *reinterpret_cast<const uint4 *>(P.state + idx) : make_uint4(0u, 0u, 0u, 0u);
            st[0] = s.x; st[1] = s.y; st[2] = s.z; st[3] = s.w;
        } else {
            y[0] = P.y[(size_t)idx * P.y_stride];
            st[0] = P.state ? P.state[idx] : 0u;
        }
#pragma unroll
        for (int e = 0; e < V; e++) {
            const bool mine = metered_pixel(P, px.i + (uint32_t)e, px.j);
            float Y = y[e];
            if (P.normalise) {
                uint32_t n = P.samples;
                if (P.state) { n = st[e] & ~kAdaptConverged; n = n ? n : 1u; }
                const float inv = 1.0f / (float)n;
                Y = inv * Y;
            }
            meter_count(hist, mine, Y, n_metered, n_dark, n_nonfinite);
        }
    }
    __syncthreads();

    for (uint32_t b = threadIdx.x; b < kMeterBins; b += kMeterThreads) {
        const uint32_t n = hist[b];
        if (n) atomicAdd(&P.hist[b], n);
    }
    add_workgroup_counts(wg_counts, n_metered, n_dark, n_nonfinite);
    __syncthreads();
    flush_workgroup_counts(wg_counts, P.counts);
}

__global__ __launch_bounds__(kToneThreads) void tone_kernel(const ToneParams P) {
    __shared__ uint32_t wg_counts[3];
    if (threadIdx.x < 3u) wg_counts[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t blown = 0, crushed = 0, nonfinite = 0;      // (a thread sees at most n / (grid x 256) < 2^32 pixels)
    const size_t n = (size_t)P.w * P.h, stride = (size_t)gridDim.x * kToneThreads;
    for (size_t pix = (size_t)blockIdx.x * kToneThreads + threadIdx.x; pix < n; pix += stride) {
        const uint32_t y = (uint32_t)(pix / P.w), x = (uint32_t)(pix - (size_t)y * P.w);
        V3 c;
        if (P.sums) {
            const size_t idx = block_linear_idx(x, y, P.tx, P.ty, P.bx);
            uint32_t ns = P.samples;
            if (P.state) { ns = P.state[idx] & ~kAdaptConverged; ns = ns ? ns : 1u; }
            const float inv = 1.0f / (float)ns;
            c = mk(inv * P.sums[idx], inv * P.sums[idx + P.comp_stride], inv * P.sums[idx + 2 * P.comp_stride]);
        } else {
            c = mk(P.xyz[3 * pix + 0], P.xyz[3 * pix + 1], P.xyz[3 * pix + 2]);
        }
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
        if (P.out_xyz) { P.out_xyz[3 * pix + 0] = o.x; P.out_xyz[3 * pix + 1] = o.y; P.out_xyz[3 * pix + 2] = o.z; }
        if (P.out_lin) { P.out_lin[3 * pix + 0] = srgb.lin.x; P.out_lin[3 * pix + 1] = srgb.lin.y; P.out_lin[3 * pix + 2] = srgb.lin.z; }
        if (P.out_q) { P.out_q[3 * pix + 0] = srgb.q.x; P.out_q[3 * pix + 1] = srgb.q.y; P.out_q[3 * pix + 2] = srgb.q.z; }
        const uint32_t tile = (y >> 3) * P.tiles_x + (x >> 3);
        if (tile % P.world == P.rank) {      // a pixel of another rank's tile is written (its sums are +0) and counted nowhere
            const bool finite = ((o.x - o.x) == 0.0f) & ((o.y - o.y) == 0.0f) & ((o.z - o.z) == 0.0f);
            nonfinite += finite ? 0u : 1u;
            blown += (srgb.q.x == 255.0f) | (srgb.q.y == 255.0f) | (srgb.q.z == 255.0f) ? 1u : 0u;
            crushed += (srgb.q.x == 0.0f) & (srgb.q.y == 0.0f) & (srgb.q.z == 0.0f) ? 1u : 0u;
        }
    }
    add_workgroup_counts(wg_counts, blown, crushed, nonfinite);
    __syncthreads();
    flush_workgroup_counts(wg_counts, P.counts);
}

}  // namespace

hipError_t launch_meter(const MeterParams &p, uint32_t n_cu, hipStream_t st) {
    if (p.n_lanes > 0x7fffffffu || p.tx == 0 || p.ty == 0 || p.bx == 0 || p.world == 0 || p.rank >= p.world || p.tiles_x == 0 || !p.y || !p.hist || !p.counts
        || p.y_stride == 0) return hipErrorInvalidValue;
    if (p.n_lanes == 0 || p.w == 0 || p.h == 0) return hipSuccess;
    // four lanes per thread where they are one 16-byte word of the plane and four pixels of one row
    const bool vec4 = p.y_stride == 1 && p.tx % 4u == 0 && p.n_lanes % 4u == 0 && (reinterpret_cast<uintptr_t>(p.y) & 15u) == 0
                      && (reinterpret_cast<uintptr_t>(p.state) & 15u) == 0;
    const uint32_t groups = vec4 ? p.n_lanes / 4u : p.n_lanes;
    const uint32_t want = (groups + kMeterThreads - 1u) / kMeterThreads;
    const uint32_t cap = std::min<uint32_t>(kMeterMaxBlocks, std::max<uint32_t>(n_cu, 1u) * 4u);
    const dim3 grid(std::min(want, cap)), block(kMeterThreads);
    if (vec4) hipLaunchKernelGGL(meter_kernel<4>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(meter_kernel<1>, grid, block, 0, st, p);
    return hipGetLastError();
}

hipError_t launch_tone(const ToneParams &p, uint32_t n_cu, hipStream_t st) {
    const size_t n = (size_t)p.w * p.h;
    if (n == 0) return hipSuccess;
    if ((!p.sums && !p.xyz) || !p.counts || p.world == 0 || p.rank >= p.world || p.tiles_x == 0) return hipErrorInvalidValue;
    if (p.sums && (p.tx == 0 || p.ty == 0 || p.bx == 0)) return hipErrorInvalidValue;
    const size_t cap = std::min<size_t>(kToneMaxBlocks, (size_t)std::max<uint32_t>(n_cu, 1u) * 16u);
    hipLaunchKernelGGL(tone_kernel, dim3((uint32_t)std::min((n + kToneThreads - 1) / kToneThreads, cap)), dim3(kToneThreads), 0, st, p);
    return hipGetLastError();
}

}  // namespace srt
