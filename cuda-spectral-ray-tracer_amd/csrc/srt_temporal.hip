// srt_temporal.hip -- temporal reprojection: the picture carried across camera moves (srt_temporal_accum / srt_temporal_kat /
// srt_denoise_features_temporal / srt_present_temporal; include/srt_c_api.h states every operation at srt_temporal_accum,
// tests/temporal_reference.py restates them in numpy).
//
// A translation unit of its own, like the firefly filter's: no render, denoise, develop, expose, present or despeckle kernel is touched and
// their machine code stays what it was.  Built with the exactness flags of the render unit (-ffp-contract=off, no fast-math, correctly
// rounded division and square root): every product, quotient and root below is rounded once, in the order written, so the restatement
// predicts the device's bits.
//
// One kernel, temporal_kernel<SRC> (two load paths, each static or moving): a 256-lane workgroup handles a 32 x 8 tile of the row-major w x h rectangle, one pixel per lane.  A
// wave owns a 16 x 4 sub-tile (lane l at (l & 15, l >> 4)), so that under a small camera move the wave's twelve 16-byte gathers -- four
// taps of three float4 history images -- fall on about five neighbouring rows of three 128-byte lines each, whichever way the picture moves.
//   Arithmetic. temporal_pixel() holds everything from the centre ray to (o, len', motion, class); both load paths call it.
//   Load paths (SRC): the denoiser's float4 colour image, whose fourth word is carried through (Quads); a row-major [h][w][3] array
//              (Rows).  The guides are two float4 per pixel and the history three, on either path.
//   Counters.  blended, fresh, offscreen, rejected, nonfinite: summed over a wave, then over the workgroup in LDS, then one integer atomic
//              per workgroup and non-zero counter, as the tone kernel counts.
//   Moments (bit 2 of SRC; srt_*_temporal_vg, stated in srt_c_api.h at "Variance measured across frames", restated in
//              tests/temporal_vg_reference.py): a fourth float4 history image (m1, m2, mlen, 0) rides on the taps the colour takes -- four
//              more 16-byte gathers on the same lines pattern -- and is blended as the colour is, with its own length.
// A second, elementwise kernel, temporal_variance_kernel, chooses per pixel between the variance the moments measure and the spatial estimate.
// No scratch, no float atomics, no inline assembly; LDS holds the five counters only (the choice kernel's: its one).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kTpTileW = 32, kTpTileH = 8, kTpThreads = kTpTileW * kTpTileH;
constexpr uint32_t kTpCounters = 5;
constexpr float kTpNaN = __builtin_nanf("");

// bit 1 of SRC: the moving variant (srt_temporal_*_moving), which projects the tracked point P.prev_point[p] of a hit pixel.  The flag
// rides in SRC so that the two static instantiations keep their symbols, and with them a by-symbol comparison of their machine code.
// bit 2 of SRC: the moments variant (srt_*_temporal_vg), which carries (m1, m2, mlen) through the colour's taps; the same reasoning.
enum TemporalSource { Quads = 0, Rows = 1, QuadsMoving = 2, RowsMoving = 3, Moments = 4 };

__device__ __forceinline__ V3 ld3(const float (&a)[3]) { return mk(a[0], a[1], a[2]); }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return ((x - x) == 0.0f) & ((y - y) == 0.0f) & ((z - z) == 0.0f); }

struct TemporalOut {
    V3 o;
    float len, mu, mv;
    uint32_t blended, fresh, offscreen, rejected, nonfinite;
    float4 hm;      // (MOMENTS only) the new moments Hm'
};

// The stage of pixel (x, y) with XYZ mean c and guides g0 = (N, z), g1 = (A, coverage), as srt_c_api.h states it: class, centre ray, point
// or direction, projection into the previous camera, bilinear gather with the acceptance tests, the result classes in their order.
// MOVING: step 3 of a hit pixel reads M = P.prev_point[p] -- M.w == 1: v = M.xyz - center'; otherwise step 4 counts as failed.
// MOMENTS: every tap the colour takes also gathers P.hist_m (when there is one) with the colour's weight; r.hm is Hm'.
template <bool MOVING, bool MOMENTS = false>
__device__ __forceinline__ TemporalOut temporal_pixel(const TemporalParams &P, uint32_t x, uint32_t y, V3 c, float4 g0, float4 g1) {
    TemporalOut r;
    r.o = c; r.len = 1.0f; r.mu = kTpNaN; r.mv = kTpNaN;
    r.blended = 0u; r.fresh = 0u; r.offscreen = 0u; r.rejected = 0u; r.nonfinite = 0u;
    const bool finite = finite3(c.x, c.y, c.z);
    bool projected = false, any_inside = false;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sl = 0.0f;
    float s1 = 0.0f, s2 = 0.0f, sm = 0.0f;      // (MOMENTS only)
    if (P.hist_c) {
        const bool hit = g1.w >= 0.5f;
        const float fi = (float)(P.ox + x), fj = (float)(P.oy + y);
        const V3 centre = ld3(P.center);
        const V3 pc = (ld3(P.p00) + fi * ld3(P.du)) + fj * ld3(P.dv);
        const V3 d = pc - centre;
        V3 v = d;
        float zexp = 0.0f;
        bool tracked = true;
        if (hit) {
            if constexpr (MOVING) {
                const float4 m = P.prev_point[(size_t)y * P.w + x];
                tracked = m.w == 1.0f;
                v = mk(m.x, m.y, m.z) - ld3(P.pcenter);
                zexp = sqrtf(dot(v, v));
            } else {
                const float L = sqrtf(dot(d, d));
                const float s = g0.w / L;
                const V3 pt = centre + s * d;
                v = pt - ld3(P.pcenter);
                zexp = sqrtf(dot(v, v));
            }
        }
        const V3 pn = ld3(P.pn), pe = ld3(P.pe);
        const float den = dot(v, pn);
        const float t = P.pk / den;
        projected = MOVING ? (t > 0.0f) & tracked : t > 0.0f;
        if (projected) {
            const V3 q = t * v - pe;
            const float u = dot(q, ld3(P.pbu)) - (float)P.ox;
            const float w = dot(q, ld3(P.pbv)) - (float)P.oy;
            r.mu = u - (float)x; r.mv = w - (float)y;
            const float x0 = floorf(u), y0 = floorf(w);
            const float fx = u - x0, fy = w - y0;
            const float fw = (float)P.w, fh = (float)P.h;
#pragma unroll
            for (int tap = 0; tap < 4; tap++) {      // (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
                const int a = tap & 1, b = tap >> 1;
                const float tx = a ? x0 + 1.0f : x0, ty = b ? y0 + 1.0f : y0;
                const float wx = a ? fx : 1.0f - fx, wy = b ? fy : 1.0f - fy;
                const float wt = wx * wy;
                // the test in float: a huge or NaN coordinate fails it and never reaches the conversion
                const bool inside = (tx >= 0.0f) & (tx < fw) & (ty >= 0.0f) & (ty < fh);
                any_inside |= inside;
                if (inside) {
                    const size_t qpix = (size_t)(uint32_t)ty * P.w + (uint32_t)tx;
                    const float4 hc = P.hist_c[qpix], h0 = P.hist_g[2 * qpix + 0], h1 = P.hist_g[2 * qpix + 1];
                    float4 hm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if constexpr (MOMENTS) if (P.hist_m) hm = P.hist_m[qpix];
                    bool ok = (hc.w > 0.0f) & finite3(hc.x, hc.y, hc.z) & ((h1.w >= 0.5f) == hit);
                    if (hit) {
                        const float nx = g0.x - h0.x, ny = g0.y - h0.y, nz = g0.z - h0.z;
                        const float dn = nx * nx + ny * ny + nz * nz;
                        const float ax = g1.x - h1.x, ay = g1.y - h1.y, az = g1.z - h1.z;
                        const float da = ax * ax + ay * ay + az * az;
                        const float zq = h0.w;
                        const float m = (zexp > zq) ? zexp : zq;
                        const float rr = (m > 0.0f) ? (zexp - zq) / m : 0.0f;
                        ok = ok & (dn <= P.kn) & (da <= P.ka) & (rr * rr <= P.kz);
                    }
                    if (ok & (wt > 0.0f)) {
                        sw += wt;
                        sx += wt * hc.x; sy += wt * hc.y; sz += wt * hc.z;
                        sl += wt * hc.w;
                        if constexpr (MOMENTS) if (P.hist_m) { s1 += wt * hm.x; s2 += wt * hm.y; sm += wt * hm.z; }
                    }
                }
            }
        }
    }
    const float Y = c.y, Q = Y * Y;
    if constexpr (MOMENTS) r.hm = make_float4(Y, Q, 1.0f, 0.0f);      // fresh, or blended with no moments history
    if (!finite) {
        r.len = 0.0f; r.nonfinite = 1u;
        if constexpr (MOMENTS) r.hm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else if (!(sw > 0.0f)) {
        r.fresh = 1u;
        if (P.hist_c) {
            const bool off = !projected | !any_inside;
            r.offscreen = off ? 1u : 0u; r.rejected = off ? 0u : 1u;
        }
    } else {
        const float hx = sx / sw, hy = sy / sw, hz = sz / sw, lh = sl / sw;
        float len = lh + 1.0f;
        len = (len < P.max_len) ? len : P.max_len;
        float a = 1.0f / len;
        a = (a > P.alpha_min) ? a : P.alpha_min;
        const bool keep = a >= 1.0f;
        r.o = keep ? c : mk(hx + a * (c.x - hx), hy + a * (c.y - hy), hz + a * (c.z - hz));
        r.len = len; r.blended = 1u;
        if constexpr (MOMENTS) {
            if (P.hist_m) {
                const float g1 = s1 / sw, g2 = s2 / sw, lm = sm / sw;
                float ml = lm + 1.0f;
                ml = (ml < P.max_len) ? ml : P.max_len;
                float b = 1.0f / ml;
                b = (b > P.alpha_min) ? b : P.alpha_min;
                const bool keep_m = b >= 1.0f;
                r.hm = make_float4(keep_m ? Y : g1 + b * (Y - g1), keep_m ? Q : g2 + b * (Q - g2), ml, 0.0f);
            }
        }
    }
    return r;
}

template <int SRC>
__global__ __launch_bounds__(kTpThreads) void temporal_kernel(const TemporalParams P) {
    __shared__ uint32_t wg_counts[kTpCounters];
    const uint32_t tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
    if (threadIdx.x < kTpCounters) wg_counts[threadIdx.x] = 0u;
    __syncthreads();
    // wave wv owns the 16 x 4 sub-tile at (16 (wv & 1), 4 (wv >> 1)) of the 32 x 8 tile
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t x = tile_x * kTpTileW + 16u * (wv & 1u) + (lane & 15u), y = tile_y * kTpTileH + 4u * (wv >> 1) + (lane >> 4);
    uint32_t n[kTpCounters] = {0u, 0u, 0u, 0u, 0u};
    if (x < P.w && y < P.h) {
        const size_t pix = (size_t)y * P.w + x;
        V3 c;
        float w4 = 0.0f;
        if constexpr ((SRC & 1) == Quads) {
            const float4 v = P.src4[pix];
            c = mk(v.x, v.y, v.z); w4 = v.w;
        } else {
            c = mk(P.xyz[3 * pix + 0], P.xyz[3 * pix + 1], P.xyz[3 * pix + 2]);
        }
        const float4 g0 = P.guides[2 * pix + 0], g1 = P.guides[2 * pix + 1];
        const TemporalOut r = temporal_pixel<(SRC & 2) != 0, (SRC & Moments) != 0>(P, x, y, c, g0, g1);
        n[0] = r.blended; n[1] = r.fresh; n[2] = r.offscreen; n[3] = r.rejected; n[4] = r.nonfinite;
        P.new_c[pix] = make_float4(r.o.x, r.o.y, r.o.z, r.len);
        P.new_g[2 * pix + 0] = g0; P.new_g[2 * pix + 1] = g1;
        if constexpr ((SRC & Moments) != 0) P.new_m[pix] = r.hm;
        if (P.dst4) P.dst4[pix] = make_float4(r.o.x, r.o.y, r.o.z, w4);
        if (P.out_xyz) { P.out_xyz[3 * pix + 0] = r.o.x; P.out_xyz[3 * pix + 1] = r.o.y; P.out_xyz[3 * pix + 2] = r.o.z; }
        if (P.out_len) P.out_len[pix] = r.len;
        if (P.out_motion) { P.out_motion[2 * pix + 0] = r.mu; P.out_motion[2 * pix + 1] = r.mv; }
        if (P.out_lin || P.out_q) {
            const SrgbPixel srgb = xyz_mean_to_srgb(r.o);
            if (P.out_lin) { P.out_lin[3 * pix + 0] = srgb.lin.x; P.out_lin[3 * pix + 1] = srgb.lin.y; P.out_lin[3 * pix + 2] = srgb.lin.z; }
            if (P.out_q) { P.out_q[3 * pix + 0] = srgb.q.x; P.out_q[3 * pix + 1] = srgb.q.y; P.out_q[3 * pix + 2] = srgb.q.z; }
        }
    }
    // every lane of the workgroup arrives here: a wave-level sum, the workgroup's word in LDS, one atomic per counter
#pragma unroll
    for (uint32_t k = 0; k < kTpCounters; k++) {
        const uint32_t s = wave_sum(n[k]);
        if (lane == 0u && s) atomicAdd(&wg_counts[k], s);
    }
    __syncthreads();
    if (threadIdx.x < kTpCounters && wg_counts[threadIdx.x]) atomicAdd(&P.counts[threadIdx.x], (unsigned long long)wg_counts[threadIdx.x]);
}

// The choice of the variance (srt_c_api.h, srt_denoise_features_temporal_vg): elementwise, one pixel per lane; the pixels that take the
// temporal variance are counted as the stage counts -- a wave sum, the workgroup's word in LDS, one integer atomic per workgroup.
__global__ __launch_bounds__(kTpThreads) void temporal_variance_kernel(const TemporalVarianceParams P) {
    __shared__ uint32_t wg_count;
    if (threadIdx.x == 0u) wg_count = 0u;
    __syncthreads();
    const uint32_t p = blockIdx.x * kTpThreads + threadIdx.x;
    uint32_t used = 0u;
    if (p < P.n) {
        const float4 hm = P.moments[p];
        const float len = P.len[(size_t)P.len_stride * p], vs = P.spatial[(size_t)P.spatial_stride * p];
        float d = hm.y - hm.x * hm.x;
        d = (d > 0.0f) ? d : 0.0f;
        const float vt = d / len;
        const bool use = (hm.z >= P.ml_min) & (len > 0.0f) & ((vt - vt) == 0.0f);
        const float v = use ? vt : vs;
        used = use ? 1u : 0u;
        if (P.colour_w) P.colour_w[(size_t)4 * p] = v;
        P.out_var[(size_t)P.out_stride * p] = v;
    }
    const uint32_t s = wave_sum(used);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(&wg_count, s);
    __syncthreads();
    if (threadIdx.x == 0u && wg_count) atomicAdd(P.count, (unsigned long long)wg_count);
}

}  // namespace

hipError_t launch_temporal_variance(const TemporalVarianceParams &p, hipStream_t st) {
    if (p.n == 0) return hipSuccess;
    if (!p.moments || !p.len || !p.spatial || !p.out_var || !p.count || p.n > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(temporal_variance_kernel, dim3((p.n + kTpThreads - 1u) / kTpThreads), dim3(kTpThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_temporal(const TemporalParams &p_in, hipStream_t st) {
    TemporalParams p = p_in;
    if (p.w == 0 || p.h == 0) return hipSuccess;
    if ((p.xyz != nullptr) + (p.src4 != nullptr) != 1 || !p.guides || !p.new_c || !p.new_g || !p.counts) return hipErrorInvalidValue;
    if ((p.hist_c != nullptr) != (p.hist_g != nullptr)) return hipErrorInvalidValue;
    // (the history is read at other pixels than the one written: never in place)
    if (p.hist_c && (p.hist_c == p.new_c || p.hist_g == p.new_g)) return hipErrorInvalidValue;
    // (a moments history needs a colour history, whose taps it rides on, and somewhere else to go)
    if (p.hist_m && (!p.new_m || !p.hist_c || p.hist_m == p.new_m)) return hipErrorInvalidValue;
    p.tiles_x = (p.w + kTpTileW - 1u) / kTpTileW;
    const uint64_t blocks = (uint64_t)p.tiles_x * ((p.h + kTpTileH - 1u) / kTpTileH);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (p.new_m) {
        const dim3 grid((uint32_t)blocks), block(kTpThreads);
        if (p.prev_point && p.src4) hipLaunchKernelGGL((temporal_kernel<QuadsMoving | Moments>), grid, block, 0, st, p);
        else if (p.prev_point) hipLaunchKernelGGL((temporal_kernel<RowsMoving | Moments>), grid, block, 0, st, p);
        else if (p.src4) hipLaunchKernelGGL((temporal_kernel<Quads | Moments>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((temporal_kernel<Rows | Moments>), grid, block, 0, st, p);
    } else if (p.prev_point && p.src4) hipLaunchKernelGGL((temporal_kernel<QuadsMoving>), dim3((uint32_t)blocks), dim3(kTpThreads), 0, st, p);
    else if (p.prev_point) hipLaunchKernelGGL((temporal_kernel<RowsMoving>), dim3((uint32_t)blocks), dim3(kTpThreads), 0, st, p);
    else if (p.src4) hipLaunchKernelGGL((temporal_kernel<Quads>), dim3((uint32_t)blocks), dim3(kTpThreads), 0, st, p);
    else hipLaunchKernelGGL((temporal_kernel<Rows>), dim3((uint32_t)blocks), dim3(kTpThreads), 0, st, p);
    return hipGetLastError();
}

}  // namespace srt
