// srt_motion.hip -- the surface-motion pass: for every pixel the surface point its centre ray sees, moved back to where the same point of
// the same triangle lay when the temporal history was written (srt_surface_motion / srt_surface_motion_kat and the *_moving temporal
// calls; include/srt_c_api.h states every operation at srt_surface_motion, tests/surface_motion_reference.py restates them in numpy).
//
// A translation unit of its own, like the temporal stage's: no render, denoise, develop, expose, present, despeckle, temporal or refit
// kernel is touched and their machine code stays what it was.  Built with the exactness flags of the temporal unit (-ffp-contract=off, no
// fast-math, correctly rounded division and square root): every product and quotient below is rounded once, in the order written.
//
// One kernel, motion_kernel: a 256-lane workgroup handles a 32 x 8 tile of the row-major w x h rectangle, one pixel per lane; a wave owns a
// 16 x 4 sub-tile (lane l at (l & 15, l >> 4)) as temporal_kernel's does, so the centre rays of a wave are neighbours and walk the tree
// together.
//   Closest hit. trace_rays_kernel's query (srt_kernels.hip), the same traversal functions with the same template arguments on the global
//              records: what srt_trace_rays answers for the ray (center, d) is what a pixel gets.
//   Stacks.    Every wave of the workgroup has its own LDS stack region of stack_slots x 64 lanes x 4 bytes (dynamic LDS: four of them).
//   Lanes outside the rectangle stay in the traversal's ballot loop with an idle query: no lane leaves before the counters are summed.
//   Counters.  hit, miss, moved, degenerate: summed over a wave, then over the workgroup in LDS, then one integer atomic per workgroup and
//              non-zero counter, as the temporal kernel counts.
// No scratch, no float atomics, no inline assembly of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kMoTileW = 32, kMoTileH = 8, kMoThreads = kMoTileW * kMoTileH, kMoWaves = kMoThreads / 64;
constexpr uint32_t kMoCounters = 4;

__device__ __forceinline__ V3 ld3(const float *a) { return mk(a[0], a[1], a[2]); }
__device__ __forceinline__ bool finite1(float v) { return (v - v) == 0.0f; }
// (a.x * b.x + a.y * b.y) + a.z * b.z, as srt_c_api.h defines a dot product
__device__ __forceinline__ float dot3(V3 a, V3 b) { const float s = a.x * b.x + a.y * b.y; return s + a.z * b.z; }
__device__ __forceinline__ bool any_nonzero(V3 v) { return (v.x != 0.0f) | (v.y != 0.0f) | (v.z != 0.0f); }

__global__ __launch_bounds__(kMoThreads) void motion_kernel(const MotionParams P) {
    extern __shared__ float4 lds4[];
    __shared__ uint32_t wg_counts[kMoCounters];
    uint32_t *s_stack = reinterpret_cast<uint32_t *>(lds4);
    const uint32_t tile_y = blockIdx.x / P.tiles_x, tile_x = blockIdx.x - tile_y * P.tiles_x;
    if (threadIdx.x < kMoCounters) wg_counts[threadIdx.x] = 0u;
    __syncthreads();
    // wave wv owns the 16 x 4 sub-tile at (16 (wv & 1), 4 (wv >> 1)) of the 32 x 8 tile
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t x = tile_x * kMoTileW + 16u * (wv & 1u) + (lane & 15u), y = tile_y * kMoTileH + 4u * (wv >> 1) + (lane >> 4);
    const bool active = x < P.w && y < P.h;
    // the centre ray (an idle lane keeps a harmless direction: it starts no query)
    const V3 centre = ld3(P.center);
    V3 d = mk(0, 0, 1);
    if (active) {
        const float fi = (float)(P.ox + x), fj = (float)(P.oy + y);
        const V3 pc = (ld3(P.p00) + fi * ld3(P.du)) + fj * ld3(P.dv);
        d = pc - centre;
    }
    const V3 o = centre;
    TravStats ts;
    Trav tv; tv.node = kTravIdle; tv.sp = 0u; tv.top = -1; tv.c = kFltMax; tv.hit = -1; tv.nf[0] = tv.nf[1] = tv.nf[2] = 0u;
    const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    // this wave's stack region, this lane's column of it
    StackRef my_stack; my_stack.s16 = nullptr; my_stack.s32 = (lds_i32 *)s_stack + (size_t)wv * P.stack_slots * 64u + lane;
    stack_init<false>(my_stack);
    if (active) trav_begin<false>(tv, stack_base<false>(my_stack), P.tris, P.root_ref, o, d, 0.0f, kFltMax, ts);
    NodeSrc ns;
    ns.global_nodes = make_rsrc(P.nodes, (uint32_t)P.n_inner * 64u);
    ns.global_fringe = make_rsrc(P.fringe, (uint32_t)(P.n_records - P.n_inner) * P.fringe_stride);
    ns.fringe_stride = P.fringe_stride;
    ns.global_nodes_sw = make_rsrc(nullptr, 0u);
    ns.n_inner = P.n_inner;
    ns.lds_q0 = ns.lds_q1 = ns.lds_q2 = nullptr; ns.lds_r0 = ns.lds_r1 = nullptr; ns.n_cached = 0;
    while (__ballot(tv.node >= 0) != 0ull) {
        if (tv.node >= P.n_inner) trav_step_fringe<false, false>(tv, ns, o, d, inv, 0.0f, my_stack, ts);
        else if (tv.node >= 0) trav_step_inner<false, false, false>(tv, ns, o, inv, 0.0f, my_stack, ts);   // n_cached = 0: global records
    }
    uint32_t n[kMoCounters] = {0u, 0u, 0u, 0u};
    if (active) {
        const size_t pix = (size_t)y * P.w + x;
        const int k = tv.hit;
        float4 point = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
        if (k >= 0 && (uint32_t)k < P.n_tris) {      // (no vertex row is read for a miss)
            const float t = tv.c;
            const V3 pt = centre + t * d;
            const float *row = P.v_cur + 9 * (size_t)k;
            const V3 a = ld3(row), b = ld3(row + 3), c = ld3(row + 6);
            const V3 e1 = b - a, e2 = c - a, r = pt - a;
            const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), r1 = dot3(r, e1), r2 = dot3(r, e2);
            const float den = d11 * d22 - d12 * d12;
            const float beta = (d22 * r1 - d12 * r2) / den, gamma = (d11 * r2 - d12 * r1) / den;
            bool moved = false, valid = true;
            V3 pp = pt;
            if (P.v_prev) {
                const float *prow = P.v_prev + 9 * (size_t)k;
                const V3 da = ld3(prow) - a, db = ld3(prow + 3) - b, dc = ld3(prow + 6) - c;
                moved = any_nonzero(da) | any_nonzero(db) | any_nonzero(dc);
                if (moved) {
                    const V3 disp = (da + beta * (db - da)) + gamma * (dc - da);
                    pp = pt + disp;
                    valid = (den > 0.0f) & finite1(beta) & finite1(gamma) & finite1(pp.x) & finite1(pp.y) & finite1(pp.z);
                }
            }
            point = valid ? make_float4(pp.x, pp.y, pp.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            b0 = t; b1 = beta; b2 = gamma;
            n[0] = 1u; n[2] = moved ? 1u : 0u; n[3] = (moved & !valid) ? 1u : 0u;
        } else {
            n[1] = 1u;
        }
        if (P.out_point) P.out_point[pix] = point;
        if (P.out_tri) P.out_tri[pix] = n[0] ? k : -1;
        if (P.out_bary) { P.out_bary[3 * pix + 0] = b0; P.out_bary[3 * pix + 1] = b1; P.out_bary[3 * pix + 2] = b2; }
    }
    // every lane of the workgroup arrives here: a wave-level sum, the workgroup's word in LDS, one atomic per counter
#pragma unroll
    for (uint32_t k = 0; k < kMoCounters; k++) {
        const uint32_t s = wave_sum(n[k]);
        if (lane == 0u && s) atomicAdd(&wg_counts[k], s);
    }
    __syncthreads();
    if (threadIdx.x < kMoCounters && wg_counts[threadIdx.x]) atomicAdd(&P.counts[threadIdx.x], (unsigned long long)wg_counts[threadIdx.x]);
}

}  // namespace

hipError_t launch_motion(const MotionParams &p_in, hipStream_t st) {
    MotionParams p = p_in;
    if (p.w == 0 || p.h == 0) return hipSuccess;
    if (!p.tris || !p.v_cur || !p.counts || p.n_tris == 0) return hipErrorInvalidValue;
    if (p.root_ref >= 0 && (!p.nodes || !p.fringe || p.n_records <= 0)) return hipErrorInvalidValue;
    p.tiles_x = (p.w + kMoTileW - 1u) / kMoTileW;
    const uint64_t blocks = (uint64_t)p.tiles_x * ((p.h + kMoTileH - 1u) / kMoTileH);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    // one stack region per wave of the workgroup (launch_trace sizes one: its workgroup is one wave)
    p.stack_slots = (uint32_t)(p.stack_depth < 1 ? 1 : p.stack_depth) + (uint32_t)kStackSentinels;
    const size_t lds = (size_t)kMoWaves * p.stack_slots * 64 * 4;
    if (lds + 64 > kLdsBudget) return hipErrorInvalidValue;
    if (lds > 48 * 1024) {
        const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void *>(&motion_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ae != hipSuccess) return ae;
    }
    hipLaunchKernelGGL(motion_kernel, dim3((uint32_t)blocks), dim3(kMoThreads), lds, st, p);
    return hipGetLastError();
}

}  // namespace srt
