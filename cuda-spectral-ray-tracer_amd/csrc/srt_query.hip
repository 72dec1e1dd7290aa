// srt_query.hip -- batched ray queries: the closest hit over an interval and any-hit occlusion (srt_intersect_rays*, srt_occluded_rays*;
// include/srt_c_api.h states every operation at "Ray queries", tests/query_reference.py restates the answers in float64).
//
// A translation unit of its own, like the surface-motion pass: no render, denoise, develop, expose, present, despeckle, temporal, refit or
// motion kernel is touched and their machine code stays what it was.  Built with the exactness flags of the other units (-ffp-contract=off,
// no fast-math, correctly rounded division): the visits below are the renderer's own C++ visit functions (srt_device.h), so a ray's closest
// hit over [0, FLT_MAX] is srt_trace_rays' answer word for word.
//
// One template, query_kernel<ANY, NARROW, ALL_CACHED, PAIRED>, in the shape the render launch plan picks for the scene (render_launch_plan,
// render_paired_variant; the context's test knobs included):
//   Workgroups. Persistent: the plan's waves per workgroup, as many workgroups as fill the device (or the test grid).  Each stages the
//              plan's n_cached INNER records into LDS once, as render_kernel does -- three plane arrays and the child references, no colour
//              tables -- and gives every wave one traversal stack of stack_depth + 2 slots x 64 lanes.
//   Rays.      A wave pulls rays from one 32-bit counter (zeroed on the call's stream before the launch) with one wave-aggregated atomic
//              per refill; a lane whose query ended takes the next ray at the wave's next refill.  A ray is two 16-byte loads: (o, tmin),
//              (d, tmax).  A ray's answer depends on the ray and the tree alone, never on the lane or wave that took it.
//   Steps.     INNER or FRINGE by the lanes waiting at each kind of record (FRINGE lanes x score_fringe against INNER lanes x 256, the
//              renderer's weights), a short burst of INNER steps per decision.
//   ANY.       The query ends after the first traversal step that accepted a triangle: up to then it made the closest query's visits.
// No scratch, no inline assembly, no spin-waits, no environment reads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr int kQueryBurst = 4;              // INNER steps per decision at most ...
constexpr uint32_t kQueryBurstDrop = 3;     // ... and the burst ends once fewer than a third of its lanes are still at inner records
constexpr uint32_t kRefillLanes = 16;       // a wave refills when this many of its lanes have no query (or none is traversing)

template <bool ANY, bool NARROW, bool ALL_CACHED, bool PAIRED>
__global__ __launch_bounds__(1024) void query_kernel(const QueryParams P) {
    extern __shared__ float4 lds4[];
    const uint32_t nc = (uint32_t)P.n_cached;
    float4 *s_q0 = lds4, *s_q1 = s_q0 + nc, *s_q2 = s_q1 + nc;
    uint32_t *s_r0 = reinterpret_cast<uint32_t *>(s_q2 + nc), *s_r1 = s_r0 + nc;
    const size_t cache_b = (((size_t)nc * (NARROW ? 52u : 56u)) + 15u) & ~(size_t)15u;
    char *s_stack_base = reinterpret_cast<char *>(lds4) + cache_b;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    // the cached INNER records, once per workgroup (render_kernel's staging)
    for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) {
        s_q0[k] = P.nodes[4 * k + 0]; s_q1[k] = P.nodes[4 * k + 1]; s_q2[k] = P.nodes[4 * k + 2];
        const float4 q3 = P.nodes[4 * k + 3];
        const uint32_t lr = __float_as_uint(q3.x), rr = __float_as_uint(q3.y);
        if (NARROW) s_r0[k] = (lr & 0xffffu) | (rr << 16);
        else { s_r0[k] = lr; s_r1[k] = rr; }
    }
    __syncthreads();      // the only barrier: from here on every wave runs on its own

    NodeSrc ns;
    ns.global_nodes = make_rsrc(P.nodes, (uint32_t)P.n_inner * 64u);
    ns.fringe_stride = P.fringe_stride;
    ns.global_fringe = make_rsrc(P.fringe, (uint32_t)(P.n_records - P.n_inner) * P.fringe_stride);
    ns.global_nodes_sw = make_rsrc(nullptr, 0u);
    ns.n_inner = P.n_inner;
    ns.lds_q0 = (lds_cf4 *)s_q0; ns.lds_q1 = (lds_cf4 *)s_q1; ns.lds_q2 = (lds_cf4 *)s_q2;
    ns.lds_r0 = (lds_cu32 *)s_r0; ns.lds_r1 = (lds_cu32 *)s_r1;
    ns.n_cached = P.n_cached;
    StackRef my_stack;
    {
        const size_t slots = (size_t)(P.stack_depth < 1 ? 1 : P.stack_depth) + kStackSentinels;
        my_stack.s16 = (lds_i16 *)(s_stack_base + (size_t)wave * slots * 128u) + lane;
        my_stack.s32 = (lds_i32 *)(s_stack_base + (size_t)wave * slots * 256u) + lane;
        stack_init<NARROW>(my_stack);      // this wave's own column: no barrier needed
    }
    const uint32_t n_inner_u = (uint32_t)P.n_inner;
    const uint32_t w_fringe = P.score_fringe;

    TravStats ts;
    Trav tv; tv.node = kTravIdle; tv.sp = 0u; tv.top = -1; tv.c = kFltMax; tv.hit = -1; tv.nf[0] = tv.nf[1] = tv.nf[2] = 0u;
    V3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f), inv = mk(0.f, 0.f, 1.f);
    float tmin = 0.f;
    uint32_t ray = 0;
    bool drained = false;      // (wave-uniform) the counter has passed n: no more refills
    for (;;) {
        // ---- a finished query writes its answer and its lane becomes free --------------------------------------------------------
        if (tv.node == kTravDone) {
            const int tri = tv.hit;
            if (ANY) {
                P.occluded[ray] = tri >= 0 ? (uint8_t)1 : (uint8_t)0;
            } else {
                // trace_rays_kernel's output row (srt_kernels.hip), the same expressions
                float ff = 0.f, mat = 0.f;
                if (tri >= 0) {
                    const float4 ta = P.tris[3 * tri + 0];
                    const float4 tc = P.tris[3 * tri + 2];
                    ff = dot(d, mk(ta.x, ta.y, ta.z)) < 0 ? 1.f : 0.f;
                    mat = (float)(__float_as_uint(tc.z) >> 8);
                }
                P.hits[ray] = make_float4(tri >= 0 ? tv.c : 0.f, (float)tri, ff, mat);
            }
            tv.node = kTravIdle;
        }
        // ---- refill: one wave-aggregated atomic hands the free lanes consecutive rays ---------------------------------------------
        const unsigned long long free_mask = __ballot(tv.node == kTravIdle);
        const unsigned long long trav_mask = __ballot(tv.node >= 0);
        const uint32_t n_free = (uint32_t)__popcll(free_mask);
        if (!drained && n_free != 0u && (n_free >= kRefillLanes || trav_mask == 0ull)) {
            const uint32_t leader = (uint32_t)__ffsll((long long)free_mask) - 1u;
            uint32_t base = 0u;
            if (lane == leader) base = atomicAdd(P.counter, n_free);
            base = __shfl(base, (int)leader, 64);
            if (base + n_free >= P.n) drained = true;
            if (tv.node == kTravIdle) {
                const uint32_t rank = (uint32_t)__popcll(free_mask & ((1ull << lane) - 1ull));
                const uint32_t r = base + rank;
                if (r < P.n) {
                    ray = r;
                    const float4 a = P.rays[2 * (size_t)r + 0], b = P.rays[2 * (size_t)r + 1];
                    o = mk(a.x, a.y, a.z); tmin = a.w;
                    d = mk(b.x, b.y, b.z);
                    inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);           // aabb.cu:17, hoisted out of the box test
                    ray_near_addresses(ns, inv, tv.nf);
                    (void)trav_begin<false>(tv, stack_base<NARROW>(my_stack), P.tris, P.root_ref, o, d, tmin, b.w, ts);   // done at once: kTravDone
                }
            }
            continue;      // (queries that ended at their start are written before the next step)
        }
        if (trav_mask == 0ull) {
            if (drained) break;
            continue;
        }
        // ---- one decision: a FRINGE step or a burst of INNER steps ----------------------------------------------------------------
        const unsigned long long fringe_mask = __ballot(tv.node >= (int)n_inner_u);
        const uint32_t n_trav = (uint32_t)__popcll(trav_mask), n_fringe = (uint32_t)__popcll(fringe_mask);
        const uint32_t n_in = n_trav - n_fringe;
        if (n_fringe * w_fringe > (n_in << 8)) {
            if (tv.node >= (int)n_inner_u) trav_step_fringe<false, NARROW, PAIRED>(tv, ns, o, d, inv, tmin, my_stack, ts);
            // the any query stops after the step that accepted a triangle (only a FRINGE step tests triangles)
            if (ANY && tv.node >= 0 && tv.hit >= 0) tv.node = kTravDone;
        } else {
            const uint32_t stay = (n_in + kQueryBurstDrop - 1u) / kQueryBurstDrop;
#pragma unroll
            for (int b = 0; b < kQueryBurst; b++) {
                if ((uint32_t)tv.node < n_inner_u) trav_step_inner<false, NARROW, ALL_CACHED>(tv, ns, o, inv, tmin, my_stack, ts);
                if ((uint32_t)__popcll(__ballot((uint32_t)tv.node < n_inner_u)) < stay) break;
            }
        }
    }
}

template <bool ANY, bool NARROW, bool ALL_CACHED, bool PAIRED>
hipError_t launch_query_variant(const QueryParams &p, uint32_t n_blocks, uint32_t waves_per_block, size_t lds, hipStream_t st) {
    const void *fn = reinterpret_cast<const void *>(&query_kernel<ANY, NARROW, ALL_CACHED, PAIRED>);
    // per launch: the attribute belongs to the function on the current device (render_kernel's launcher does the same)
    if (const hipError_t ae = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget)) return ae;
    hipLaunchKernelGGL((query_kernel<ANY, NARROW, ALL_CACHED, PAIRED>), dim3(n_blocks), dim3(64u * waves_per_block), lds, st, p);
    return hipGetLastError();
}

template <bool ANY>
hipError_t launch_query_any(const QueryParams &p, const QueryShape &s, hipStream_t st) {
    // the shapes render_paired_variant allows a PAIRED variant in (<1,1> and <0,0>), the general variant everywhere
    if (s.narrow && s.all_cached) return s.paired ? launch_query_variant<ANY, true, true, true>(p, s.n_blocks, s.waves_per_block, s.lds, st)
                                                  : launch_query_variant<ANY, true, true, false>(p, s.n_blocks, s.waves_per_block, s.lds, st);
    if (!s.narrow && !s.all_cached) return s.paired ? launch_query_variant<ANY, false, false, true>(p, s.n_blocks, s.waves_per_block, s.lds, st)
                                                    : launch_query_variant<ANY, false, false, false>(p, s.n_blocks, s.waves_per_block, s.lds, st);
    if (s.narrow) return launch_query_variant<ANY, true, false, false>(p, s.n_blocks, s.waves_per_block, s.lds, st);
    return launch_query_variant<ANY, false, true, false>(p, s.n_blocks, s.waves_per_block, s.lds, st);
}

}  // namespace

QueryShape query_shape(const LaunchPlan &lp, bool narrow, bool paired, int stack_depth, int n_records, const PlanKnobs &knobs, uint32_t n_cu,
                       uint32_t max_waves, size_t n_rays) {
    QueryShape s;
    s.narrow = narrow; s.all_cached = lp.all_cached; s.paired = paired; s.n_cached = lp.n_cached;
    uint64_t waves = (uint64_t)n_cu * (uint64_t)lp.waves_per_cu;
    const uint64_t needed = (n_rays + 63) / 64;
    if (waves > needed) waves = needed;
    if (max_waves > 0 && waves > max_waves) waves = max_waves;
    if (waves < 1) waves = 1;
    s.waves_per_block = (uint32_t)std::min<uint64_t>((uint64_t)lp.waves_per_block, waves);
    s.n_blocks = (uint32_t)((waves + s.waves_per_block - 1) / s.waves_per_block);
    s.waves = s.n_blocks * s.waves_per_block;
    // the render workgroup's LDS without its tables (uniform block, colour matching rows): the cache and one stack per wave
    s.lds = render_lds_bytes(stack_depth, (int)s.waves_per_block, lp.n_cached, n_records, knobs) - (size_t)kLdsTablesF4 * 16;
    return s;
}

hipError_t launch_query(const QueryParams &p, const QueryShape &s, bool any, hipStream_t st) {
    if (p.n == 0) return hipSuccess;
    if (!p.counter || !p.rays || !p.tris || (any ? !p.occluded : !p.hits)) return hipErrorInvalidValue;
    if (p.root_ref >= 0 && (!p.nodes || !p.fringe || p.n_records <= 0)) return hipErrorInvalidValue;
    if (s.lds > kLdsBudget) return hipErrorInvalidValue;
    return any ? launch_query_any<true>(p, s, st) : launch_query_any<false>(p, s, st);
}

}  // namespace srt
