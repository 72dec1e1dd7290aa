// srt_refit.hip -- BVH refit on the device: new vertices on the uploaded topology (srt_refit_vertices / srt_refit_vertices_dev;
// include/srt_c_api.h states the operation at srt_scene_refit and srt_refit_vertices).
//
// A translation unit of its own, like the temporal stage's: no render, denoise, develop, expose, present, despeckle or temporal kernel is
// touched and their machine code stays what it was.  Built with the exactness flags of the render unit (-ffp-contract=off, no fast-math,
// correctly rounded division and square root): every product, sum, quotient and root below is rounded once, in the order written, which
// is the order of tri_precompute and finish_boxes_and_depth (srt_host.cpp) -- the images this unit writes are what flatten_scene would
// make of the host-refitted scene, equal as values (a minimum or maximum of +0 and -0 may carry either sign, a NaN any payload).
//
// Three kernels.
//   refit_validate_kernel   counts the coordinates that are not finite: a grid-stride loop, a wave-level sum, one integer atomic per wave.
//   refit_triangle_kernel   one thread per triangle: tri::init restated (normal, D, projection plane, winding, padded box), the 12-word
//                           triangle record, the normal of the shading record, the leaf box into scratch, and the triangle's inline copy
//                           into the FRINGE block that holds it (words 0 .. 10; word 11, the reference, stays).
//   refit_level_kernel      one thread per record of ONE height (height = 1 + the largest height among the child records, a leaf child
//                           counting 0), launched once per height from the bottom up: the children's boxes -- from the leaf scratch or
//                           from the child record's own box, which the launch before wrote -- go into the record, their union (left,
//                           right) into the record's own box.  The kernel boundary is the only synchronisation there is.
// No scratch memory, no LDS, no inline assembly, no atomics on boxes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srt_c_api.h"
#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kRefitThreads = 256;
constexpr uint32_t kRefitValidateMaxBlocks = 1024;

// fminf / fmaxf of the host on finite operands, as a compare and a select (a = the first operand, b = the second)
__device__ __forceinline__ float min_sel(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float max_sel(float a, float b) { return (b > a) ? b : a; }
__device__ __forceinline__ float comp(float x, float y, float z, int a) { return a == 0 ? x : (a == 1 ? y : z); }
__device__ __forceinline__ float bits_f(uint32_t u) { return __uint_as_float(u); }

__global__ __launch_bounds__(kRefitThreads) void refit_validate_kernel(const float *verts, size_t n, uint32_t *count) {
    uint32_t bad = 0u;
    for (size_t i = (size_t)blockIdx.x * kRefitThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kRefitThreads) {
        const float x = verts[i];
        bad += ((x - x) == 0.0f) ? 0u : 1u;      // (an infinity and a NaN both give NaN)
    }
    const uint32_t s = wave_sum(bad);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(count, s);
}

// the padded box of one axis: aabb(v0, v1, v2).pad() (tri_precompute)
__device__ __forceinline__ void axis_box(float a0, float a1, float a2, float &lo, float &hi) {
    lo = min_sel(a0, min_sel(a1, a2));
    hi = max_sel(a0, max_sel(a1, a2));
    const float delta = 0.0001f;
    if (!((hi - lo) >= delta)) { const float padding = delta / 2; lo = lo - padding; hi = hi + padding; }
}

__global__ __launch_bounds__(kRefitThreads) void refit_triangle_kernel(const RefitParams P) {
    const uint32_t k = blockIdx.x * kRefitThreads + threadIdx.x;
    if (k >= P.n_tris) return;
    const float *v = P.verts + 9 * (size_t)k;
    const float v0x = v[0], v0y = v[1], v0z = v[2], v1x = v[3], v1y = v[4], v1z = v[5], v2x = v[6], v2y = v[7], v2z = v[8];
    // n = unit3(cross3(v1 - v0, v2 - v0)), unit3(c) = (1 / len3(c)) * c
    const float ux = v1x - v0x, uy = v1y - v0y, uz = v1z - v0z;
    const float wx = v2x - v0x, wy = v2y - v0y, wz = v2z - v0z;
    const float cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    const float len = sqrtf(cx * cx + cy * cy + cz * cz);
    const float inv = 1 / len;
    const float nx = inv * cx, ny = inv * cy, nz = inv * cz;
    // |dot(normal, axis)| < 1e-8 with the full three-term dots
    const bool perp_x = fabsf(nx * 1.f + ny * 0.f + nz * 0.f) < 1e-8f;
    const bool perp_y = fabsf(nx * 0.f + ny * 1.f + nz * 0.f) < 1e-8f;
    const bool perp_z = fabsf(nx * 0.f + ny * 0.f + nz * 1.f) < 1e-8f;
    uint32_t plane = P.tri_tab[2 * (size_t)k];      // the raw, sticky aa_plane: kept unless the triangle is axis aligned
    if (perp_y && perp_z) plane = SRT_AAP_YZ;
    else if (perp_x && perp_z) plane = SRT_AAP_XZ;
    else if (perp_x && perp_y) plane = SRT_AAP_XY;
    const float D = nx * v0x + ny * v0y + nz * v0z;
    const int w = plane == SRT_AAP_YZ ? 1 : 0, h = (plane == SRT_AAP_YZ || plane == SRT_AAP_XZ) ? 2 : 1;
    const float v0w = comp(v0x, v0y, v0z, w), v0h = comp(v0x, v0y, v0z, h);
    const float v1w = comp(v1x, v1y, v1z, w), v1h = comp(v1x, v1y, v1z, h);
    const float v2w = comp(v2x, v2y, v2z, w), v2h = comp(v2x, v2y, v2z, h);
    const float area = (v0w - v2w) * (v1h - v2h) - (v1w - v2w) * (v0h - v2h);
    const bool clockwise = area >= 0;
    float box[6];
    axis_box(v0x, v1x, v2x, box[0], box[1]);
    axis_box(v0y, v1y, v2y, box[2], box[3]);
    axis_box(v0z, v1z, v2z, box[4], box[5]);

    float *shade = P.shade + 12 * (size_t)k;
    const uint32_t mat = __float_as_uint(shade[3]);      // the material index: an input, as on the host
    const uint32_t flags = (w == 1 ? 1u : 0u) | (h == 2 ? 2u : 0u) | (clockwise ? 4u : 0u) | (mat << 8);
    float4 *tri = reinterpret_cast<float4 *>(P.tris + 12 * (size_t)k);
    tri[0] = make_float4(nx, ny, nz, D);
    tri[1] = make_float4(v0w, v0h, v1w, v1h);
    tri[2] = make_float4(v2w, v2h, bits_f(flags), 0.f);
    shade[0] = nx; shade[1] = ny; shade[2] = nz;
#pragma unroll
    for (int a = 0; a < 6; a++) P.leaf_box[6 * (size_t)k + a] = box[a];
    const uint32_t slot = P.tri_tab[2 * (size_t)k + 1];
    if (slot != kRefitNoSlot) {
        // the inline copy in the parent's FRINGE block: pair j holds word j of the left and of the right child; bit 31 of the flags is
        // the sign flip of a counter-clockwise triangle (flatten_scene)
        float *o = P.fringe + (size_t)(slot >> 1) * P.fringe_stride + (slot & 1u);
        const float b[11] = {nx, ny, nz, D, v0w, v0h, v1w, v1h, v2w, v2h, bits_f(clockwise ? flags : (flags | 0x80000000u))};
#pragma unroll
        for (int j = 0; j < 11; j++) o[2 * j] = b[j];
    }
}

__global__ __launch_bounds__(kRefitThreads) void refit_level_kernel(const RefitParams P, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x;
    if (i >= count) return;
    const uint32_t r = P.sched[first + i];
    const int32_t cl = P.child[2 * (size_t)r], cr = P.child[2 * (size_t)r + 1];
    const float *bl = cl < 0 ? P.leaf_box + 6 * (size_t)(uint32_t)~cl : P.rec_box + 6 * (size_t)cl;
    const float *br = cr < 0 ? P.leaf_box + 6 * (size_t)(uint32_t)~cr : P.rec_box + 6 * (size_t)cr;
    float L[6], R[6];
#pragma unroll
    for (int a = 0; a < 6; a++) { L[a] = bl[a]; R[a] = br[a]; }
    if (r < P.n_inner) {
        // INNER: per axis (lo_L, lo_R, hi_L, hi_R); the swizzled image repeats (lo_L, lo_R) behind them
        float4 *o = reinterpret_cast<float4 *>(P.nodes + 16 * (size_t)r);
#pragma unroll
        for (int a = 0; a < 3; a++) o[a] = make_float4(L[2 * a], R[2 * a], L[2 * a + 1], R[2 * a + 1]);
        if (P.nodes_sw) {
            float *s = P.nodes_sw + 20 * (size_t)r;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                s[6 * a + 0] = L[2 * a]; s[6 * a + 1] = R[2 * a]; s[6 * a + 2] = L[2 * a + 1]; s[6 * a + 3] = R[2 * a + 1];
                s[6 * a + 4] = L[2 * a]; s[6 * a + 5] = R[2 * a];
            }
        }
    } else {
        // FRINGE: the box words of an internal child's block (a leaf child's block is its triangle's copy: refit_triangle_kernel)
        float *o = P.fringe + (size_t)(r - P.n_inner) * P.fringe_stride;
        if (cl >= 0) {
#pragma unroll
            for (int a = 0; a < 6; a++) o[2 * a] = L[a];
        }
        if (cr >= 0) {
#pragma unroll
            for (int a = 0; a < 6; a++) o[2 * a + 1] = R[a];
        }
    }
    float *own = P.rec_box + 6 * (size_t)r;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        own[2 * a] = min_sel(L[2 * a], R[2 * a]);
        own[2 * a + 1] = max_sel(L[2 * a + 1], R[2 * a + 1]);
    }
}

}  // namespace

hipError_t launch_refit_validate(const float *verts, size_t n_floats, uint32_t *count, hipStream_t st) {
    if (!verts || !count) return hipErrorInvalidValue;
    if (n_floats == 0) return hipSuccess;
    const size_t blocks = (n_floats + kRefitThreads - 1) / kRefitThreads;
    const uint32_t grid = (uint32_t)(blocks < kRefitValidateMaxBlocks ? blocks : kRefitValidateMaxBlocks);
    hipLaunchKernelGGL(refit_validate_kernel, dim3(grid), dim3(kRefitThreads), 0, st, verts, n_floats, count);
    return hipGetLastError();
}

hipError_t launch_refit_triangles(const RefitParams &p, hipStream_t st) {
    if (!p.verts || !p.tri_tab || !p.tris || !p.shade || !p.fringe || !p.leaf_box || p.fringe_stride < 24u) return hipErrorInvalidValue;
    if (p.n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(refit_triangle_kernel, dim3((p.n_tris + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_refit_level(const RefitParams &p, uint32_t first, uint32_t count, hipStream_t st) {
    if (!p.child || !p.sched || !p.nodes || !p.fringe || !p.leaf_box || !p.rec_box || p.fringe_stride < 24u) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(refit_level_kernel, dim3((count + kRefitThreads - 1) / kRefitThreads), dim3(kRefitThreads), 0, st, p, first, count);
    return hipGetLastError();
}

}  // namespace srt
