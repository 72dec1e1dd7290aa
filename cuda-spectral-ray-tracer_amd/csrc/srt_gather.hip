// srt_gather.hip -- the exchange unit of an accumulation (srt_pack_accum / srt_unpack_accum; include/srt_c_api.h states the calls,
// srt_internal.h at GatherParams the layout, tests/gather_reference.py restates it in numpy): the records of a rank's own 8 x 8 tiles
// copied out of the block-linear accumulation buffers into one contiguous unit, and the units of the other ranks copied back into the
// buffers of the context that gathers them.  After the unpack that context holds the accumulation a (0, 1) context would hold.
//
// A translation unit of its own, like the present's and the firefly filter's: no existing kernel is touched and their machine code
// stays what it was.  The work is a pure copy -- no arithmetic, every word moves as its bit pattern (the kernels use integer types
// throughout: a state word or a NaN payload is a float slot's bits and nothing else) -- so it is bandwidth bound and is built for wide,
// contiguous accesses on both sides.
//
// One kernel, two directions (template argument), one workgroup of ONE wave per tile record:
//   * lane lt resolves slot lt of the tile to its block-linear lane index (tile_slot_pixel, queue_slot_in_chunk, block_linear_idx: the
//     render kernel's own map) and leaves it in LDS -- kNoLane for a slot outside the chunk, all 64 for a tile beyond the grid;
//   * the plane words: a tile row of eight pixels is two groups of four consecutive columns.  With tx a multiple of four such a group
//     lies inside one block row, so its four lanes are consecutive and the first one is a multiple of four: one 16-byte access on the
//     grid side against one on the unit side (plane p, group g: unit words 64 p + 4 g ..).  The (plane, group) pairs -- 48 or 80 --
//     are flattened over the 64 lanes.  A group that is not whole (the chunk ends inside it) or not consecutive, any other tx, and
//     misaligned bases walk the four slots with 4-byte accesses: the same bits;
//   * the feature rows (32 B per lane) and the film rows (384 B per lane): (slot, quad) is flattened over the lanes, so consecutive
//     lanes move consecutive 16-byte quads -- the unit side is one contiguous run per instruction, the grid side runs of a whole row
//     -- instead of every lane walking its own row at a 384-byte stride.
// The pack writes +0 where a slot is outside the chunk (a unit is a function of the accumulation alone); the unpack skips those slots
// and the whole unit of its own rank.  No atomics, no cross-workgroup synchronisation, no scratch; 256 B of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srt_kernel_common.h"

namespace srt {

namespace {

constexpr uint32_t kNoLane = 0xffffffffu;

__device__ __forceinline__ uint32_t *gather_plane(const GatherParams &P, uint32_t plane) {
    // (selects, not a table: a table indexed per lane would live in scratch)
    uint32_t *p = P.sums + (size_t)plane * P.n_lanes;
    p = plane == 3u ? P.state : p;
    p = plane == 4u ? P.sum2 : p;
    return p;
}

// the rows of one kind: `quads` 16-byte quads per lane of the grid at `rows`, per slot of the tile at `rec`
template <bool UNPACK>
__device__ __forceinline__ void gather_rows(uint32_t *rows, uint32_t *rec, uint32_t quads, const uint32_t *lane_of, bool vec) {
    const uint32_t items = (uint32_t)kTileLanes * quads;
    for (uint32_t item = threadIdx.x; item < items; item += (uint32_t)kTileLanes) {
        const uint32_t slot = item / quads, q = item - slot * quads;
        const uint32_t idx = lane_of[slot];
        uint32_t *u = rec + (size_t)item * 4u;
        uint32_t *g = rows + ((size_t)idx * quads + q) * 4u;      // (formed, not touched, when idx == kNoLane)
        if (vec) {
            if (UNPACK) { if (idx != kNoLane) *reinterpret_cast<uint4 *>(g) = *reinterpret_cast<const uint4 *>(u); }
            else *reinterpret_cast<uint4 *>(u) = idx != kNoLane ? *reinterpret_cast<const uint4 *>(g) : make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (uint32_t e = 0; e < 4u; e++) {
                if (UNPACK) { if (idx != kNoLane) g[e] = u[e]; }
                else u[e] = idx != kNoLane ? g[e] : 0u;
            }
        }
    }
}

template <bool UNPACK>
__global__ __launch_bounds__(kTileLanes) void gather_kernel(const GatherParams P) {
    __shared__ uint32_t lane_of[kTileLanes];
    // pack: the records of this rank's unit; unpack: the records of every unit but this rank's own
    const uint32_t r = UNPACK ? blockIdx.x / P.tiles_padded : P.rank;
    const uint32_t t = UNPACK ? blockIdx.x - r * P.tiles_padded : blockIdx.x;
    if (UNPACK && r == P.rank) return;      // (the whole workgroup: nobody waits at the barrier below)
    const uint32_t lt = threadIdx.x;
    const uint32_t tile = queue_global_tile(t, r, P.world);
    const PixelIJ px = tile_slot_pixel(tile, lt, P.tiles_x);
    const bool in = queue_slot_in_chunk(tile, lt, px, P.n_tiles, (uint32_t)kTileLanes, P.width, P.height, P.tx, P.ty, P.bx, P.by);
    lane_of[lt] = in ? block_linear_idx(px.i, px.j, P.tx, P.ty, P.bx) : kNoLane;
    __syncthreads();
    uint32_t *rec = P.unit + ((size_t)(UNPACK ? r : 0u) * P.tiles_padded + t) * P.tile_words;

    // the plane words [plane][slot]
    for (uint32_t item = lt; item < P.n_planes * 16u; item += (uint32_t)kTileLanes) {
        const uint32_t plane = item >> 4, g = item & 15u;
        uint32_t *grid = gather_plane(P, plane);
        uint32_t *u = rec + plane * (uint32_t)kTileLanes + 4u * g;
        const uint32_t i0 = lane_of[4u * g], i1 = lane_of[4u * g + 1u], i2 = lane_of[4u * g + 2u], i3 = lane_of[4u * g + 3u];
        const bool whole = (i0 != kNoLane) & (i3 != kNoLane) & (i1 == i0 + 1u) & (i2 == i0 + 2u) & (i3 == i0 + 3u) & ((i0 & 3u) == 0u);
        if (P.vec && whole) {
            if (UNPACK) *reinterpret_cast<uint4 *>(grid + i0) = *reinterpret_cast<const uint4 *>(u);
            else *reinterpret_cast<uint4 *>(u) = *reinterpret_cast<const uint4 *>(grid + i0);
        } else {
            const uint32_t idx[4] = {i0, i1, i2, i3};      // (unrolled below: registers)
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                if (UNPACK) { if (idx[e] != kNoLane) grid[idx[e]] = u[e]; }
                else u[e] = idx[e] != kNoLane ? grid[idx[e]] : 0u;
            }
        }
    }
    uint32_t *next = rec + P.n_planes * (uint32_t)kTileLanes;
    if (P.features) {
        gather_rows<UNPACK>(P.features, next, kFeatureStride / 4u, lane_of, P.vec != 0u);
        next += (uint32_t)kTileLanes * kFeatureStride;
    }
    if (P.film) gather_rows<UNPACK>(P.film, next, kFilmStride / 4u, lane_of, P.vec != 0u);
}

}  // namespace

uint32_t gather_tile_words(uint32_t n_planes, bool features, bool film) {
    return (uint32_t)kTileLanes * (n_planes + (features ? kFeatureStride : 0u) + (film ? kFilmStride : 0u));
}

hipError_t launch_gather(const GatherParams &p, bool unpack, bool allow_vector, hipStream_t st) {
    if (!p.unit || !p.sums || (p.n_planes != 3u && p.n_planes != 5u) || (p.n_planes == 5u && (!p.state || !p.sum2))) return hipErrorInvalidValue;
    if (p.world == 0 || p.rank >= p.world || p.tiles_x == 0 || p.tx == 0 || p.ty == 0 || p.bx == 0 || p.by == 0) return hipErrorInvalidValue;
    if (p.tile_words != gather_tile_words(p.n_planes, p.features != nullptr, p.film != nullptr)) return hipErrorInvalidValue;
    if ((uint64_t)p.tx * p.ty * p.bx * p.by != p.n_lanes) return hipErrorInvalidValue;      // every index the kernel forms is below n_lanes
    if (p.tiles_padded != (p.n_tiles + p.world - 1u) / p.world) return hipErrorInvalidValue;
    const uint64_t records = (uint64_t)p.tiles_padded * (unpack ? p.world : 1u);
    if (records == 0 || (unpack && p.world == 1u)) return hipSuccess;
    if (records > 0x7fffffffull) return hipErrorInvalidValue;
    // the 16-byte paths: every base on the 16-byte grid, four columns of a tile row inside one block row
    auto aligned = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    GatherParams k = p;
    k.vec = allow_vector && p.tx % 4u == 0 && p.n_lanes % 4u == 0 && aligned(p.unit) && aligned(p.sums) && aligned(p.state) && aligned(p.sum2) &&
                    aligned(p.features) && aligned(p.film)
                ? 1u : 0u;
    if (unpack) hipLaunchKernelGGL(gather_kernel<true>, dim3((uint32_t)records), dim3(kTileLanes), 0, st, k);
    else hipLaunchKernelGGL(gather_kernel<false>, dim3((uint32_t)records), dim3(kTileLanes), 0, st, k);
    return hipGetLastError();
}

}  // namespace srt
