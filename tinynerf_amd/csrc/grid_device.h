// The regular grid of the mesh exports (mesh.hip, tsdf.hip), written once: nx x ny x nz cells, (nx+1)(ny+1)(nz+1) nodes, x fastest in
// both; the node idx on an axis sits at fmaf(idx, h, lo).
#pragma once
#include "tn_common.h"

namespace tn {

// the number of a grid's cells, or of its nodes: 0 with an empty axis, -1 for a negative dim or a number of 2^31 or more
inline int64_t grid_count(const int32_t *dims, bool nodes)
{
    const int64_t limit = (int64_t)1 << 31;
    if (dims[0] < 0 || dims[1] < 0 || dims[2] < 0) return -1;
    if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return 0;
    const int64_t e = nodes ? 1 : 0, xy = (dims[0] + e) * (dims[1] + e);      // (< 2^62)
    if (xy >= limit || xy * (dims[2] + e) >= limit) return -1;
    return xy * (dims[2] + e);
}

// cell c -> its index on every axis and its lowest corner's node
__device__ __forceinline__ void cell_of(int nx, int ny, uint32_t c, int idx[3], int64_t &node)
{
    const uint32_t row = c / (uint32_t)nx, k = row / (uint32_t)ny;
    idx[0] = (int)(c - row * (uint32_t)nx);
    idx[1] = (int)(row - k * (uint32_t)ny);
    idx[2] = (int)k;
    node = idx[0] + ((int64_t)nx + 1) * (idx[1] + ((int64_t)ny + 1) * idx[2]);
}

// f(d, n) for the eight corners d = dx + 2 dy + 4 dz of the cell whose lowest corner is `node`; n: the corner's node
template <typename F>
__device__ __forceinline__ void for_corners(int nx, int ny, int64_t node, F f)
{
    const int64_t sy = (int64_t)nx + 1, sz = sy * ((int64_t)ny + 1);
#pragma unroll
    for (int d = 0; d < 8; ++d) f(d, node + (d & 1) + ((d >> 1) & 1) * sy + (d >> 2) * sz);
}

// node m of a grid with sx x sy x .. nodes -> its position; I is the width of the two divisions
template <typename I>
__device__ __forceinline__ void node_position(I m, I sx, I sy, const float lo[3], const float h[3], float x[3])
{
    const I row = m / sx, k = row / sy;
    const I idx[3] = {m - row * sx, row - k * sy, k};
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = fmaf((float)idx[a], h[a], lo[a]);
}

}  // namespace tn
