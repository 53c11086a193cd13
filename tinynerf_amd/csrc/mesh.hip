// Triangle mesh of a scalar field sampled on a regular grid: naive Surface Nets -- one vertex per cell the level set passes
// through, one quad per grid edge it crosses --, kept on the device.  No reference call site: the reference renders images and exports
// no geometry.
//
// Definition (include/tinynerf_hip.h has it in full) -- fp32 throughout:
//   node (i,j,k) is inside when values[i + (nx+1)(j + (ny+1)k)] >= level (false for NaN); a cell is active when its 8 corners disagree
//   vertex of an active cell: u = (sum over its crossed edges, in the fixed order of 12, of the edge's crossing point in cell
//     coordinates) / their number, with t = clamp((level - v0) / (v1 - v0), 0, 1) along the edge (0.5 when an end is not finite);
//     p_c = fmaf(idx_c + u_c, h_c, lo_c); normal = -grad / |grad| of the cell's trilinear interpolant at u (0 when that is not finite)
//   quad of a crossed edge from node (i,j,k) along axis a with idx_b >= 1 and idx_c >= 1: the vertex ids of the 4 cells around it,
//     counter-clockwise seen from +a, reversed when the lower node is outside; triangles (q0,q1,q2), (q0,q2,q3)
// The k-th active cell in cell order writes vertex row k, the m-th quad in (cell, axis) order face rows 2m and 2m + 1.
//
// Four launches on the caller's stream, one lane per cell, no atomics -- the same bytes on every call (the pattern's pieces:
// compact_device.h; the grid's: grid_device.h):
//   mesh_mark_kernel      every wave writes 4 ballots (active, quad on axis 0 / 1 / 2), every workgroup of 256 its two counts
//   mesh_scan_kernel      one workgroup per count column turns it into exclusive offsets and writes its entry of counts[2]
//   mesh_vertex_kernel    rank = workgroup offset + active cells of the earlier waves + set ballot bits below the lane; stores the
//                         cell's vertex id (-1: inactive) in the map and, if rank < vertex_capacity, the vertex and normal rows
//   mesh_face_kernel      quad rank likewise over the three quad ballots; reads 4 ids from the map, stores 6 indices
// Workspace (tn_mesh_workspace_bytes), G = ceil(cells / 256): G x 4 waves x 4 ballots of 8 B, 2 x G counts of 8 B, cells ids of 4 B.
#include <cmath>
#include "compact_device.h"
#include "grid_device.h"

namespace {

constexpr int THREADS = tn::COMPACT_THREADS; // mark / vertices / faces: 4 waves, one pair of workspace slots per workgroup
constexpr int BALLOTS = 4;                   // per wave: active, quad on axis 0, 1, 2
constexpr int COLUMNS = 2;                   // counts per workgroup: vertices, quads (the three quad ballots summed)
constexpr int SCAN_THREADS = 1024;           // scan: workgroup counts per trip of its loop

struct MeshGrid {
    const float *values;
    int nx, ny, nz;
    float lo[3], h[3];
    float level;
    int64_t cells;
};

// corner d = dx + 2 dy + 4 dz of the cell whose lowest corner is `node`; bit d of the result: inside
__device__ __forceinline__ uint32_t load_corners(const MeshGrid &g, int64_t node, float v[8])
{
    uint32_t in = 0;
    tn::for_corners(g.nx, g.ny, node, [&](int d, int64_t n) {
        v[d] = g.values[n];
        in |= (v[d] >= g.level ? 1u : 0u) << d;
    });
    return in;
}

__global__ __launch_bounds__(THREADS) void mesh_mark_kernel(MeshGrid g, uint64_t *__restrict__ ballots, int64_t *__restrict__ group, int64_t n_groups)
{
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    bool bit[BALLOTS] = {false, false, false, false};            // active, a quad on axis 0 / 1 / 2
    if (c < g.cells) {                                           // (lanes past the last cell stay in the ballots with 0 bits)
        int idx[3];
        int64_t node;
        float v[8];
        tn::cell_of(g.nx, g.ny, (uint32_t)c, idx, node);
        const uint32_t in = load_corners(g, node, v);
        bit[0] = in != 0u && in != 255u;
#pragma unroll
        for (int a = 0; a < 3; ++a) bit[1 + a] = ((in ^ (in >> (1 << a))) & 1u) && idx[(a + 1) % 3] >= 1 && idx[(a + 2) % 3] >= 1;
    }
    tn::compact_mark<BALLOTS, COLUMNS>(bit, ballots, group, n_groups);
}

// workgroup 0 / 1 takes the vertex / quad column of group: counts in, exclusive offsets out; counts[0] = vertices, counts[1] = triangles
// (two per quad).  The columns are independent and a trip is all latency: side by side they take the time of one.
__global__ __launch_bounds__(SCAN_THREADS) void mesh_scan_kernel(int64_t *__restrict__ group, int64_t n_groups, int64_t *__restrict__ counts)
{
    const int64_t column = blockIdx.x;
    tn::scan_group_counts<SCAN_THREADS>(group + column * n_groups, n_groups, counts + column, column + 1);
}

__global__ __launch_bounds__(THREADS) void mesh_vertex_kernel(MeshGrid g, const uint64_t *__restrict__ ballots, const int64_t *__restrict__ group,
                                                              int64_t capacity, float *__restrict__ vertices, float *__restrict__ normals,
                                                              int32_t *__restrict__ map)
{
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= g.cells) return;
    const int64_t rank = tn::compact_rank<BALLOTS>(ballots, group, 0);
    map[c] = (int32_t)rank;                                      // (-1: inactive; whatever the capacity: the faces name every vertex)
    if (rank < 0 || rank >= capacity) return;
    int idx[3];
    int64_t node;
    float v[8];
    tn::cell_of(g.nx, g.ny, (uint32_t)c, idx, node);
    const uint32_t in = load_corners(g, node, v);
    float sum[3] = {0.0f, 0.0f, 0.0f};
    int crossed = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ib = (a + 1) % 3, ic = (a + 2) % 3, ob = e & 1, oc = e >> 1;
            const int d0 = (ob << ib) | (oc << ic), d1 = d0 | (1 << a);
            if (((in >> d0) ^ (in >> d1)) & 1u) {
                float t = 0.5f;
                if (isfinite(v[d0]) && isfinite(v[d1])) {
                    t = __fdiv_rn(g.level - v[d0], v[d1] - v[d0]);
                    t = fminf(fmaxf(t, 0.0f), 1.0f);
                }
                sum[a] += t;
                sum[ib] += (float)ob;
                sum[ic] += (float)oc;
                ++crossed;
            }
        }
    }
    float u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k] = __fdiv_rn(sum[k], (float)crossed);
        vertices[3 * rank + k] = fmaf((float)idx[k] + u[k], g.h[k], g.lo[k]);
    }
    if (normals == nullptr) return;
    float grad[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int ib = (a + 1) % 3, ic = (a + 2) % 3;
        const float ub = u[ib], uc = u[ic], nb = 1.0f - ub, nc = 1.0f - uc;
        const int s = 1 << a, sb = 1 << ib, sc = 1 << ic;
        const float d = (v[s] - v[0]) * (nb * nc) + (v[s | sb] - v[sb]) * (ub * nc) + (v[s | sc] - v[sc]) * (nb * uc) + (v[s | sb | sc] - v[sb | sc]) * (ub * uc);
        grad[a] = __fdiv_rn(d, g.h[a]);
    }
    const float len = sqrtf(grad[0] * grad[0] + grad[1] * grad[1] + grad[2] * grad[2]);
    const bool ok = len > 0.0f && isfinite(len);                 // (NaN fails the first test)
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[3 * rank + k] = ok ? __fdiv_rn(-grad[k], len) : 0.0f;
}

__global__ __launch_bounds__(THREADS) void mesh_face_kernel(MeshGrid g, const uint64_t *__restrict__ ballots, const int64_t *__restrict__ group,
                                                            int64_t n_groups, int64_t capacity, const int32_t *__restrict__ map,
                                                            int32_t *__restrict__ faces)
{
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= g.cells) return;
    uint32_t quads;                                              // bit a: this cell has a quad on axis a
    int64_t rank = tn::compact_rank<BALLOTS, 3>(ballots, group + n_groups, 1, &quads);
    if (rank < 0) return;
    int idx[3];
    int64_t node;
    tn::cell_of(g.nx, g.ny, (uint32_t)c, idx, node);
    const bool lower_inside = g.values[node] >= g.level;
    const int64_t stride[3] = {1, g.nx, (int64_t)g.nx * g.ny};     // of the cell index (a quad's axes b, c have idx >= 1: no wrap)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((quads >> a) & 1)) continue;
        const int64_t sb = stride[(a + 1) % 3], sc = stride[(a + 2) % 3];
        int32_t q0 = map[c - sb - sc], q1 = map[c - sc], q2 = map[c], q3 = map[c - sb];
        if (!lower_inside) {
            int32_t t = q0;
            q0 = q3, q3 = t;
            t = q1, q1 = q2, q2 = t;
        }
        const int64_t row = 2 * rank;
        if (row < capacity) faces[3 * row] = q0, faces[3 * row + 1] = q1, faces[3 * row + 2] = q2;
        if (row + 1 < capacity) faces[3 * row + 3] = q0, faces[3 * row + 4] = q2, faces[3 * row + 5] = q3;
        ++rank;
    }
}

__global__ __launch_bounds__(THREADS) void grid_nodes_kernel(MeshGrid g, int64_t first, int64_t n, float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= n) return;
    float x[3];
    tn::node_position<int64_t>(first + t, (int64_t)g.nx + 1, (int64_t)g.ny + 1, g.lo, g.h, x);      // (64-bit: a grid's nodes can pass 2^31)
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * t + a] = x[a];
}

MeshGrid grid_of(const float *values, const int32_t *dims, const float *lo, const float *h, float level, int64_t cells)
{
    MeshGrid g;
    g.values = values;
    g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
    for (int a = 0; a < 3; ++a) g.lo[a] = lo[a], g.h[a] = h[a];
    g.level = level;
    g.cells = cells;
    return g;
}

}  // namespace

extern "C" int tn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t *bytes)
{
    TN_REQUIRE(bytes, TN_E_NULL, "tn_mesh_workspace_bytes: null pointer");
    const int32_t dims[3] = {nx, ny, nz};
    const int64_t cells = tn::grid_count(dims, false);
    TN_REQUIRE(cells >= 0, TN_E_SIZE, "tn_mesh_workspace_bytes: dims must be >= 0 with fewer than 2^31 cells");
    *bytes = tn::compact_bytes<BALLOTS, COLUMNS>(tn::ceil_div(cells, THREADS)) + 8 * tn::ceil_div(cells, 2);
    return TN_OK;
}

extern "C" int tn_grid_nodes(const float *lo, const float *h, const int32_t *dims, int64_t first, int64_t n, float *out, void *stream)
{
    TN_REQUIRE(lo && h && dims, TN_E_NULL, "tn_grid_nodes: null pointer (lo, h, dims)");
    const int64_t cells = tn::grid_count(dims, false);
    TN_REQUIRE(cells >= 0, TN_E_SIZE, "tn_grid_nodes: dims must be >= 0 with fewer than 2^31 cells");
    const int64_t nodes = ((int64_t)dims[0] + 1) * ((int64_t)dims[1] + 1) * ((int64_t)dims[2] + 1);      // (< 2^34, or 2^62 with an empty axis)
    TN_REQUIRE(first >= 0 && n >= 0 && n <= nodes && first <= nodes - n, TN_E_SIZE, "tn_grid_nodes: first .. first + n must lie inside the grid's nodes");
    if (n == 0) return TN_OK;
    TN_REQUIRE(out, TN_E_NULL, "tn_grid_nodes: null pointer (out)");
    TN_REQUIRE(tn::ceil_div(n, THREADS) < ((int64_t)1 << 31), TN_E_SIZE, "tn_grid_nodes: n must be below 2^39");
    const MeshGrid g = grid_of(nullptr, dims, lo, h, 0.0f, cells);
    grid_nodes_kernel<<<dim3((unsigned)tn::ceil_div(n, THREADS)), dim3(THREADS), 0, (hipStream_t)stream>>>(g, first, n, out);
    return tn::check_launch("grid_nodes_kernel");
}

extern "C" int tn_mesh_extract(const float *values, const int32_t *dims, const float *lo, const float *h, float level, int64_t vertex_capacity,
                               int64_t face_capacity, float *vertices, float *normals, int32_t *faces, int64_t *counts, void *workspace,
                               void *stream)
{
    TN_REQUIRE(dims && lo && h, TN_E_NULL, "tn_mesh_extract: null pointer (dims, lo, h)");
    const int64_t cells = tn::grid_count(dims, false);
    TN_REQUIRE(cells >= 0, TN_E_SIZE, "tn_mesh_extract: dims must be >= 0 with fewer than 2^31 cells (vertex ids are int32)");
    TN_REQUIRE(vertex_capacity >= 0 && face_capacity >= 0, TN_E_SIZE, "tn_mesh_extract: negative capacity");
    TN_REQUIRE(std::isfinite(level), TN_E_CONFIG, "tn_mesh_extract: level must be finite");
    TN_REQUIRE(counts, TN_E_NULL, "tn_mesh_extract: null pointer (counts)");
    TN_REQUIRE(vertex_capacity == 0 || vertices, TN_E_NULL, "tn_mesh_extract: null output pointer (vertices) with vertex_capacity > 0");
    TN_REQUIRE(face_capacity == 0 || faces, TN_E_NULL, "tn_mesh_extract: null output pointer (faces) with face_capacity > 0");
    hipStream_t s = (hipStream_t)stream;
    if (cells == 0) return tn::zero_bytes(counts, 2 * sizeof(int64_t), s, "tn_mesh_extract");
    TN_REQUIRE(values && workspace, TN_E_NULL, "tn_mesh_extract: null pointer (values, workspace)");
    TN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)counts & 7) == 0, TN_E_ALIGN, "tn_mesh_extract: workspace and counts must be 8-byte aligned");
    const MeshGrid g = grid_of(values, dims, lo, h, level, cells);
    const int64_t n_groups = tn::ceil_div(cells, THREADS);
    uint64_t *ballots = (uint64_t *)workspace;
    int64_t *group = tn::compact_group<BALLOTS>(workspace, n_groups);
    int32_t *map = (int32_t *)(group + COLUMNS * n_groups);
    mesh_mark_kernel<<<dim3((unsigned)n_groups), dim3(THREADS), 0, s>>>(g, ballots, group, n_groups);
    int rc = tn::check_launch("mesh_mark_kernel");
    if (rc != TN_OK) return rc;
    mesh_scan_kernel<<<dim3(COLUMNS), dim3(SCAN_THREADS), 0, s>>>(group, n_groups, counts);
    rc = tn::check_launch("mesh_scan_kernel");
    if (rc != TN_OK || (vertex_capacity == 0 && face_capacity == 0)) return rc;
    mesh_vertex_kernel<<<dim3((unsigned)n_groups), dim3(THREADS), 0, s>>>(g, ballots, group, vertex_capacity, vertices, normals, map);
    rc = tn::check_launch("mesh_vertex_kernel");
    if (rc != TN_OK || face_capacity == 0) return rc;
    mesh_face_kernel<<<dim3((unsigned)n_groups), dim3(THREADS), 0, s>>>(g, ballots, group, n_groups, face_capacity, map, faces);
    return tn::check_launch("mesh_face_kernel");
}
