// Taubin smoothing of an indexed triangle mesh, the vertex adjacency it runs on and the vertex normals of the smoothed faces,
// on the device.  No reference call site: the reference renders images and exports no geometry.
//
// Definition (include/tinynerf_hip.h has it in full):
//   a face takes part when its three indices lie in [0, V) and are pairwise different; vertex v's row holds one pair (a, b) -- the
//   face's other two corners in its cyclic order after v -- per participating face that names v, in ascending face id;
//   offsets = the exclusive prefix sums of the row lengths d(v); pinned[v] = 1 when d(v) == 0 or some id of the row does not occur
//   exactly twice in it; stats = (participating faces, vertices with pinned == 0, the largest d)
//   pass: out[v] = in[v] + f (c - in[v]), c = (the fp32 sum of the row's 2 d positions in row order) / (2 d), for the vertices that move
//   normals: g(v) = the sum over the row, in row order, of (p[a] - p[v]) x (p[b] - p[v]); n = g / |g|, else the fallback row
//
// tn_mesh_adjacency -- a memset and nine launches on the caller's stream, no host read-back:
//   adjacency_degree_kernel   one lane per face: integer atomicAdd of its three corners into cursor[v] (zeroed by the memset)
//   adjacency_group_kernel    per workgroup of 256 vertices: the sum of their degrees -> group[g]
//   adjacency_scan_kernel     one workgroup: group -> exclusive offsets (compact_device.h's scan, 1024 workgroups per trip)
//   adjacency_offsets_kernel  offsets[v] = group[g] + the degrees before v in its workgroup; offsets[V]; pinned[v] = (d == 0); cursor[v] = 0
//   adjacency_fill_kernel     one lane per face: corner 3 f + k goes to slot offsets[v] + atomicAdd(cursor[v], 1) of `corner`
//   adjacency_order_kernel    one lane per slot: the rank of its corner id among its row's -> the pair (a, b) to pairs[offsets[v] + rank]
//   adjacency_pin_kernel      one lane per slot: its pair's two ids counted over the row; a count other than 2 stores pinned[v] = 1
//   adjacency_stats_kernel    per workgroup of 256 vertices: free vertices, the largest degree -> two partials
//   adjacency_reduce_kernel   one workgroup adds / maximises the partials in a fixed order -> stats[3]
// The atomics decide the ROUTE, not the result: integer sums do not depend on the order of their operands, and the slot an atomic
// hands a corner only says where in `corner` the row's ids lie before they are ranked -- a row's corner ids are distinct, so the
// ranks are a permutation whatever that order was.  pinned[v] = 1 is a plain store of one value by every lane that finds a reason.
// Ranking and counting cost d reads per slot, d^2 per row: quadratic in the degree, spread over the row's d lanes.
// Workspace (tn_mesh_adjacency_workspace_bytes), G = ceil(V / 256): G sums of 8 B, 2 G partials of 8 B, V cursors of 4 B, 3 F corner
// ids of 4 B (both rounded up to 8 B).  Every word is written before it is read.
//
// tn_mesh_smooth_pass / tn_mesh_vertex_normals -- one launch each, one lane per vertex, no atomics; tn_mesh_smooth enqueues 2 N passes.
#include "compact_device.h"

namespace {

constexpr int THREADS = tn::COMPACT_THREADS; // every kernel but the two single-workgroup ones: 4 waves
constexpr int WAVES = THREADS / TN_WAVE;
constexpr int SCAN_THREADS = 1024;           // scan / reduce: workgroup values per trip of the loop

// the three indices of face f and whether it takes part: all in [0, V), pairwise different (a (-1,-1,-1) row fails the first)
__device__ __forceinline__ bool load_face(const int32_t *__restrict__ faces, int64_t f, int32_t n_vertices, int32_t v[3])
{
    v[0] = faces[3 * f], v[1] = faces[3 * f + 1], v[2] = faces[3 * f + 2];
    const bool inside = (uint32_t)v[0] < (uint32_t)n_vertices && (uint32_t)v[1] < (uint32_t)n_vertices && (uint32_t)v[2] < (uint32_t)n_vertices;
    return inside && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
}

__global__ __launch_bounds__(THREADS) void adjacency_degree_kernel(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_vertices,
                                                                   int32_t *__restrict__ cursor)
{
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    if (!load_face(faces, f, n_vertices, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(cursor + v[k], 1);
}

__global__ __launch_bounds__(THREADS) void adjacency_group_kernel(const int32_t *__restrict__ cursor, int64_t n_vertices, int64_t *__restrict__ group)
{
    __shared__ int32_t wave_part[WAVES];
    const int tid = (int)threadIdx.x;
    const int64_t v = (int64_t)blockIdx.x * THREADS + tid;
    const int32_t s = tn::wave_sum(v < n_vertices ? cursor[v] : 0);
    if (tn::lane_id() == 0) wave_part[tid / TN_WAVE] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) total += wave_part[w];
        group[blockIdx.x] = total;
    }
}

// (the total, 3 F' < 2^31, goes to offsets[V] from the offsets kernel: *count lands in the first partial, which the stats kernel rewrites)
__global__ __launch_bounds__(SCAN_THREADS) void adjacency_scan_kernel(int64_t *__restrict__ group, int64_t n_groups, int64_t *__restrict__ count)
{
    tn::scan_group_counts<SCAN_THREADS>(group, n_groups, count);
}

__global__ __launch_bounds__(THREADS) void adjacency_offsets_kernel(int32_t *__restrict__ cursor, int64_t n_vertices, const int64_t *__restrict__ group,
                                                                    int32_t *__restrict__ offsets, uint8_t *__restrict__ pinned)
{
    __shared__ int32_t wave_total[WAVES];
    const int tid = (int)threadIdx.x, wave = tid / TN_WAVE;
    const int64_t v = (int64_t)blockIdx.x * THREADS + tid;
    const int32_t d = v < n_vertices ? cursor[v] : 0;
    const int32_t s = tn::wave_scan(d);
    if (tn::lane_id() == TN_WAVE - 1) wave_total[wave] = s;
    __syncthreads();
    if (v >= n_vertices) return;
    int32_t before = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) before += w < wave ? wave_total[w] : 0;
    const int32_t first = (int32_t)group[blockIdx.x] + before + (s - d);
    offsets[v] = first;
    if (v == n_vertices - 1) offsets[n_vertices] = first + d;
    pinned[v] = d == 0 ? 1 : 0;
    cursor[v] = 0;
}

__global__ __launch_bounds__(THREADS) void adjacency_fill_kernel(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_vertices,
                                                                 const int32_t *__restrict__ offsets, int32_t *__restrict__ cursor,
                                                                 int32_t *__restrict__ corner)
{
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    if (!load_face(faces, f, n_vertices, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) corner[offsets[v[k]] + atomicAdd(cursor + v[k], 1)] = (int32_t)(3 * f + k);      // (below the row's end: the degree kernel counted this corner)
}

// slot s of `corner` lies in the row of the vertex its corner names; that row's bounds
__device__ __forceinline__ int32_t row_of_slot(const int32_t *__restrict__ faces, const int32_t *__restrict__ offsets, int32_t c, int32_t *first, int32_t *last)
{
    const int32_t v = faces[c];                                    // (faces [F,3] flat: corner c = 3 f + k is its entry c)
    *first = offsets[v], *last = offsets[v + 1];
    return v;
}

__global__ __launch_bounds__(THREADS) void adjacency_order_kernel(const int32_t *__restrict__ faces, const int32_t *__restrict__ offsets, int64_t n_vertices,
                                                                  const int32_t *__restrict__ corner, int32_t *__restrict__ pairs)
{
    const int64_t s = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (s >= offsets[n_vertices]) return;
    const int32_t c = corner[s];
    int32_t first, last;
    row_of_slot(faces, offsets, c, &first, &last);
    int32_t rank = 0;
    for (int32_t j = first; j < last; ++j) rank += corner[j] < c ? 1 : 0;
    const int32_t f = c / 3, k = c - 3 * f;
    const int64_t row = (int64_t)first + rank;
    pairs[2 * row] = faces[3 * (int64_t)f + (k + 1) % 3];
    pairs[2 * row + 1] = faces[3 * (int64_t)f + (k + 2) % 3];
}

__global__ __launch_bounds__(THREADS) void adjacency_pin_kernel(const int32_t *__restrict__ faces, const int32_t *__restrict__ offsets, int64_t n_vertices,
                                                                const int32_t *__restrict__ corner, const int32_t *__restrict__ pairs,
                                                                uint8_t *__restrict__ pinned)
{
    const int64_t s = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (s >= offsets[n_vertices]) return;
    int32_t first, last;
    const int32_t v = row_of_slot(faces, offsets, corner[s], &first, &last);
    const int32_t a = pairs[2 * s], b = pairs[2 * s + 1];
    int32_t count_a = 0, count_b = 0;
    for (int64_t j = 2 * (int64_t)first; j < 2 * (int64_t)last; ++j) {
        const int32_t id = pairs[j];
        count_a += id == a ? 1 : 0, count_b += id == b ? 1 : 0;
    }
    if (count_a != 2 || count_b != 2) pinned[v] = 1;               // (every writer stores the same byte)
}

__global__ __launch_bounds__(THREADS) void adjacency_stats_kernel(const int32_t *__restrict__ offsets, const uint8_t *__restrict__ pinned, int64_t n_vertices,
                                                                  int64_t *__restrict__ partial)
{
    __shared__ int32_t wave_free[WAVES], wave_largest[WAVES];
    const int tid = (int)threadIdx.x, wave = tid / TN_WAVE;
    const int64_t v = (int64_t)blockIdx.x * THREADS + tid;
    const bool live = v < n_vertices;
    const uint64_t free_lanes = __ballot(live && pinned[v] == 0);
    int32_t largest = live ? offsets[v + 1] - offsets[v] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, __shfl_xor(largest, o, TN_WAVE));
    if (tn::lane_id() == 0) wave_free[wave] = __popcll(free_lanes), wave_largest[wave] = largest;
    __syncthreads();
    if (tid == 0) {
        int32_t n = 0, m = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) n += wave_free[w], m = max(m, wave_largest[w]);
        partial[2 * (int64_t)blockIdx.x] = n, partial[2 * (int64_t)blockIdx.x + 1] = m;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void adjacency_reduce_kernel(const int64_t *__restrict__ partial, int64_t n_groups, const int32_t *__restrict__ offsets,
                                                                        int64_t n_vertices, int64_t *__restrict__ stats)
{
    __shared__ int64_t part[2][SCAN_THREADS];
    const int tid = (int)threadIdx.x;
    int64_t n = 0, m = 0;
    for (int64_t i = tid; i < n_groups; i += SCAN_THREADS) n += partial[2 * i], m = max(m, partial[2 * i + 1]);
    part[0][tid] = n, part[1][tid] = m;
    __syncthreads();
    for (int s = SCAN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) part[0][tid] += part[0][tid + s], part[1][tid] = max(part[1][tid], part[1][tid + s]);
        __syncthreads();
    }
    if (tid == 0) stats[0] = offsets[n_vertices] / 3, stats[1] = part[0][0], stats[2] = part[1][0];
}

// every vertex without faces: offsets 0, pinned 1 (F == 0)
__global__ __launch_bounds__(THREADS) void adjacency_empty_kernel(int64_t n_vertices, int32_t *__restrict__ offsets, uint8_t *__restrict__ pinned)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v > n_vertices) return;
    offsets[v] = 0;
    if (v < n_vertices) pinned[v] = 1;
}

__global__ __launch_bounds__(THREADS) void smooth_pass_kernel(const float *__restrict__ in, const int32_t *__restrict__ offsets, const int32_t *__restrict__ pairs,
                                                              const uint8_t *__restrict__ pinned, int64_t n_vertices, float factor, float *__restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const int32_t first = offsets[v], d = offsets[v + 1] - first;
    const float px = in[3 * v], py = in[3 * v + 1], pz = in[3 * v + 2];
    if (d <= 0 || (pinned != nullptr && pinned[v] != 0)) {          // does not move: the row bit for bit
        out[3 * v] = px, out[3 * v + 1] = py, out[3 * v + 2] = pz;
        return;
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int64_t j = 2 * (int64_t)first; j < 2 * ((int64_t)first + d); ++j) {
        const int64_t q = pairs[j];
        sx += in[3 * q], sy += in[3 * q + 1], sz += in[3 * q + 2];
    }
    const float n = (float)(2 * (int64_t)d);
    out[3 * v] = fmaf(factor, sx / n - px, px);
    out[3 * v + 1] = fmaf(factor, sy / n - py, py);
    out[3 * v + 2] = fmaf(factor, sz / n - pz, pz);
}

__global__ __launch_bounds__(THREADS) void vertex_normals_kernel(const float *__restrict__ vertices, const int32_t *__restrict__ offsets,
                                                                 const int32_t *__restrict__ pairs, int64_t n_vertices, const float *__restrict__ fallback,
                                                                 float *__restrict__ normals)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const int32_t first = offsets[v], last = offsets[v + 1];
    const float px = vertices[3 * v], py = vertices[3 * v + 1], pz = vertices[3 * v + 2];
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    for (int64_t j = first; j < last; ++j) {
        const int64_t a = pairs[2 * j], b = pairs[2 * j + 1];
        const float ex = vertices[3 * a] - px, ey = vertices[3 * a + 1] - py, ez = vertices[3 * a + 2] - pz;
        const float fx = vertices[3 * b] - px, fy = vertices[3 * b + 1] - py, fz = vertices[3 * b + 2] - pz;
        gx = fmaf(-ez, fy, fmaf(ey, fz, gx));
        gy = fmaf(-ex, fz, fmaf(ez, fx, gy));
        gz = fmaf(-ey, fx, fmaf(ex, fy, gz));
    }
    const float length = sqrtf(fmaf(gx, gx, fmaf(gy, gy, gz * gz)));
    float nx, ny, nz;
    if (last > first && length > 0.0f && length <= 3.402823466e+38f) {      // (NaN fails both comparisons)
        nx = gx / length, ny = gy / length, nz = gz / length;
    } else if (fallback != nullptr) {
        nx = fallback[3 * v], ny = fallback[3 * v + 1], nz = fallback[3 * v + 2];
    } else {
        nx = ny = nz = 0.0f;
    }
    normals[3 * v] = nx, normals[3 * v + 1] = ny, normals[3 * v + 2] = nz;
}

bool sizes_ok(int64_t n_vertices, int64_t n_faces)
{
    const int64_t limit = (int64_t)1 << 31;
    return n_vertices >= 0 && n_faces >= 0 && n_vertices < limit && n_faces < limit && 3 * n_faces < limit;
}

bool finite(float x) { return __builtin_isfinite(x); }

bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

int launch_pass(const float *in, const int32_t *offsets, const int32_t *pairs, const uint8_t *pinned, int64_t n_vertices, float factor, float *out,
                hipStream_t s)
{
    smooth_pass_kernel<<<dim3((unsigned)tn::ceil_div(n_vertices, THREADS)), dim3(THREADS), 0, s>>>(in, offsets, pairs, pinned, n_vertices, factor, out);
    return tn::check_launch("smooth_pass_kernel");
}

}  // namespace

extern "C" int tn_mesh_adjacency_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t *bytes)
{
    TN_REQUIRE(bytes, TN_E_NULL, "tn_mesh_adjacency_workspace_bytes: null pointer");
    TN_REQUIRE(sizes_ok(n_vertices, n_faces), TN_E_SIZE, "tn_mesh_adjacency_workspace_bytes: sizes must be >= 0, V and 3 F below 2^31");
    *bytes = 3 * 8 * tn::ceil_div(n_vertices, THREADS) + 8 * tn::ceil_div(n_vertices, 2) + 8 * tn::ceil_div(3 * n_faces, 2);
    return TN_OK;
}

extern "C" int tn_mesh_adjacency(const int32_t *faces, int64_t n_vertices, int64_t n_faces, int32_t *offsets, int32_t *pairs, uint8_t *pinned,
                                 int64_t *stats, void *workspace, void *stream)
{
    TN_REQUIRE(sizes_ok(n_vertices, n_faces), TN_E_SIZE,
               "tn_mesh_adjacency: n_vertices and n_faces must be >= 0, n_vertices and 3 n_faces below 2^31 (vertex ids and row offsets are int32)");
    TN_REQUIRE(stats, TN_E_NULL, "tn_mesh_adjacency: null pointer (stats)");
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices == 0) return tn::zero_bytes(stats, 3 * sizeof(int64_t), s, "tn_mesh_adjacency");
    TN_REQUIRE(offsets && pinned && workspace, TN_E_NULL, "tn_mesh_adjacency: null pointer (offsets, pinned, workspace)");
    TN_REQUIRE(n_faces == 0 || (faces && pairs), TN_E_NULL, "tn_mesh_adjacency: null pointer (faces, pairs) with n_faces > 0");
    TN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, TN_E_ALIGN, "tn_mesh_adjacency: workspace and stats must be 8-byte aligned");
    TN_REQUIRE(aligned4(faces) && aligned4(offsets) && aligned4(pairs), TN_E_ALIGN, "tn_mesh_adjacency: faces, offsets and pairs must be 4-byte aligned");
    const int64_t vertex_groups = tn::ceil_div(n_vertices, THREADS), face_groups = tn::ceil_div(n_faces, THREADS);
    const int64_t slot_groups = tn::ceil_div(3 * n_faces, THREADS);
    int64_t *group = (int64_t *)workspace, *partial = group + vertex_groups;
    int32_t *cursor = (int32_t *)(partial + 2 * vertex_groups);
    int32_t *corner = cursor + 2 * tn::ceil_div(n_vertices, 2);
    const dim3 block(THREADS);
    int rc;
    if (n_faces == 0) {
        adjacency_empty_kernel<<<dim3((unsigned)tn::ceil_div(n_vertices + 1, THREADS)), block, 0, s>>>(n_vertices, offsets, pinned);
        rc = tn::check_launch("adjacency_empty_kernel");
        if (rc != TN_OK) return rc;
    } else {
        rc = tn::zero_bytes(cursor, 4 * (size_t)n_vertices, s, "tn_mesh_adjacency");
        if (rc != TN_OK) return rc;
        adjacency_degree_kernel<<<dim3((unsigned)face_groups), block, 0, s>>>(faces, n_faces, (int32_t)n_vertices, cursor);
        rc = tn::check_launch("adjacency_degree_kernel");
        if (rc != TN_OK) return rc;
        adjacency_group_kernel<<<dim3((unsigned)vertex_groups), block, 0, s>>>(cursor, n_vertices, group);
        rc = tn::check_launch("adjacency_group_kernel");
        if (rc != TN_OK) return rc;
        adjacency_scan_kernel<<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(group, vertex_groups, partial);
        rc = tn::check_launch("adjacency_scan_kernel");
        if (rc != TN_OK) return rc;
        adjacency_offsets_kernel<<<dim3((unsigned)vertex_groups), block, 0, s>>>(cursor, n_vertices, group, offsets, pinned);
        rc = tn::check_launch("adjacency_offsets_kernel");
        if (rc != TN_OK) return rc;
        adjacency_fill_kernel<<<dim3((unsigned)face_groups), block, 0, s>>>(faces, n_faces, (int32_t)n_vertices, offsets, cursor, corner);
        rc = tn::check_launch("adjacency_fill_kernel");
        if (rc != TN_OK) return rc;
        adjacency_order_kernel<<<dim3((unsigned)slot_groups), block, 0, s>>>(faces, offsets, n_vertices, corner, pairs);
        rc = tn::check_launch("adjacency_order_kernel");
        if (rc != TN_OK) return rc;
        adjacency_pin_kernel<<<dim3((unsigned)slot_groups), block, 0, s>>>(faces, offsets, n_vertices, corner, pairs, pinned);
        rc = tn::check_launch("adjacency_pin_kernel");
        if (rc != TN_OK) return rc;
    }
    adjacency_stats_kernel<<<dim3((unsigned)vertex_groups), block, 0, s>>>(offsets, pinned, n_vertices, partial);
    rc = tn::check_launch("adjacency_stats_kernel");
    if (rc != TN_OK) return rc;
    adjacency_reduce_kernel<<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(partial, vertex_groups, offsets, n_vertices, stats);
    return tn::check_launch("adjacency_reduce_kernel");
}

extern "C" int tn_mesh_smooth_pass(const float *in, const int32_t *offsets, const int32_t *pairs, const uint8_t *pinned, int64_t n_vertices, float factor,
                                   float *out, void *stream)
{
    TN_REQUIRE(sizes_ok(n_vertices, 0), TN_E_SIZE, "tn_mesh_smooth_pass: n_vertices must be >= 0 and below 2^31");
    TN_REQUIRE(finite(factor), TN_E_CONFIG, "tn_mesh_smooth_pass: the factor must be finite");
    TN_REQUIRE(in == nullptr || in != out, TN_E_CONFIG, "tn_mesh_smooth_pass: out must not alias in (every lane reads its neighbours' rows)");
    if (n_vertices == 0) return TN_OK;
    TN_REQUIRE(in && offsets && pairs && out, TN_E_NULL, "tn_mesh_smooth_pass: null pointer (in, offsets, pairs, out)");
    TN_REQUIRE(aligned4(in) && aligned4(offsets) && aligned4(pairs) && aligned4(out), TN_E_ALIGN, "tn_mesh_smooth_pass: pointers must be 4-byte aligned");
    return launch_pass(in, offsets, pairs, pinned, n_vertices, factor, out, (hipStream_t)stream);
}

extern "C" int tn_mesh_smooth(const float *vertices, const int32_t *offsets, const int32_t *pairs, const uint8_t *pinned, int64_t n_vertices,
                              int32_t iterations, float lambda, float mu, float *scratch, float *out, void *stream)
{
    TN_REQUIRE(sizes_ok(n_vertices, 0) && iterations >= 0, TN_E_SIZE, "tn_mesh_smooth: n_vertices must be >= 0 and below 2^31, iterations >= 0");
    TN_REQUIRE(finite(lambda) && finite(mu), TN_E_CONFIG, "tn_mesh_smooth: lambda and mu must be finite");
    TN_REQUIRE((vertices == nullptr || (vertices != out && vertices != scratch)) && (out == nullptr || out != scratch), TN_E_CONFIG,
               "tn_mesh_smooth: vertices, scratch and out must not alias each other (the passes go to and fro between scratch and out)");
    if (n_vertices == 0) return TN_OK;
    TN_REQUIRE(vertices && offsets && pairs && scratch && out, TN_E_NULL, "tn_mesh_smooth: null pointer (vertices, offsets, pairs, scratch, out)");
    TN_REQUIRE(aligned4(vertices) && aligned4(offsets) && aligned4(pairs) && aligned4(scratch) && aligned4(out), TN_E_ALIGN,
               "tn_mesh_smooth: pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (iterations == 0) {
        hipError_t e = hipMemcpyAsync(out, vertices, 12 * (size_t)n_vertices, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) {
            tn::set_error("tn_mesh_smooth: %s", hipGetErrorString(e));
            return (int)e;
        }
        return TN_OK;
    }
    const float *from = vertices;
    for (int32_t i = 0; i < iterations; ++i) {                     // lambda into scratch, mu into out: the last pass lands in out
        int rc = launch_pass(from, offsets, pairs, pinned, n_vertices, lambda, scratch, s);
        if (rc != TN_OK) return rc;
        rc = launch_pass(scratch, offsets, pairs, pinned, n_vertices, mu, out, s);
        if (rc != TN_OK) return rc;
        from = out;
    }
    return TN_OK;
}

extern "C" int tn_mesh_vertex_normals(const float *vertices, const int32_t *offsets, const int32_t *pairs, int64_t n_vertices, const float *fallback,
                                      float *normals, void *stream)
{
    TN_REQUIRE(sizes_ok(n_vertices, 0), TN_E_SIZE, "tn_mesh_vertex_normals: n_vertices must be >= 0 and below 2^31");
    if (n_vertices == 0) return TN_OK;
    TN_REQUIRE(vertices && offsets && pairs && normals, TN_E_NULL, "tn_mesh_vertex_normals: null pointer (vertices, offsets, pairs, normals)");
    TN_REQUIRE(aligned4(vertices) && aligned4(offsets) && aligned4(pairs) && aligned4(fallback) && aligned4(normals), TN_E_ALIGN,
               "tn_mesh_vertex_normals: pointers must be 4-byte aligned");
    vertex_normals_kernel<<<dim3((unsigned)tn::ceil_div(n_vertices, THREADS)), dim3(THREADS), 0, (hipStream_t)stream>>>(vertices, offsets, pairs, n_vertices,
                                                                                                                      fallback, normals);
    return tn::check_launch("vertex_normals_kernel");
}
