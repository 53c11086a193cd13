// Connected components of an indexed triangle mesh and the filter that keeps the large ones, on the device.  No reference
// call site: the reference renders images and exports no geometry.
//
// Definition (include/tinynerf_hip.h has it in full) -- integers throughout:
//   a face is valid when its three indices lie in [0, V); two vertices are connected when a valid face names both;
//   label[v] = the smallest vertex id of v's component; face_count[r] = the valid faces whose vertices carry label r (0 unless
//   label[r] == r); stats = (components, components with a face, largest face_count)
//   filter: vertex v is kept when face_count[label[v]] >= T, a valid face when its component is; kept rows keep their order, the
//   k-th kept vertex becomes row k (src[k] = its old id), kept faces are renumbered through the old -> new map
//
// tn_mesh_components -- six launches on the caller's stream, no host read-back:
//   components_init_kernel     labels[v] = v, face_counts[v] = 0
//   components_hook_kernel     one lane per face: a lock-free union-find on labels itself.  find() walks up with path splitting
//                              (atomicMin of the grandparent: a parent only ever decreases); the larger of two roots is linked under
//                              the smaller by atomicCAS(&labels[hi], hi, lo), and a lost race starts again from where it stood
//   components_flatten_kernel  labels[v] = its root
//   components_count_kernel    one lane per face: the lanes of a wave that share a label add their number with one atomicAdd
//   components_stats_kernel    per workgroup of 256 vertices: roots, roots with a face, the largest count -> three partials
//   components_reduce_kernel   one workgroup adds / maximises the partials in a fixed order -> stats[3]
// The atomics decide the ROUTE, not the result: the smaller id always wins, so a component's final root is its minimum whatever the
// interleaving, and integer min and integer sum are order-independent -- the same bytes on every call.  Every shared word of labels is
// read and written with relaxed agent-scope atomics while the hook kernel runs (a plain load may be served a stale line by the XCD's
// L2 for ever; a stale parent is still an ancestor, but a retry loop must see the CAS that beat it).
//
// tn_mesh_filter -- four launches, no atomics, the ballot / scan / ranked-store pattern of mesh.hip (compact_device.h):
//   filter_mark_kernel    lane i takes vertex i and face i: every wave writes 2 ballots (vertex kept, face kept), every workgroup 2 counts
//   filter_scan_kernel    one workgroup per count column: exclusive offsets and its entry of counts[2]
//   filter_vertex_kernel  rank = workgroup offset + kept vertices of the earlier waves + set ballot bits below the lane; stores the
//                         old -> new map (-1: dropped) and, if rank < vertex_capacity, the attribute rows and src
//   filter_face_kernel    rank likewise over the face ballots; stores the three indices renumbered through the map
// Workspace (tn_mesh_filter_workspace_bytes), G = ceil(max(V, F) / 256): G x 4 waves x 2 ballots of 8 B, 2 x G counts of 8 B, V ids of 4 B.
#include "compact_device.h"

namespace {

constexpr int THREADS = tn::COMPACT_THREADS; // every kernel but the two single-workgroup ones: 4 waves
constexpr int WAVES = THREADS / TN_WAVE;
constexpr int BALLOTS = 2;                   // per wave: vertex kept, face kept -- and a count column for each
constexpr int SCAN_THREADS = 1024;           // scan / reduce: workgroup values per trip of the loop

__device__ __forceinline__ int32_t load_label(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool valid_id(int32_t i, int32_t n_vertices) { return (uint32_t)i < (uint32_t)n_vertices; }

// the three indices of face f and whether all lie in [0, V)
__device__ __forceinline__ bool load_face(const int32_t *__restrict__ faces, int64_t f, int32_t n_vertices, int32_t v[3])
{
    v[0] = faces[3 * f], v[1] = faces[3 * f + 1], v[2] = faces[3 * f + 2];
    return valid_id(v[0], n_vertices) && valid_id(v[1], n_vertices) && valid_id(v[2], n_vertices);
}

// the root above x as far as this lane can see; every node passed is re-hung under its grandparent (labels[x] <= x always, so the
// walk strictly descends and ends)
__device__ __forceinline__ int32_t find_root(int32_t *labels, int32_t x)
{
    int32_t p = load_label(labels + x);
    while (p != x) {
        const int32_t g = load_label(labels + p);
        if (g != p) atomicMin(labels + x, g);
        x = p, p = g;
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t *labels, int32_t a, int32_t b)
{
    while (true) {
        a = find_root(labels, a), b = find_root(labels, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(labels + hi, hi, lo) == hi) return;
        a = hi, b = lo;                                            // hi got a parent meanwhile: on from there (lock-free: some CAS won)
    }
}

__global__ __launch_bounds__(THREADS) void components_init_kernel(int32_t *__restrict__ labels, int32_t *__restrict__ face_counts, int64_t n_vertices)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    labels[v] = (int32_t)v;
    face_counts[v] = 0;
}

__global__ __launch_bounds__(THREADS) void components_hook_kernel(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_vertices, int32_t *labels)
{
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    if (!load_face(faces, f, n_vertices, v)) return;
    if (v[0] != v[1]) unite(labels, v[0], v[1]);
    if (v[1] != v[2]) unite(labels, v[1], v[2]);
}

// (labels[v] turns from an ancestor into the root under other lanes' walks: either value leads to the same root, and roots stay)
__global__ __launch_bounds__(THREADS) void components_flatten_kernel(int32_t *labels, int64_t n_vertices)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    int32_t r = (int32_t)v, p = load_label(labels + r);
    while (p != r) r = p, p = load_label(labels + r);
    __hip_atomic_store(labels + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(THREADS) void components_count_kernel(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_vertices,
                                                                   const int32_t *__restrict__ labels, int32_t *__restrict__ face_counts)
{
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    int32_t v[3];
    bool open = f < n_faces && load_face(faces, f, n_vertices, v);
    const int32_t label = open ? labels[v[0]] : -1;
    // a mesh in extraction order has a few labels per wave: one add per label, not 64 into one address
    for (uint64_t todo = __ballot(open); todo != 0; todo = __ballot(open)) {
        const int32_t first = __shfl(label, __ffsll((unsigned long long)todo) - 1, TN_WAVE);
        const bool mine = open && label == first;
        const uint64_t same = __ballot(mine);
        if (mine && tn::rank_below(same) == 0) atomicAdd(face_counts + first, (int32_t)__popcll(same));
        open = open && !mine;
    }
}

__global__ __launch_bounds__(THREADS) void components_stats_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ face_counts,
                                                                   int64_t n_vertices, int64_t *__restrict__ partial)
{
    __shared__ int32_t wave_roots[WAVES], wave_faced[WAVES], wave_largest[WAVES];
    const int tid = (int)threadIdx.x, wave = tid / TN_WAVE;
    const int64_t v = (int64_t)blockIdx.x * THREADS + tid;
    const bool root = v < n_vertices && labels[v] == (int32_t)v;
    const int32_t count = root ? face_counts[v] : 0;
    const uint64_t roots = __ballot(root), faced = __ballot(count > 0);
    int32_t largest = count;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, __shfl_xor(largest, o, TN_WAVE));
    if (tn::lane_id() == 0) wave_roots[wave] = __popcll(roots), wave_faced[wave] = __popcll(faced), wave_largest[wave] = largest;
    __syncthreads();
    if (tid == 0) {
        int32_t r = 0, n = 0, m = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) r += wave_roots[w], n += wave_faced[w], m = max(m, wave_largest[w]);
        partial[3 * (int64_t)blockIdx.x] = r, partial[3 * (int64_t)blockIdx.x + 1] = n, partial[3 * (int64_t)blockIdx.x + 2] = m;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void components_reduce_kernel(const int64_t *__restrict__ partial, int64_t n_groups, int64_t *__restrict__ stats)
{
    __shared__ int64_t part[3][SCAN_THREADS];
    const int tid = (int)threadIdx.x;
    int64_t r = 0, n = 0, m = 0;
    for (int64_t i = tid; i < n_groups; i += SCAN_THREADS) r += partial[3 * i], n += partial[3 * i + 1], m = max(m, partial[3 * i + 2]);
    part[0][tid] = r, part[1][tid] = n, part[2][tid] = m;
    __syncthreads();
    for (int s = SCAN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) part[0][tid] += part[0][tid + s], part[1][tid] += part[1][tid + s], part[2][tid] = max(part[2][tid], part[2][tid + s]);
        __syncthreads();
    }
    if (tid < 3) stats[tid] = part[tid][0];
}

struct FilterMesh {
    const int32_t *faces, *labels, *face_counts;
    int64_t n_vertices, n_faces, threshold;
};

// (labels are tn_mesh_components': an id outside [0, V) -- not one of its labels -- drops the vertex rather than being read through)
__device__ __forceinline__ bool vertex_kept(const FilterMesh &m, int32_t v)
{
    const int32_t label = m.labels[v];
    return valid_id(label, (int32_t)m.n_vertices) && (int64_t)m.face_counts[label] >= m.threshold;
}

__global__ __launch_bounds__(THREADS) void filter_mark_kernel(FilterMesh m, uint64_t *__restrict__ ballots, int64_t *__restrict__ group, int64_t n_groups)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    bool keep[BALLOTS] = {i < m.n_vertices && vertex_kept(m, (int32_t)i), false};      // vertex i, face i
    if (i < m.n_faces) {                                           // (lanes past the last vertex / face stay in the ballots with 0 bits)
        int32_t v[3];
        keep[1] = load_face(m.faces, i, (int32_t)m.n_vertices, v) && vertex_kept(m, v[0]);
    }
    tn::compact_mark<BALLOTS, BALLOTS>(keep, ballots, group, n_groups);
}

// workgroup 0 / 1 takes the vertex / face column of group: counts in, exclusive offsets out; counts[0] = kept vertices, counts[1] = kept faces
__global__ __launch_bounds__(SCAN_THREADS) void filter_scan_kernel(int64_t *__restrict__ group, int64_t n_groups, int64_t *__restrict__ counts)
{
    const int64_t column = blockIdx.x;
    tn::scan_group_counts<SCAN_THREADS>(group + column * n_groups, n_groups, counts + column);
}

__global__ __launch_bounds__(THREADS) void filter_vertex_kernel(int64_t n_vertices, const uint64_t *__restrict__ ballots, const int64_t *__restrict__ group,
                                                                int64_t capacity, const float *__restrict__ vertices, const float *__restrict__ normals,
                                                                const uint8_t *__restrict__ colors, float *__restrict__ out_vertices,
                                                                float *__restrict__ out_normals, uint8_t *__restrict__ out_colors,
                                                                int32_t *__restrict__ src, int32_t *__restrict__ map)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const int64_t rank = tn::compact_rank<BALLOTS>(ballots, group, 0);
    map[v] = (int32_t)rank;                                        // (whatever the capacity: the kept faces name every kept vertex)
    if (rank < 0 || rank >= capacity) return;
    src[rank] = (int32_t)v;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_vertices[3 * rank + k] = vertices[3 * v + k];
        if (normals != nullptr) out_normals[3 * rank + k] = normals[3 * v + k];
        if (colors != nullptr) out_colors[3 * rank + k] = colors[3 * v + k];
    }
}

__global__ __launch_bounds__(THREADS) void filter_face_kernel(const int32_t *__restrict__ faces, int64_t n_faces, const uint64_t *__restrict__ ballots,
                                                              const int64_t *__restrict__ group, int64_t n_groups, int64_t capacity,
                                                              const int32_t *__restrict__ map, int32_t *__restrict__ out_faces)
{
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t rank = tn::compact_rank<BALLOTS>(ballots, group + n_groups, 1);
    if (rank < 0 || rank >= capacity) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * rank + k] = map[faces[3 * f + k]];      // (a kept face is valid: its ids lie in [0, V))
}

bool sizes_ok(int64_t n_vertices, int64_t n_faces)
{
    const int64_t limit = (int64_t)1 << 31;
    return n_vertices >= 0 && n_faces >= 0 && n_vertices < limit && n_faces < limit;
}

}  // namespace

extern "C" int tn_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t *bytes)
{
    TN_REQUIRE(bytes, TN_E_NULL, "tn_mesh_components_workspace_bytes: null pointer");
    TN_REQUIRE(sizes_ok(n_vertices, n_faces), TN_E_SIZE, "tn_mesh_components_workspace_bytes: sizes must be >= 0 and below 2^31");
    *bytes = 3 * 8 * tn::ceil_div(n_vertices, THREADS);
    return TN_OK;
}

extern "C" int tn_mesh_components(const int32_t *faces, int64_t n_vertices, int64_t n_faces, int32_t *labels, int32_t *face_counts, int64_t *stats,
                                  void *workspace, void *stream)
{
    TN_REQUIRE(sizes_ok(n_vertices, n_faces), TN_E_SIZE, "tn_mesh_components: n_vertices and n_faces must be >= 0 and below 2^31 (vertex ids are int32)");
    TN_REQUIRE(stats, TN_E_NULL, "tn_mesh_components: null pointer (stats)");
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices == 0) return tn::zero_bytes(stats, 3 * sizeof(int64_t), s, "tn_mesh_components");
    TN_REQUIRE(labels && face_counts && workspace, TN_E_NULL, "tn_mesh_components: null pointer (labels, face_counts, workspace)");
    TN_REQUIRE(n_faces == 0 || faces, TN_E_NULL, "tn_mesh_components: null pointer (faces) with n_faces > 0");
    TN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, TN_E_ALIGN, "tn_mesh_components: workspace and stats must be 8-byte aligned");
    const int64_t vertex_groups = tn::ceil_div(n_vertices, THREADS), face_groups = tn::ceil_div(n_faces, THREADS);
    int64_t *partial = (int64_t *)workspace;
    components_init_kernel<<<dim3((unsigned)vertex_groups), dim3(THREADS), 0, s>>>(labels, face_counts, n_vertices);
    int rc = tn::check_launch("components_init_kernel");
    if (rc != TN_OK) return rc;
    if (n_faces > 0) {
        components_hook_kernel<<<dim3((unsigned)face_groups), dim3(THREADS), 0, s>>>(faces, n_faces, (int32_t)n_vertices, labels);
        rc = tn::check_launch("components_hook_kernel");
        if (rc != TN_OK) return rc;
        components_flatten_kernel<<<dim3((unsigned)vertex_groups), dim3(THREADS), 0, s>>>(labels, n_vertices);
        rc = tn::check_launch("components_flatten_kernel");
        if (rc != TN_OK) return rc;
        components_count_kernel<<<dim3((unsigned)face_groups), dim3(THREADS), 0, s>>>(faces, n_faces, (int32_t)n_vertices, labels, face_counts);
        rc = tn::check_launch("components_count_kernel");
        if (rc != TN_OK) return rc;
    }
    components_stats_kernel<<<dim3((unsigned)vertex_groups), dim3(THREADS), 0, s>>>(labels, face_counts, n_vertices, partial);
    rc = tn::check_launch("components_stats_kernel");
    if (rc != TN_OK) return rc;
    components_reduce_kernel<<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(partial, vertex_groups, stats);
    return tn::check_launch("components_reduce_kernel");
}

extern "C" int tn_mesh_filter_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t *bytes)
{
    TN_REQUIRE(bytes, TN_E_NULL, "tn_mesh_filter_workspace_bytes: null pointer");
    TN_REQUIRE(sizes_ok(n_vertices, n_faces), TN_E_SIZE, "tn_mesh_filter_workspace_bytes: sizes must be >= 0 and below 2^31");
    *bytes = tn::compact_bytes<BALLOTS, BALLOTS>(tn::ceil_div(n_vertices > n_faces ? n_vertices : n_faces, THREADS)) + 8 * tn::ceil_div(n_vertices, 2);
    return TN_OK;
}

extern "C" int tn_mesh_filter(const int32_t *faces, const int32_t *labels, const int32_t *face_counts, int64_t threshold, const float *vertices,
                              const float *normals, const uint8_t *colors, int64_t n_vertices, int64_t n_faces, int64_t vertex_capacity,
                              int64_t face_capacity, float *out_vertices, float *out_normals, uint8_t *out_colors, int32_t *src, int32_t *out_faces,
                              int64_t *counts, void *workspace, void *stream)
{
    TN_REQUIRE(sizes_ok(n_vertices, n_faces), TN_E_SIZE, "tn_mesh_filter: n_vertices and n_faces must be >= 0 and below 2^31 (vertex ids are int32)");
    TN_REQUIRE(vertex_capacity >= 0 && face_capacity >= 0, TN_E_SIZE, "tn_mesh_filter: negative capacity");
    TN_REQUIRE(threshold >= 0, TN_E_CONFIG, "tn_mesh_filter: threshold must be >= 0");
    TN_REQUIRE(counts, TN_E_NULL, "tn_mesh_filter: null pointer (counts)");
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices == 0) return tn::zero_bytes(counts, 2 * sizeof(int64_t), s, "tn_mesh_filter");
    TN_REQUIRE(labels && face_counts && workspace, TN_E_NULL, "tn_mesh_filter: null pointer (labels, face_counts, workspace)");
    TN_REQUIRE(n_faces == 0 || faces, TN_E_NULL, "tn_mesh_filter: null pointer (faces) with n_faces > 0");
    TN_REQUIRE(vertex_capacity == 0 || (vertices && out_vertices && src), TN_E_NULL,
               "tn_mesh_filter: null pointer (vertices, out_vertices, src) with vertex_capacity > 0");
    TN_REQUIRE(vertex_capacity == 0 || ((!normals || out_normals) && (!colors || out_colors)), TN_E_NULL,
               "tn_mesh_filter: null output pointer (out_normals, out_colors) for an input that is given, with vertex_capacity > 0");
    TN_REQUIRE(face_capacity == 0 || out_faces, TN_E_NULL, "tn_mesh_filter: null output pointer (out_faces) with face_capacity > 0");
    TN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)counts & 7) == 0, TN_E_ALIGN, "tn_mesh_filter: workspace and counts must be 8-byte aligned");
    const int64_t vertex_groups = tn::ceil_div(n_vertices, THREADS), face_groups = tn::ceil_div(n_faces, THREADS);
    const int64_t n_groups = vertex_groups > face_groups ? vertex_groups : face_groups;
    uint64_t *ballots = (uint64_t *)workspace;
    int64_t *group = tn::compact_group<BALLOTS>(workspace, n_groups);
    int32_t *map = (int32_t *)(group + BALLOTS * n_groups);
    FilterMesh m;
    m.faces = faces, m.labels = labels, m.face_counts = face_counts;
    m.n_vertices = n_vertices, m.n_faces = n_faces, m.threshold = threshold;
    filter_mark_kernel<<<dim3((unsigned)n_groups), dim3(THREADS), 0, s>>>(m, ballots, group, n_groups);
    int rc = tn::check_launch("filter_mark_kernel");
    if (rc != TN_OK) return rc;
    filter_scan_kernel<<<dim3(BALLOTS), dim3(SCAN_THREADS), 0, s>>>(group, n_groups, counts);
    rc = tn::check_launch("filter_scan_kernel");
    if (rc != TN_OK || (vertex_capacity == 0 && face_capacity == 0)) return rc;
    filter_vertex_kernel<<<dim3((unsigned)vertex_groups), dim3(THREADS), 0, s>>>(n_vertices, ballots, group, vertex_capacity, vertices, normals, colors,
                                                                               out_vertices, out_normals, out_colors, src, map);
    rc = tn::check_launch("filter_vertex_kernel");
    if (rc != TN_OK || face_capacity == 0 || n_faces == 0) return rc;
    filter_face_kernel<<<dim3((unsigned)face_groups), dim3(THREADS), 0, s>>>(faces, n_faces, ballots, group, n_groups, face_capacity, map, out_faces);
    return tn::check_launch("filter_face_kernel");
}
