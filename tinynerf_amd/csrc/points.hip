// Coloured point cloud of rendered rays: filter, back-projection and order-preserving compaction of the per-ray maps of
// tn_ray_maps, kept on the device.  No reference call site: the reference renders images and exports no geometry.
//
// Definition (include/tinynerf_hip.h has it in full) -- fp32 throughout, every fused multiply-add an explicit fmaf:
//   p_c  = fmaf(depth_i, d_ic, o_ic)                                         (d is used as given, not normalised)
//   keep = opacity_i >= min_opacity  &&  depth_i > 0 and finite  &&  p finite  &&  (no box  ||  lo_c <= p_c <= hi_c on every axis)
//   u_c  = fmaf(-(1 - opacity_i), bg_c, rgb_ic) / opacity_i   (correctly rounded division),  c = clamp(u_c, 0, 1) with NaN -> 0,
//   byte = (uint8_t)fmaf(c, 255, 0.5)
// The k-th kept ray, in ray order, writes row k of points / colors / src while k < capacity; *count = the number of kept rays.
//
// Three launches on the caller's stream, one lane per ray, no atomics -- the same bytes on every call (the pattern's pieces: compact_device.h):
//   points_mark_kernel    evaluates the predicate; every wave writes its 64-bit ballot, every workgroup of 256 its number of kept rays
//   points_scan_kernel    ONE workgroup turns the workgroup counts into exclusive offsets, 1024 at a time with a carry, and writes *count
//   points_write_kernel   rank = workgroup offset + kept rays of the workgroup's earlier waves + set ballot bits below the lane; a kept
//                         lane recomputes its point and colour and stores row `rank` (12 + 3 + 4 B) if rank < capacity
// Workspace, G = ceil(n / 256): G x 4 waves x 1 ballot of 8 B, then G workgroup counts of 8 B (tn_points_workspace_bytes).
#include "compact_device.h"

namespace {

constexpr int THREADS = tn::COMPACT_THREADS; // mark / write: 4 waves, one workspace slot per workgroup
constexpr int SCAN_THREADS = 1024;           // scan: workgroup counts per trip of its loop

struct PointsArgs {
    const float *rays_o, *rays_d, *rgb, *opacity, *depth, *bg, *box;
    float min_opacity;
    int64_t n;
};

__device__ __forceinline__ void point_of(const PointsArgs &a, int64_t r, float depth, float p[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = fmaf(depth, a.rays_d[3 * r + c], a.rays_o[3 * r + c]);
}

__device__ __forceinline__ bool keeps(const PointsArgs &a, int64_t r)
{
    const float op = a.opacity[r], depth = a.depth[r];
    if (!(op >= a.min_opacity) || !(depth > 0.0f) || !isfinite(depth)) return false;
    float p[3];
    point_of(a, r, depth, p);
    bool keep = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    if (a.box != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) keep = keep && a.box[c] <= p[c] && p[c] <= a.box[3 + c];
    }
    return keep;
}

__global__ __launch_bounds__(THREADS) void points_mark_kernel(PointsArgs a, uint64_t *__restrict__ ballots, int64_t *__restrict__ group)
{
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool keep[1] = {r < a.n && keeps(a, r)};               // (lanes past n stay in the ballot with a 0 bit)
    tn::compact_mark<1, 1>(keep, ballots, group, gridDim.x);
}

// group[0..n_groups): counts in, exclusive offsets out (a total stays below 2^31: n does)
__global__ __launch_bounds__(SCAN_THREADS) void points_scan_kernel(int64_t *__restrict__ group, int64_t n_groups, int64_t *__restrict__ count)
{
    tn::scan_group_counts<SCAN_THREADS>(group, n_groups, count);
}

__global__ __launch_bounds__(THREADS) void points_write_kernel(PointsArgs a, const uint64_t *__restrict__ ballots, const int64_t *__restrict__ group,
                                                               int64_t capacity, float *__restrict__ points, uint8_t *__restrict__ colors,
                                                               int32_t *__restrict__ src)
{
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= a.n) return;
    const int64_t rank = tn::compact_rank<1>(ballots, group, 0);
    if (rank < 0 || rank >= capacity) return;
    const float op = a.opacity[r];
    float p[3];
    point_of(a, r, a.depth[r], p);
    const float t = 1.0f - op;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float u = __fdiv_rn(fmaf(-t, a.bg != nullptr ? a.bg[c] : 0.0f, a.rgb[3 * r + c]), op);
        const float v = u > 0.0f ? (u < 1.0f ? u : 1.0f) : 0.0f;         // NaN -> 0
        points[3 * rank + c] = p[c];
        colors[3 * rank + c] = (uint8_t)fmaf(v, 255.0f, 0.5f);
    }
    src[rank] = (int32_t)r;
}

}  // namespace

extern "C" int tn_points_workspace_bytes(int64_t n, int64_t *bytes)
{
    TN_REQUIRE(bytes, TN_E_NULL, "tn_points_workspace_bytes: null pointer");
    TN_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), TN_E_SIZE, "tn_points_workspace_bytes: n must be in [0, 2^31)");
    *bytes = tn::compact_bytes<1, 1>(tn::ceil_div(n, THREADS));
    return TN_OK;
}

extern "C" int tn_points_compact(const float *rays_o, const float *rays_d, const float *rgb, const float *opacity, const float *depth,
                                 const float *bg, const float *box, float min_opacity, int64_t n, int64_t capacity, float *points,
                                 uint8_t *colors, int32_t *src, int64_t *count, void *workspace, void *stream)
{
    TN_REQUIRE(n >= 0 && capacity >= 0, TN_E_SIZE, "tn_points_compact: negative size");
    TN_REQUIRE(n < ((int64_t)1 << 31), TN_E_SIZE, "tn_points_compact: src is int32, n must be below 2^31");
    TN_REQUIRE(min_opacity > 0.0f, TN_E_CONFIG, "tn_points_compact: min_opacity must be > 0 (the colour is divided by the opacity)");
    TN_REQUIRE(count, TN_E_NULL, "tn_points_compact: null pointer (count)");
    TN_REQUIRE(capacity == 0 || (points && colors && src), TN_E_NULL, "tn_points_compact: null output pointer with capacity > 0");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return tn::zero_bytes(count, sizeof(int64_t), s, "tn_points_compact");
    TN_REQUIRE(rays_o && rays_d && rgb && opacity && depth && workspace, TN_E_NULL, "tn_points_compact: null pointer");
    TN_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)count & 7) == 0, TN_E_ALIGN, "tn_points_compact: workspace and count must be 8-byte aligned");
    const PointsArgs a = {rays_o, rays_d, rgb, opacity, depth, bg, box, min_opacity, n};
    const int64_t n_groups = tn::ceil_div(n, THREADS);
    uint64_t *ballots = (uint64_t *)workspace;
    int64_t *group = tn::compact_group<1>(workspace, n_groups);
    points_mark_kernel<<<dim3((unsigned)n_groups), dim3(THREADS), 0, s>>>(a, ballots, group);
    int rc = tn::check_launch("points_mark_kernel");
    if (rc != TN_OK) return rc;
    points_scan_kernel<<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(group, n_groups, count);
    rc = tn::check_launch("points_scan_kernel");
    if (rc != TN_OK || capacity == 0) return rc;
    points_write_kernel<<<dim3((unsigned)n_groups), dim3(THREADS), 0, s>>>(a, ballots, group, capacity, points, colors, src);
    return tn::check_launch("points_write_kernel");
}
