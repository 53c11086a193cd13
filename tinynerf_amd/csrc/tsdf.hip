// Fusion of rendered depth maps into a truncated signed distance field on tn_mesh_extract's grid, and the mask that keeps the
// extractor's faces out of cells no view has observed.  No reference call site: the reference renders images and exports
// no geometry.
//
// Definition (include/tinynerf_hip.h has it in full) -- fp32 throughout, every fused multiply-add an explicit fmaf:
//   node x_c = fmaf((float)idx_c, h_c, lo_c); per view, in ascending order:
//     p = x - t, q = R^T p, z = -q_z > 0, (x', y') = (q_x, -q_y) / z                      camera frame, image axes y down
//     (xd, yd) = the lens' forward model of (x', y'); skip unless 1 + 3 k1 s + 5 k2 s^2 + 7 k3 s^3 + 9 k4 s^4 > 0
//     (u, v) = (fx xd + cx, fy yd + cy) inside [0, w) x [0, h); g = pixel_offset + floor(v) w + floor(u)
//     D = depth[g] finite and > 0 (and opacity[g] >= min_opacity); sdf = D - |p| >= -trunc;  S += min(sdf / trunc, 1), W += 1
//
// tn_tsdf_integrate -- one launch: one lane per node (i fastest), 256 per workgroup, the loop over the views inside the kernel.  A
//   view's table row (pose, lens, model, size, offset: 26 dwords) has a wave-uniform address and is read with scalar loads; what
//   varies per lane is the node and the pixel it lands on.  Neighbouring nodes land on neighbouring pixels, so a wave's depth gather
//   touches a few cache lines of one map.  No atomics: the lane owns its node's S and W, reads them once, adds the views in order
//   and writes them once -- a range of views in one call and the same range split over calls give the same bytes.
// tn_tsdf_mask_faces -- two launches: per cell whose id in the extractor's map is >= 0, observed[id] = all 8 corner weights > 0;
//   per face, (-1, -1, -1) when an index lies outside [0, V) or names a vertex that is not observed.
//
// The colour volume: four floats per node, C = (sum w r, sum w g, sum w b, sum w).  After the same steps 1-5 -- written
// once below, tsdf_view_pixel, for both passes -- a view inside the band -trunc <= sdf <= trunc adds the pixel's colour with the
// background taken out again (tn_points_compact's colour) at the weight w = 1 - |sdf| / trunc.
// tn_tsdf_integrate_color -- tn_tsdf_integrate's launch shape; the lane reads its node's accumulators as one 16-byte load before the
//   loop and writes them once after it; per contributing view three gathers (depth, opacity, 12 B of rgb).  No atomics.
// tn_tsdf_sample_colors -- one launch, one lane per point: the trilinear interpolant of the cell's 8 corners, numerators and
//   denominator apart, then their quotient; corners without colour have weight 0 and drop out of the average.
#include <cmath>
#include "grid_device.h"

namespace {

constexpr int THREADS = 256;

struct TsdfGrid {
    int sx, sy;                      // nodes on x and y: nx + 1, ny + 1
    int64_t nodes;
    float lo[3], h[3];
    float trunc, min_opacity;
};

// 1 + s (c1 + s (c2 + s (c3 + s c4)))
__device__ __forceinline__ float poly4(float s, float c1, float c2, float c3, float c4)
{
    return fmaf(s, fmaf(s, fmaf(s, fmaf(s, c4, c3), c2), c1), 1.0f);
}

// the camera table's columns as the kernels read them: read-only for the launch, and `view` is the same in every lane, so a view's row
// has a wave-uniform address and these become scalar loads
struct TsdfViews {
    const float *__restrict__ c2w, *__restrict__ lens;
    const int32_t *__restrict__ model, *__restrict__ size;
    const int64_t *__restrict__ pixel_offset;
    __device__ explicit TsdfViews(const tn_camera_table &t) : c2w(t.c2w), lens(t.lens), model(t.model), size(t.size), pixel_offset(t.pixel_offset) {}
};

// Steps 1-5 of the per-view update, written once for the geometry and the colour pass: camera frame, lens forward model, monotonicity
// guard, pixel, depth gate and opacity gate.  Returns when this view adds nothing to node x; otherwise calls step6(p, px, D) with
// p = x - t, px the flat pixel the node lands in and D its depth.
template <typename F>
__device__ __forceinline__ void tsdf_view_pixel(const TsdfViews &cams, int view, const float x[3], const float *__restrict__ depth,
                                                const float *__restrict__ opacity, float min_opacity, F step6)
{
    const float *M = cams.c2w + 12 * (int64_t)view;
    const float p0 = x[0] - M[3], p1 = x[1] - M[7], p2 = x[2] - M[11];
    const float z = -fmaf(M[2], p0, fmaf(M[6], p1, M[10] * p2));
    if (!(z > 0.0f)) return;                                      // behind the camera (or NaN)
    const float qx = fmaf(M[0], p0, fmaf(M[4], p1, M[8] * p2)), qy = fmaf(M[1], p0, fmaf(M[5], p1, M[9] * p2));
    const float xu = __fdiv_rn(qx, z), yu = __fdiv_rn(-qy, z);
    const float *L = cams.lens + 10 * (int64_t)view;
    const int model = cams.model[view];
    float xd = xu, yd = yu;
    if (model != TN_LENS_PINHOLE) {
        const float k1 = L[4], k2 = L[5], k3 = L[6], k4 = L[7];
        const float r2 = fmaf(xu, xu, yu * yu);
        float s;                                                  // what the radial polynomial is a polynomial of
        if (model == TN_LENS_OPENCV) {
            const float t1 = L[8], t2 = L[9], xy = xu * yu;
            const float rad = poly4(r2, k1, k2, k3, k4);
            xd = fmaf(xu, rad, fmaf(2.0f * t1, xy, t2 * fmaf(2.0f * xu, xu, r2)));
            yd = fmaf(yu, rad, fmaf(2.0f * t2, xy, t1 * fmaf(2.0f * yu, yu, r2)));
            s = r2;
        } else {
            const float r = sqrtf(r2), theta = atanf(r);
            s = theta * theta;
            const float scale = r > 0.0f ? __fdiv_rn(theta * poly4(s, k1, k2, k3, k4), r) : 1.0f;
            xd = xu * scale, yd = yu * scale;
        }
        if (!(poly4(s, 3.0f * k1, 5.0f * k2, 7.0f * k3, 9.0f * k4) > 0.0f)) return;            // the radial map has turned back here
    }
    const float u = fmaf(L[0], xd, L[2]), v = fmaf(L[1], yd, L[3]);
    const int w = cams.size[2 * view], h = cams.size[2 * view + 1];
    if (!(u >= 0.0f && u < (float)w && v >= 0.0f && v < (float)h)) return;                    // (NaN fails: nothing outside the map is read)
    const int64_t px = cams.pixel_offset[view] + (int64_t)(int)v * w + (int)u;
    const float D = depth[px];
    if (!(D > 0.0f && isfinite(D))) return;
    if (opacity != nullptr && !(opacity[px] >= min_opacity)) return;
    const float p[3] = {p0, p1, p2};
    step6(p, px, D);
}

// |p| of step 6
__device__ __forceinline__ float tsdf_distance(const float p[3]) { return sqrtf(fmaf(p[0], p[0], fmaf(p[1], p[1], p[2] * p[2]))); }

__global__ __launch_bounds__(THREADS) void tsdf_integrate_kernel(tn_camera_table table, const float *__restrict__ depth, const float *__restrict__ opacity,
                                                                 TsdfGrid g, int view_first, int view_count, float *__restrict__ S,
                                                                 float *__restrict__ W)
{
    const int64_t m = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (m >= g.nodes) return;
    float x[3];
    tn::node_position<uint32_t>((uint32_t)m, (uint32_t)g.sx, (uint32_t)g.sy, g.lo, g.h, x);      // (32-bit divisions: nodes < 2^31)
    const TsdfViews cams(table);
    float s_sum = S[m], w_sum = W[m];
    for (int view = view_first; view < view_first + view_count; ++view) {
        tsdf_view_pixel(cams, view, x, depth, opacity, g.min_opacity, [&](const float p[3], int64_t, float D) {
            const float sdf = D - tsdf_distance(p);
            if (sdf < -g.trunc) return;                           // hidden behind the surface in this view
            s_sum += fminf(__fdiv_rn(sdf, g.trunc), 1.0f);
            w_sum += 1.0f;
        });
    }
    S[m] = s_sum;
    W[m] = w_sum;
}

// the colour pass: the node's four accumulators are one 16-byte load before the loop and one 16-byte store after it
__global__ __launch_bounds__(THREADS) void tsdf_integrate_color_kernel(tn_camera_table table, const float *__restrict__ depth,
                                                                       const float *__restrict__ opacity, const float *__restrict__ rgb,
                                                                       const float *__restrict__ bg, TsdfGrid g, int view_first, int view_count,
                                                                       float4 *__restrict__ C)
{
    const int64_t m = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (m >= g.nodes) return;
    float x[3];
    tn::node_position<uint32_t>((uint32_t)m, (uint32_t)g.sx, (uint32_t)g.sy, g.lo, g.h, x);
    const TsdfViews cams(table);
    const float b0 = bg != nullptr ? bg[0] : 0.0f, b1 = bg != nullptr ? bg[1] : 0.0f, b2 = bg != nullptr ? bg[2] : 0.0f;
    float4 acc = C[m];
    for (int view = view_first; view < view_first + view_count; ++view) {
        tsdf_view_pixel(cams, view, x, depth, opacity, g.min_opacity, [&](const float p[3], int64_t px, float D) {
            const float sdf = D - tsdf_distance(p);
            if (!(sdf >= -g.trunc && sdf <= g.trunc)) return;     // outside the band: free space and hidden nodes say nothing about colour
            const float w = 1.0f - __fdiv_rn(fabsf(sdf), g.trunc);
            const float op = opacity != nullptr ? opacity[px] : 1.0f, t = 1.0f - op;
            const float bgc[3] = {b0, b1, b2};
            float c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float u = __fdiv_rn(fmaf(-t, bgc[k], rgb[3 * px + k]), op);
                c[k] = u > 0.0f ? (u < 1.0f ? u : 1.0f) : 0.0f;   // NaN -> 0
            }
            acc.x = fmaf(w, c[0], acc.x), acc.y = fmaf(w, c[1], acc.y), acc.z = fmaf(w, c[2], acc.z);
            acc.w += w;
        });
    }
    C[m] = acc;
}

struct SampleGrid {
    int nx, ny, nz;
    int64_t n;
    float lo[3], h[3];
};

__global__ __launch_bounds__(THREADS) void tsdf_sample_colors_kernel(const float4 *__restrict__ C, SampleGrid g, const float *__restrict__ points,
                                                                     float4 *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= g.n) return;
    const int cells[3] = {g.nx, g.ny, g.nz};
    int idx[3];
    float u[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = points[3 * r + a];
        finite = finite && isfinite(p);
        const float ga = __fdiv_rn(p - g.lo[a], g.h[a]);
        const float cell = fmaxf(floorf(ga), 0.0f);                // (NaN -> 0)
        // (compared as floats so that nothing overflows the int; the index itself is clamped as an int: beyond 2^24 cells on an axis
        //  (float)(n - 1) may round up to n)
        idx[a] = cell < (float)(cells[a] - 1) ? min((int)cell, cells[a] - 1) : cells[a] - 1;
        u[a] = fminf(fmaxf(ga - (float)idx[a], 0.0f), 1.0f);
    }
    const int64_t node = idx[0] + ((int64_t)g.nx + 1) * (idx[1] + ((int64_t)g.ny + 1) * idx[2]);
    float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
    tn::for_corners(g.nx, g.ny, node, [&](int d, int64_t n) {
        const float t = ((d & 1 ? u[0] : 1.0f - u[0]) * (d & 2 ? u[1] : 1.0f - u[1])) * (d & 4 ? u[2] : 1.0f - u[2]);
        const float4 c = C[n];
        num[0] = fmaf(t, c.x, num[0]), num[1] = fmaf(t, c.y, num[1]), num[2] = fmaf(t, c.z, num[2]);
        den = fmaf(t, c.w, den);
    });
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (finite && den > 0.0f) o = make_float4(__fdiv_rn(num[0], den), __fdiv_rn(num[1], den), __fdiv_rn(num[2], den), den);
    out[r] = o;
}

struct MaskGrid {
    int nx, ny;
    int64_t cells;
};

__global__ __launch_bounds__(THREADS) void tsdf_observed_kernel(const float *__restrict__ W, MaskGrid g, const int32_t *__restrict__ cell_ids,
                                                                int32_t n_vertices, uint8_t *__restrict__ observed)
{
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= g.cells) return;
    const int32_t id = cell_ids[c];
    if ((uint32_t)id >= (uint32_t)n_vertices) return;             // -1: no vertex; an id that is not the extractor's writes nothing
    int idx[3];
    int64_t node;
    tn::cell_of(g.nx, g.ny, (uint32_t)c, idx, node);
    bool all = true;
    tn::for_corners(g.nx, g.ny, node, [&](int, int64_t n) { all = all && W[n] > 0.0f; });
    observed[id] = all ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void tsdf_mask_kernel(const uint8_t *__restrict__ observed, int32_t n_vertices, int64_t n_faces,
                                                            int32_t *__restrict__ faces)
{
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_faces) return;
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t v = faces[3 * f + k];
        keep = keep && (uint32_t)v < (uint32_t)n_vertices && observed[(uint32_t)v < (uint32_t)n_vertices ? v : 0] != 0;
    }
    if (!keep) faces[3 * f] = -1, faces[3 * f + 1] = -1, faces[3 * f + 2] = -1;
}

}  // namespace

extern "C" int tn_tsdf_integrate(const tn_camera_table *cams, const float *depth, const float *opacity, float min_opacity, const int32_t *dims,
                                 const float *lo, const float *h, float trunc, int32_t view_first, int32_t view_count, float *S, float *W,
                                 void *stream)
{
    TN_REQUIRE(cams && dims && lo && h, TN_E_NULL, "tn_tsdf_integrate: null pointer (cams, dims, lo, h)");
    const int64_t nodes = tn::grid_count(dims, true);
    TN_REQUIRE(nodes >= 0, TN_E_SIZE, "tn_tsdf_integrate: dims must be >= 0 with fewer than 2^31 nodes");
    TN_REQUIRE(view_first >= 0 && view_count >= 0 && cams->n_img >= 0 && view_count <= cams->n_img && view_first <= cams->n_img - view_count, TN_E_SIZE,
               "tn_tsdf_integrate: view_first .. view_first + view_count must lie inside the camera table");
    TN_REQUIRE(std::isfinite(trunc) && trunc > 0.0f, TN_E_CONFIG, "tn_tsdf_integrate: trunc must be finite and > 0");
    if (view_count == 0 || nodes == 0) return TN_OK;
    TN_REQUIRE(cams->c2w && cams->lens && cams->model && cams->size && cams->pixel_offset, TN_E_NULL,
               "tn_tsdf_integrate: null pointer in the camera table (rgb is not read)");
    TN_REQUIRE(depth && S && W, TN_E_NULL, "tn_tsdf_integrate: null pointer (depth, S, W)");
    TN_REQUIRE(((uintptr_t)depth & 3) == 0 && ((uintptr_t)opacity & 3) == 0 && ((uintptr_t)S & 3) == 0 && ((uintptr_t)W & 3) == 0, TN_E_ALIGN,
               "tn_tsdf_integrate: depth, opacity, S and W must be 4-byte aligned");
    TsdfGrid g;
    g.sx = dims[0] + 1, g.sy = dims[1] + 1;
    g.nodes = nodes;
    for (int a = 0; a < 3; ++a) g.lo[a] = lo[a], g.h[a] = h[a];
    g.trunc = trunc, g.min_opacity = min_opacity;
    tsdf_integrate_kernel<<<dim3((unsigned)tn::ceil_div(nodes, THREADS)), dim3(THREADS), 0, (hipStream_t)stream>>>(*cams, depth, opacity, g, view_first,
                                                                                                           view_count, S, W);
    return tn::check_launch("tsdf_integrate_kernel");
}

extern "C" int tn_tsdf_integrate_color(const tn_camera_table *cams, const float *depth, const float *opacity, float min_opacity, const float *rgb,
                                       const float *bg, const int32_t *dims, const float *lo, const float *h, float trunc, int32_t view_first,
                                       int32_t view_count, float *C, void *stream)
{
    TN_REQUIRE(cams && dims && lo && h, TN_E_NULL, "tn_tsdf_integrate_color: null pointer (cams, dims, lo, h)");
    const int64_t nodes = tn::grid_count(dims, true);
    TN_REQUIRE(nodes >= 0, TN_E_SIZE, "tn_tsdf_integrate_color: dims must be >= 0 with fewer than 2^31 nodes");
    TN_REQUIRE(view_first >= 0 && view_count >= 0 && cams->n_img >= 0 && view_count <= cams->n_img && view_first <= cams->n_img - view_count, TN_E_SIZE,
               "tn_tsdf_integrate_color: view_first .. view_first + view_count must lie inside the camera table");
    TN_REQUIRE(std::isfinite(trunc) && trunc > 0.0f, TN_E_CONFIG, "tn_tsdf_integrate_color: trunc must be finite and > 0");
    TN_REQUIRE(opacity == nullptr || min_opacity > 0.0f, TN_E_CONFIG,
               "tn_tsdf_integrate_color: with an opacity map min_opacity must be > 0 (the colour is divided by the opacity)");
    if (view_count == 0 || nodes == 0) return TN_OK;
    TN_REQUIRE(cams->c2w && cams->lens && cams->model && cams->size && cams->pixel_offset, TN_E_NULL,
               "tn_tsdf_integrate_color: null pointer in the camera table (rgb is not read)");
    TN_REQUIRE(depth && rgb && C, TN_E_NULL, "tn_tsdf_integrate_color: null pointer (depth, rgb, C)");
    TN_REQUIRE(((uintptr_t)depth & 3) == 0 && ((uintptr_t)opacity & 3) == 0 && ((uintptr_t)rgb & 3) == 0 && ((uintptr_t)bg & 3) == 0, TN_E_ALIGN,
               "tn_tsdf_integrate_color: depth, opacity, rgb and bg must be 4-byte aligned");
    TN_REQUIRE(((uintptr_t)C & 15) == 0, TN_E_ALIGN, "tn_tsdf_integrate_color: C must be 16-byte aligned");
    TsdfGrid g;
    g.sx = dims[0] + 1, g.sy = dims[1] + 1;
    g.nodes = nodes;
    for (int a = 0; a < 3; ++a) g.lo[a] = lo[a], g.h[a] = h[a];
    g.trunc = trunc, g.min_opacity = min_opacity;
    tsdf_integrate_color_kernel<<<dim3((unsigned)tn::ceil_div(nodes, THREADS)), dim3(THREADS), 0, (hipStream_t)stream>>>(
        *cams, depth, opacity, rgb, bg, g, view_first, view_count, (float4 *)C);
    return tn::check_launch("tsdf_integrate_color_kernel");
}

extern "C" int tn_tsdf_sample_colors(const float *C, const int32_t *dims, const float *lo, const float *h, const float *points, int64_t n, float *out,
                                     void *stream)
{
    TN_REQUIRE(dims && lo && h, TN_E_NULL, "tn_tsdf_sample_colors: null pointer (dims, lo, h)");
    const int64_t nodes = tn::grid_count(dims, true);
    TN_REQUIRE(nodes >= 0, TN_E_SIZE, "tn_tsdf_sample_colors: dims must be >= 0 with fewer than 2^31 nodes");
    TN_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), TN_E_SIZE, "tn_tsdf_sample_colors: n must be in [0, 2^31)");
    if (n == 0 || nodes == 0) return TN_OK;
    TN_REQUIRE(C && points && out, TN_E_NULL, "tn_tsdf_sample_colors: null pointer (C, points, out)");
    TN_REQUIRE(((uintptr_t)points & 3) == 0, TN_E_ALIGN, "tn_tsdf_sample_colors: points must be 4-byte aligned");
    TN_REQUIRE(((uintptr_t)C & 15) == 0 && ((uintptr_t)out & 15) == 0, TN_E_ALIGN, "tn_tsdf_sample_colors: C and out must be 16-byte aligned");
    SampleGrid g;
    g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
    g.n = n;
    for (int a = 0; a < 3; ++a) g.lo[a] = lo[a], g.h[a] = h[a];
    tsdf_sample_colors_kernel<<<dim3((unsigned)tn::ceil_div(n, THREADS)), dim3(THREADS), 0, (hipStream_t)stream>>>((const float4 *)C, g, points,
                                                                                                           (float4 *)out);
    return tn::check_launch("tsdf_sample_colors_kernel");
}

extern "C" int tn_tsdf_mask_faces(const float *W, const int32_t *dims, const int32_t *cell_ids, int64_t n_vertices, int32_t *faces, int64_t n_faces,
                                  uint8_t *observed, void *stream)
{
    TN_REQUIRE(dims, TN_E_NULL, "tn_tsdf_mask_faces: null pointer (dims)");
    const int64_t cells = tn::grid_count(dims, false), limit = (int64_t)1 << 31;
    TN_REQUIRE(cells >= 0 && tn::grid_count(dims, true) >= 0, TN_E_SIZE, "tn_tsdf_mask_faces: dims must be >= 0 with fewer than 2^31 nodes");
    TN_REQUIRE(n_vertices >= 0 && n_faces >= 0 && n_vertices < limit && n_faces < limit, TN_E_SIZE,
               "tn_tsdf_mask_faces: n_vertices and n_faces must be >= 0 and below 2^31 (vertex ids are int32)");
    if (n_faces == 0) return TN_OK;
    TN_REQUIRE(faces, TN_E_NULL, "tn_tsdf_mask_faces: null pointer (faces)");
    TN_REQUIRE(n_vertices == 0 || observed, TN_E_NULL, "tn_tsdf_mask_faces: null pointer (observed)");
    TN_REQUIRE(n_vertices == 0 || cells == 0 || (W && cell_ids), TN_E_NULL, "tn_tsdf_mask_faces: null pointer (W, cell_ids)");
    TN_REQUIRE(((uintptr_t)W & 3) == 0 && ((uintptr_t)cell_ids & 3) == 0 && ((uintptr_t)faces & 3) == 0, TN_E_ALIGN,
               "tn_tsdf_mask_faces: W, cell_ids and faces must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices > 0) {
        if (int rc = tn::zero_bytes(observed, (size_t)n_vertices, s, "tn_tsdf_mask_faces")) return rc;      // a vertex no cell names is not observed
        if (cells > 0) {
            MaskGrid g;
            g.nx = dims[0], g.ny = dims[1];
            g.cells = cells;
            tsdf_observed_kernel<<<dim3((unsigned)tn::ceil_div(cells, THREADS)), dim3(THREADS), 0, s>>>(W, g, cell_ids, (int32_t)n_vertices, observed);
            const int rc = tn::check_launch("tsdf_observed_kernel");
            if (rc != TN_OK) return rc;
        }
    }
    tsdf_mask_kernel<<<dim3((unsigned)tn::ceil_div(n_faces, THREADS)), dim3(THREADS), 0, s>>>(observed, (int32_t)n_vertices, n_faces, faces);
    return tn::check_launch("tsdf_mask_kernel");
}
