// Rays of photographed scenes, made on the fly from a camera table: what tn_gather_rays reads from three fp32 tables of
// 36 B per pixel, tn_camera_rays computes from 96 B per IMAGE (pose, lens, size) and 3 B per pixel (8-bit colour).
//
// Ray i belongs to flat pixel g = first + stride * (idx ? idx[i] : i) of the split; its image is found by binary search in
// pixel_offset (n_img + 1 entries, a few hundred: they sit in cache), its pixel (u, v) row-major inside the image.
//
// Lens models -- the OpenCV / COLMAP definitions, image axes x right / y down, camera axes x right / y up / looking down -z:
//   xd = (u + 0.5 - cx) / fx,  yd = (v + 0.5 - cy) / fy
//   0 pinhole:  (x, y) = (xd, yd)
//   1 OpenCV:   (x, y) solves  xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2),
//               rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3 + k4 r2^4,  r2 = x^2 + y^2          (Newton, analytic 2 x 2 Jacobian, start (xd, yd))
//   2 fisheye:  theta_d = |(xd, yd)|,  theta solves theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)   (Newton from theta_d)
//               camera direction (xd s, -yd s, -cos theta),  s = sin(theta) / theta_d  (1 at the centre)
//   pinhole / OpenCV camera direction: (x, -y, -1).
//   out_d = R dir / |R dir|  (ONE normalisation, as the reference's data.py:52-70 does for its pinhole), out_o = the translation
//   column, bit for bit; out_rgb = float(byte) / 255 with a correctly rounded division.
// Newton runs a FIXED number of iterations (no data-dependent exit: a wave whose lanes sit on different pixels does not diverge in the
// loop; once converged a further iteration moves the iterate by an ulp at most).  A lens model that is not invertible at a pixel can end
// anywhere; if the direction that comes out is not finite, the pixel gets its pinhole direction: the outputs are always finite and unit.
//
// Layout: one lane per ray; a workgroup of 256 stages its 256 x 3 outputs of each array in LDS (stride 3 floats: no bank conflict) and
// writes them back as 3 x 256 consecutive dwords per array, the store pattern of gather_rays_kernel.
#include "tn_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int NEWTON_ITERS = 8;      // fp32 is converged after 4 on every lens of the tests; 8 leaves a margin for stronger lenses

__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

__global__ __launch_bounds__(THREADS) void camera_rays_kernel(tn_camera_table cams, const int32_t *__restrict__ idx, int64_t first, int64_t stride,
                                                              int64_t n, float *__restrict__ out_o, float *__restrict__ out_d,
                                                              float *__restrict__ out_rgb)
{
    __shared__ float so[3 * THREADS], sd[3 * THREADS], sc[3 * THREADS];
    const int tid = (int)threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * THREADS + tid;
    const bool colours = out_rgb != nullptr;
    if (r < n) {
        int64_t g = first + stride * (idx != nullptr ? (int64_t)idx[r] : r);
        g = min(max(g, (int64_t)0), cams.n_pixels - 1);          // an index outside the table (idx is not checked on the host) reads its nearest pixel, never outside the table
        int lo = 0, hi = cams.n_img;                              // pixel_offset[lo] <= g < pixel_offset[hi]; the trip count depends on n_img alone
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cams.pixel_offset[mid] <= g) lo = mid; else hi = mid;
        }
        const int img = lo;
        const int64_t p = g - cams.pixel_offset[img];
        const int w = max(cams.size[2 * img], 1);
        int u, v;
        if ((uint64_t)p <= 0xffffffffull) {                       // (every real image: a 32-bit division)
            const uint32_t q = (uint32_t)p / (uint32_t)w;
            v = (int)q;
            u = (int)((uint32_t)p - q * (uint32_t)w);
        } else {
            const int64_t q = p / w;
            v = (int)q;
            u = (int)(p - q * w);
        }
        const float *L = cams.lens + 10 * (int64_t)img;
        const float fx = L[0], fy = L[1], cx = L[2], cy = L[3], k1 = L[4], k2 = L[5], k3 = L[6], k4 = L[7], p1 = L[8], p2 = L[9];
        const float xd = ((float)u + 0.5f - cx) / fx, yd = ((float)v + 0.5f - cy) / fy;
        const int model = cams.model[img];
        float dx = xd, dy = -yd, dz = -1.0f;                      // pinhole
        if (model == 1) {
            float x = xd, y = yd;
#pragma unroll
            for (int it = 0; it < NEWTON_ITERS; ++it) {
                const float xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
                const float rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)));
                const float dr = k1 + r2 * (2.0f * k2 + r2 * (3.0f * k3 + r2 * (4.0f * k4)));      // d rad / d r2
                const float f1 = x * rad + 2.0f * p1 * xy + p2 * (r2 + 2.0f * xx) - xd;
                const float f2 = y * rad + 2.0f * p2 * xy + p1 * (r2 + 2.0f * yy) - yd;
                const float j11 = rad + 2.0f * xx * dr + 2.0f * p1 * y + 6.0f * p2 * x;
                const float j12 = 2.0f * xy * dr + 2.0f * p1 * x + 2.0f * p2 * y;                  // = j21
                const float j22 = rad + 2.0f * yy * dr + 2.0f * p2 * x + 6.0f * p1 * y;
                const float inv = 1.0f / (j11 * j22 - j12 * j12);
                x -= (j22 * f1 - j12 * f2) * inv;
                y -= (j11 * f2 - j12 * f1) * inv;
            }
            dx = x; dy = -y;
        } else if (model == 2) {
            const float td = sqrtf(xd * xd + yd * yd);
            float th = td;
#pragma unroll
            for (int it = 0; it < NEWTON_ITERS; ++it) {
                const float t2 = th * th;
                const float f = th * (1.0f + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td;
                const float df = 1.0f + t2 * (3.0f * k1 + t2 * (5.0f * k2 + t2 * (7.0f * k3 + t2 * (9.0f * k4))));
                th -= f / df;
            }
            const float s = td > 1e-20f ? sinf(th) / td : 1.0f;
            dx = xd * s; dy = -yd * s; dz = -cosf(th);
        }
        const float *M = cams.c2w + 12 * (int64_t)img;
        const float r00 = M[0], r01 = M[1], r02 = M[2], r10 = M[4], r11 = M[5], r12 = M[6], r20 = M[8], r21 = M[9], r22 = M[10];
        float wx = r00 * dx + r01 * dy + r02 * dz, wy = r10 * dx + r11 * dy + r12 * dz, wz = r20 * dx + r21 * dy + r22 * dz;
        float s = 1.0f / sqrtf(wx * wx + wy * wy + wz * wz);
        wx *= s; wy *= s; wz *= s;
        if (!finite3(wx, wy, wz)) {                               // the lens model is not invertible here: the pixel's pinhole direction
            dx = xd; dy = -yd; dz = -1.0f;
            wx = r00 * dx + r01 * dy + r02 * dz; wy = r10 * dx + r11 * dy + r12 * dz; wz = r20 * dx + r21 * dy + r22 * dz;
            s = 1.0f / sqrtf(wx * wx + wy * wy + wz * wz);
            wx *= s; wy *= s; wz *= s;
        }
        so[3 * tid] = M[3]; so[3 * tid + 1] = M[7]; so[3 * tid + 2] = M[11];
        sd[3 * tid] = wx; sd[3 * tid + 1] = wy; sd[3 * tid + 2] = wz;
        if (colours) {
            const uint8_t *c = cams.rgb + 3 * g;
            sc[3 * tid] = __fdiv_rn((float)c[0], 255.0f);
            sc[3 * tid + 1] = __fdiv_rn((float)c[1], 255.0f);
            sc[3 * tid + 2] = __fdiv_rn((float)c[2], 255.0f);
        }
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (3 * THREADS), total = 3 * n;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = k * THREADS + tid;
        if (base + e < total) {
            out_o[base + e] = so[e];
            out_d[base + e] = sd[e];
            if (colours) out_rgb[base + e] = sc[e];
        }
    }
}

}  // namespace

extern "C" int tn_camera_rays(const tn_camera_table *cams, const int32_t *idx, int64_t first, int64_t stride, int64_t n, float *out_o,
                              float *out_d, float *out_rgb, void *stream)
{
    TN_REQUIRE(n >= 0, TN_E_SIZE, "tn_camera_rays: negative size");
    if (n == 0) return TN_OK;
    TN_REQUIRE(cams && out_o && out_d, TN_E_NULL, "tn_camera_rays: null pointer");
    TN_REQUIRE(cams->c2w && cams->lens && cams->model && cams->size && cams->pixel_offset && (!out_rgb || cams->rgb), TN_E_NULL,
               "tn_camera_rays: null pointer in the camera table (out_rgb needs the table's colours)");
    TN_REQUIRE(cams->n_img >= 1 && cams->n_pixels >= 1, TN_E_SIZE, "tn_camera_rays: empty camera table");
    TN_REQUIRE(n <= ((int64_t)1 << 38), TN_E_SIZE, "tn_camera_rays: too many rays for one launch");
    if (idx == nullptr) {                                         // the whole range is known here: it must lie inside the table
        int64_t span, last;
        TN_REQUIRE(!__builtin_mul_overflow(stride, n - 1, &span) && !__builtin_add_overflow(first, span, &last) && first >= 0 &&
                       first < cams->n_pixels && last >= 0 && last < cams->n_pixels,
                   TN_E_SIZE, "tn_camera_rays: first + stride * (n - 1) lies outside the table");
    }
    camera_rays_kernel<<<dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream>>>(*cams, idx, first, stride, n, out_o,
                                                                                                                out_d, out_rgb);
    return tn::check_launch("camera_rays_kernel");
}
