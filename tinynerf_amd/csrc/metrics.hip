// Image metrics of the evaluation harness: single-scale SSIM (Wang et al. 2004) of two [H, W, C] float images.
//
// Definition (the form of the NeRF evaluation scripts: TensoRF / K-Planes rgb_ssim, skimage's structural_similarity with
// gaussian_weights=True, use_sample_covariance=False):
//   window 11 x 11, w(i,j) = g(i) g(j), g(i) = exp(-(i-5)^2 / (2 * 1.5^2)) / sum -- evaluated in fp64, rounded to fp32 once (SSIM_G);
//   "valid" windows only: one value per window wholly inside the image -> a map of (H-10) x (W-10) x C, no padding;
//   per window and channel   mu_a = sum w a,  var_a = sum w (a - mu_a)^2,  cov = sum w (a - mu_a)(b - mu_b)   (weighted population moments)
//   c1 = (0.01 L)^2, c2 = (0.03 L)^2, L = data_range
//   ssim = (2 mu_a mu_b + c1)(2 cov + c2) / ((mu_a^2 + mu_b^2 + c1)(var_a + var_b + c2));   the image's SSIM = plain mean of the map.
//
// The moments are CENTRED, two passes over the window: on a flat background var + c2 = c2 = 9e-4 L^2 is the whole denominator of the
// second factor, and the textbook E[a^2] - mu^2 leaves a 1e-7 cancellation error there = 1e-4 of SSIM (4.9e-4 against
// 1.4e-6 on an fp32 emulation).  An error of mu enters the centred sums only in second order (sum w (a - mu) = 0).
//
// Layout: a workgroup of 256 threads owns a tile of 32 x 8 windows and stages the 42 x 18 halo of both images in LDS once, one plane
// per channel: a wave reads two rows of 32 consecutive floats per tap, each 32-lane group of a ds_read_b32 one row -> no bank
// conflict whatever C is (channel-last rows would be 4 C bytes apart).  A thread computes its window for every channel: 2 x 121 taps
// for the means, 2 x 121 for the centred sums.  Per-tile sums of the map go to the caller's workspace as fp64, tn_ssim's second launch
// (one workgroup) adds them in a fixed order and divides: no atomics, the mean is the same bits on every call.
#include "tn_common.h"

namespace {

constexpr int WIN = 11, HALO = WIN - 1;
constexpr int TW = 32, TH = 8;                      // tile of windows; TW = half a wave, so a 32-lane LDS group is one row
constexpr int SW = TW + HALO, SH = TH + HALO;       // staged halo: 42 x 18
constexpr int PLANE = SW * SH;
constexpr int THREADS = TW * TH;
constexpr int MAX_C = 4;
constexpr int64_t MAX_SIDE = 65536;                 // (H - 10) / TH tiles must fit gridDim.y

__constant__ float SSIM_G[WIN] = {
    0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,      // 1.028380124e-03 7.598758209e-03
    0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f,                     // 3.600077331e-02 1.093606874e-01
                                                                                                        // 2.130055428e-01 2.660117149e-01
};

template <int C>
__global__ __launch_bounds__(THREADS) void ssim_tile_kernel(const float *__restrict__ a, const float *__restrict__ b, int H, int W, float c1,
                                                            float c2, float *__restrict__ map, double *__restrict__ partial)
{
    __shared__ float sa[C * PLANE], sb[C * PLANE];
    __shared__ double wave_part[THREADS / 64];
    const int x0 = (int)blockIdx.x * TW, y0 = (int)blockIdx.y * TH;
    const int rows = min(SH, H - y0), cols = min(SW, W - x0);       // the part of the halo that lies inside the image (>= 11 x 11)
    // global order (y, x, c) is the images' own: a halo row is cols * C consecutive floats
    for (int e = (int)threadIdx.x; e < SH * SW * C; e += THREADS) {
        const int y = e / (SW * C), r = e - y * (SW * C), x = r / C, c = r - x * C;
        float va = 0.0f, vb = 0.0f;                                 // outside the image: only windows that are not output read these
        if (y < rows && x < cols) {
            const int64_t g = ((int64_t)(y0 + y) * W + (x0 + x)) * C + c;
            va = a[g];
            vb = b[g];
        }
        sa[c * PLANE + y * SW + x] = va;
        sb[c * PLANE + y * SW + x] = vb;
    }
    __syncthreads();

    const int tx = (int)threadIdx.x & (TW - 1), ty = (int)threadIdx.x / TW;
    const int ox = x0 + tx, oy = y0 + ty, OW = W - HALO;
    const bool valid = ox < OW && oy < H - HALO;
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float *pa = sa + c * PLANE + ty * SW + tx, *pb = sb + c * PLANE + ty * SW + tx;
        float mua = 0.0f, mub = 0.0f;
        for (int i = 0; i < WIN; ++i) {
            const float gi = SSIM_G[i];
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const float w = gi * SSIM_G[j];
                mua = fmaf(w, pa[i * SW + j], mua);
                mub = fmaf(w, pb[i * SW + j], mub);
            }
        }
        float vaa = 0.0f, vbb = 0.0f, vab = 0.0f;
        for (int i = 0; i < WIN; ++i) {
            const float gi = SSIM_G[i];
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const float w = gi * SSIM_G[j];
                const float da = pa[i * SW + j] - mua, db = pb[i * SW + j] - mub;
                const float wda = w * da;
                vaa = fmaf(wda, da, vaa);
                vab = fmaf(wda, db, vab);
                vbb = fmaf(w * db, db, vbb);
            }
        }
        const float num = (2.0f * mua * mub + c1) * (2.0f * vab + c2);
        const float den = (mua * mua + mub * mub + c1) * (vaa + vbb + c2);
        const float s = num / den;
        if (valid) {
            acc += s;
            if (map != nullptr) map[((int64_t)oy * OW + ox) * C + c] = s;
        }
    }
    // the tile's sum: a fixed tree inside the wave, then the four waves in order
    double s = (double)acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (tn::lane_id() == 0) wave_part[threadIdx.x / 64] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wave_part[0];
#pragma unroll
        for (int k = 1; k < THREADS / 64; ++k) t += wave_part[k];
        partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

// one workgroup: thread t adds partial[t], partial[t + 256], ... in that order, then a fixed tree over the 256 sums
__global__ __launch_bounds__(256) void ssim_mean_kernel(const double *__restrict__ partial, int64_t n, double inv_count, float *__restrict__ mean)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += partial[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[0] = (float)(sh[0] * inv_count);
}

// shared argument checks of the two entry points; *tiles_x, *tiles_y: the launch grid
int ssim_shape(const char *fn, int64_t H, int64_t W, int32_t C, int64_t *tiles_x, int64_t *tiles_y)
{
    if (H < 0 || W < 0 || C < 0 || H > MAX_SIDE || W > MAX_SIDE) {
        tn::set_error("%s: negative size or an image side above %lld", fn, (long long)MAX_SIDE);
        return TN_E_SIZE;
    }
    if (H < WIN || W < WIN || C < 1 || C > MAX_C) {
        tn::set_error("%s: needs H >= 11, W >= 11 (one whole window) and 1 <= C <= 4", fn);
        return TN_E_CONFIG;
    }
    *tiles_x = (W - HALO + TW - 1) / TW;
    *tiles_y = (H - HALO + TH - 1) / TH;
    return TN_OK;
}

}  // namespace

extern "C" int tn_ssim_workspace_bytes(int64_t H, int64_t W, int32_t C, int64_t *bytes)
{
    int64_t nx, ny;
    if (int rc = ssim_shape("tn_ssim_workspace_bytes", H, W, C, &nx, &ny)) return rc;
    TN_REQUIRE(bytes, TN_E_NULL, "tn_ssim_workspace_bytes: null pointer");
    *bytes = nx * ny * (int64_t)sizeof(double);
    return TN_OK;
}

extern "C" int tn_ssim(const float *a, const float *b, int64_t H, int64_t W, int32_t C, float data_range, float *map, void *workspace,
                       int64_t workspace_bytes, float *mean, void *stream)
{
    TN_REQUIRE(workspace_bytes >= 0, TN_E_SIZE, "tn_ssim: negative size");
    int64_t nx, ny;
    if (int rc = ssim_shape("tn_ssim", H, W, C, &nx, &ny)) return rc;
    TN_REQUIRE(a && b && workspace && mean, TN_E_NULL, "tn_ssim: null pointer");
    TN_REQUIRE(data_range > 0.0f && data_range <= 3.0e38f, TN_E_CONFIG, "tn_ssim: data_range must be a finite number > 0");
    TN_REQUIRE(workspace_bytes >= nx * ny * (int64_t)sizeof(double), TN_E_CONFIG, "tn_ssim: workspace smaller than tn_ssim_workspace_bytes says");
    TN_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)map | (uintptr_t)mean) & 3) == 0 && ((uintptr_t)workspace & 7) == 0, TN_E_ALIGN,
               "tn_ssim: images, map and mean must be 4-byte aligned, the workspace 8-byte aligned");
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    const dim3 grid((unsigned)nx, (unsigned)ny), block(THREADS);
    double *partial = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
    case 1: ssim_tile_kernel<1><<<grid, block, 0, st>>>(a, b, (int)H, (int)W, c1, c2, map, partial); break;
    case 2: ssim_tile_kernel<2><<<grid, block, 0, st>>>(a, b, (int)H, (int)W, c1, c2, map, partial); break;
    case 3: ssim_tile_kernel<3><<<grid, block, 0, st>>>(a, b, (int)H, (int)W, c1, c2, map, partial); break;
    default: ssim_tile_kernel<4><<<grid, block, 0, st>>>(a, b, (int)H, (int)W, c1, c2, map, partial); break;
    }
    if (int rc = tn::check_launch("ssim_tile_kernel")) return rc;
    const double count = (double)(H - HALO) * (double)(W - HALO) * (double)C;
    ssim_mean_kernel<<<dim3(1), dim3(256), 0, st>>>(partial, nx * ny, 1.0 / count, mean);
    return tn::check_launch("ssim_mean_kernel");
}
