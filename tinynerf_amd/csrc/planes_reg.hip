// K-Planes total-variation / L1 regularisers (reference src/models.py:115-121,165-181) for
// channel-last planes [H][W][C].  The reference evaluates, per plane, two mse_loss calls on shifted
// strided views (plus their autograd backward): ~0.5 GB of traffic per step over the 126 MiB of
// planes.  Here the forward is one streaming read per plane with an fp64 block
// reduction, and the backward one pass that adds the 5-point stencil of the gradient straight into
// the plane's gradient buffer.  HBM-bound: fwd 4 B/element, bwd 12 B/element.
//
// Seven kernels, one copy of each piece of arithmetic: adam_update (one element), reg_texel (one float4 of the
// regulariser's stencil and sums) and block_add3 (the sums' block reduction); on the host bias_corrections, the
// REQUIRE_ADAM_ITEM checks and for_chunks (the multi entry points' pack-and-launch loop).
#include "tn_common.h"
#include <algorithm>
#include <math.h>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

struct AdamHyper { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; };

// Adam's bias corrections in doubles, like torch's python scalars (device: adam_multi_kernel<true>, from its device-side count)
__host__ __device__ inline void bias_corrections(float b1, float b2, double step, float &bc1, float &bc2_sqrt)
{
    bc1 = (float)(1.0 - pow((double)b1, step));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, step));
}

// torch.optim.Adam (no amsgrad, coupled weight decay) for one element
__device__ __forceinline__ void adam_update(const AdamHyper &h, float &p, float g, float &m, float &v)
{
    const float gg = g + h.wd * p;
    m = m + (gg - m) * (1.0f - h.b1);            // lerp form, as torch
    v = h.b2 * v + (1.0f - h.b2) * gg * gg;
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = p - (h.lr / h.bc1) * (m / denom);
}

__device__ __forceinline__ void adam_update4(const AdamHyper &h, f4 &p, const f4 &g, f4 &m, f4 &v)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float pc = p[c], mc = m[c], vc = v[c];  // (a reference cannot bind to a vector's element)
        adam_update(h, pc, g[c], mc, vc);
        p[c] = pc; m[c] = mc; v[c] = vc;
    }
}

template <typename S> struct Sums3 { S y = 0, x = 0, l = 0; };      // TV along y, TV along x, L1

// float4 i (value v) of the plane q [H][W][C4]: the regulariser's gradient term 2cy dy + 2cx dx + cl1 sign(v), before the upstream
// factor.  SUMS: the texel's squared forward differences and its |v| are added to *s as well, each per-texel term in fp32 and then
// converted to S.
template <bool SUMS, typename S = float>
__device__ __forceinline__ f4 reg_texel(const f4 *__restrict__ q, int64_t i, const f4 v, int H, int W, int C4, float cy2, float cx2,
                                        float cl1, Sums3<S> *s = nullptr)
{
    const int64_t texel = i / C4;
    const int x = (int)(texel % W), y = (int)(texel / W);
    f4 dy = {0.f, 0.f, 0.f, 0.f}, dx = {0.f, 0.f, 0.f, 0.f};
    if (y > 0) dy += v - q[i - (int64_t)W * C4];
    if (x > 0) dx += v - q[i - C4];
    if (y + 1 < H) {
        const f4 d = q[i + (int64_t)W * C4] - v;
        dy -= d;
        if constexpr (SUMS) s->y += (S)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
    }
    if (x + 1 < W) {
        const f4 d = q[i + C4] - v;
        dx -= d;
        if constexpr (SUMS) s->x += (S)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
    }
    if constexpr (SUMS) s->l += (S)(fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]) + fabsf(v[3]));
    f4 r = dy * cy2 + dx * cx2;
    if (cl1 != 0.0f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] += cl1 * (v[c] > 0.f ? 1.f : (v[c] < 0.f ? -1.f : 0.f));
    }
    return r;
}

// the block's three sums, one atomicAdd each to out[0..2]; every thread of the (256-thread) block calls this
__device__ __forceinline__ void block_add3(double sy, double sx, double sl, double *__restrict__ out)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sy += __shfl_xor(sy, o, 64); sx += __shfl_xor(sx, o, 64); sl += __shfl_xor(sl, o, 64); }
    __shared__ double red[3][4];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sy; red[1][threadIdx.x >> 6] = sx; red[2][threadIdx.x >> 6] = sl; }
    __syncthreads();
    if (threadIdx.x < 3) atomicAdd(&out[threadIdx.x], red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}

__global__ __launch_bounds__(256) void plane_reg_fwd_kernel(const float *__restrict__ p, int H, int W, int C4,
                                                            double *__restrict__ sums)
{
    const int64_t total = (int64_t)H * W * C4;
    Sums3<double> s;                 // unlike the multi kernels, every per-texel term is widened to fp64 before it is added
    const f4 *q = reinterpret_cast<const f4 *>(p);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        reg_texel<true>(q, i, q[i], H, W, C4, 0.0f, 0.0f, 0.0f, &s);        // (the sums alone: the gradient term is not used)
    block_add3(s.y, s.x, s.l, sums);
}

__global__ __launch_bounds__(256) void plane_reg_bwd_kernel(const float *__restrict__ p, int H, int W, int C4, float cy, float cx,
                                                            float cl1, const float *__restrict__ upstream, float *__restrict__ grad)
{
    const int64_t total = (int64_t)H * W * C4;
    const float up = upstream[0];    // autograd's backward: the upstream gradient is a device scalar (a launch argument in the multi forms)
    const f4 *q = reinterpret_cast<const f4 *>(p);
    f4 *g = reinterpret_cast<f4 *>(grad);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        g[i] += reg_texel<false>(q, i, q[i], H, W, C4, 2.0f * cy, 2.0f * cx, cl1) * up;
}

// torch.optim.Adam for one tensor, element-wise, any memory layout
__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                   float *__restrict__ v, int64_t n4, int64_t n, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2_sqrt, int zero_grad)
{
    const AdamHyper h{lr, b1, b2, eps, wd, bc1, bc2_sqrt};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        if (4 * i + 3 < n) {
            f4 pv = reinterpret_cast<f4 *>(p)[i], gv = reinterpret_cast<f4 *>(g)[i];
            f4 mv = reinterpret_cast<f4 *>(m)[i], vv = reinterpret_cast<f4 *>(v)[i];
            adam_update4(h, pv, gv, mv, vv);
            reinterpret_cast<f4 *>(p)[i] = pv; reinterpret_cast<f4 *>(m)[i] = mv; reinterpret_cast<f4 *>(v)[i] = vv;
            if (zero_grad) reinterpret_cast<f4 *>(g)[i] = f4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int64_t e = 4 * i; e < n; ++e) {
                adam_update(h, p[e], g[e], m[e], v[e]);
                if (zero_grad) g[e] = 0.0f;
            }
        }
    }
}

// ---- multi-tensor forms: the harness has 9 planes and ~20 parameter tensors; one launch each instead of one per
// tensor removes ~40 launches (and the host time between them) from every step.  blockIdx.y = item.
struct RegItems { tn_plane_reg_item it[TN_MULTI_MAX]; };
struct AdamItems { tn_adam_item it[TN_MULTI_MAX]; };

// fused forward + backward of the regulariser for a constant upstream gradient: the plane is read once, the three
// sums go to fp64 accumulators and the 5-point stencil of the gradient is added to the gradient buffer.
__global__ __launch_bounds__(256) void plane_reg_multi_kernel(RegItems items, float up, double *__restrict__ sums)
{
    const tn_plane_reg_item &t = items.it[blockIdx.y];
    const int W = t.W, H = t.H, C4 = t.C >> 2;
    const int64_t total = (int64_t)H * W * C4;
    const f4 *q = reinterpret_cast<const f4 *>(t.plane);
    f4 *g = reinterpret_cast<f4 *>(t.grad);
    const float cy2 = 2.0f * t.cy, cx2 = 2.0f * t.cx;
    Sums3<float> s;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const f4 r = reg_texel<true>(q, i, q[i], H, W, C4, cy2, cx2, t.cl1, &s);
        if (g != nullptr) g[i] += r * up;
    }
    if (sums == nullptr) return;
    // per-thread partials are fp32 over <= a few hundred texels; everything above that is fp64.  The slot is the item's position.
    block_add3(s.y, s.x, s.l, sums + 3 * blockIdx.y);
}

__global__ void adam_gate_kernel(int32_t *__restrict__ step, const float *__restrict__ gate)
{
    if (gate[0] > 0.0f) step[0] += 1;
}

// The only Adam kernel that tracks `bad`.  GATED: bias corrections from a device-side step count, nothing but the optional gradient
// zeroing when the gate is closed
template <bool GATED>
__global__ __launch_bounds__(256) void adam_multi_kernel(AdamItems items, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                         float bc2_sqrt, int zero_grad, const int32_t *__restrict__ step_dev,
                                                         const float *__restrict__ gate, int32_t *__restrict__ nonfinite)
{
    const tn_adam_item &t = items.it[blockIdx.y];
    bool bad = false;            // an updated parameter that is not finite (see tn_adam_multi_gated: zero_grad bit 1)
    float *__restrict__ p = t.param; float *__restrict__ g = t.grad; float *__restrict__ m = t.exp_avg; float *__restrict__ v = t.exp_avg_sq;
    const int64_t n = t.n, n4 = (n + 3) / 4;
    if constexpr (GATED) {
        if (!(gate[0] > 0.0f)) {
            if (zero_grad)
                for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) g[e] = 0.0f;
            return;
        }
        bias_corrections(b1, b2, (double)step_dev[0], bc1, bc2_sqrt);
    }
    const AdamHyper h{lr, b1, b2, eps, wd, bc1, bc2_sqrt};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        if (4 * i + 3 < n) {
            f4 pv = reinterpret_cast<f4 *>(p)[i], gv = reinterpret_cast<f4 *>(g)[i];
            f4 mv = reinterpret_cast<f4 *>(m)[i], vv = reinterpret_cast<f4 *>(v)[i];
            adam_update4(h, pv, gv, mv, vv);
#pragma unroll
            for (int c = 0; c < 4; ++c) bad |= !(fabsf(pv[c]) <= 3.402823466e38f);
            reinterpret_cast<f4 *>(p)[i] = pv; reinterpret_cast<f4 *>(m)[i] = mv; reinterpret_cast<f4 *>(v)[i] = vv;
            if (zero_grad) reinterpret_cast<f4 *>(g)[i] = f4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int64_t e = 4 * i; e < n; ++e) {
                adam_update(h, p[e], g[e], m[e], v[e]);
                bad |= !(fabsf(p[e]) <= 3.402823466e38f);
                if (zero_grad) g[e] = 0.0f;
            }
        }
    }
    if (nonfinite != nullptr && bad) nonfinite[0] = 1;          // (plain stores of one value: no atomic needed)
}

// Adam with the K-Planes regulariser folded in (harness): for plane tensors the total-variation / L1 gradient is built
// from the CURRENT values while the update is written to a second buffer (the caller swaps the two), so the planes, their
// gradients and both moments are streamed exactly once per step instead of once for the regulariser and once for Adam.
struct AdamRegItems { tn_adam_reg_item it[TN_MULTI_MAX / 2]; };

__global__ __launch_bounds__(256) void adam_reg_multi_kernel(AdamRegItems items, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                             float bc2_sqrt, int zero_grad, float up, double *__restrict__ sums)
{
    const tn_adam_reg_item &t = items.it[blockIdx.y];
    const AdamHyper h{lr, b1, b2, eps, wd, bc1, bc2_sqrt};
    const float *__restrict__ p = t.param; float *__restrict__ po = t.param_out;      // the stencil needs its neighbours' old values
    float *__restrict__ g = t.grad; float *__restrict__ m = t.exp_avg; float *__restrict__ v = t.exp_avg_sq;
    const int64_t n = t.n, n4 = (n + 3) / 4;
    const bool reg = t.H > 0;                                   // H == 0: a tensor without a regulariser
    const int W = t.W, H = t.H, C4 = t.C >> 2;
    const float cy2 = 2.0f * t.cy, cx2 = 2.0f * t.cx;
    Sums3<float> s;
    // sharded pass: this rank's rows of the plane as a range of float4 indices (everything, unless row1 > 0)
    const int64_t own0 = (reg && t.row1 > 0) ? (int64_t)t.row0 * W * C4 : 0, own1 = (reg && t.row1 > 0) ? (int64_t)t.row1 * W * C4 : n4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < own0 || i >= own1) {                            // another rank's rows: only the gradient buffer is cleared
            if (zero_grad) reinterpret_cast<f4 *>(g)[i] = f4{0.f, 0.f, 0.f, 0.f};
            continue;
        }
        if (4 * i + 3 < n) {
            const f4 *q = reinterpret_cast<const f4 *>(p);
            f4 pv = q[i], gv = reinterpret_cast<f4 *>(g)[i];
            f4 mv = reinterpret_cast<f4 *>(m)[i], vv = reinterpret_cast<f4 *>(v)[i];
            if (reg) gv += reg_texel<true>(q, i, pv, H, W, C4, cy2, cx2, t.cl1, &s) * up;     // as plane_reg_multi_kernel: g += r * upstream
            adam_update4(h, pv, gv, mv, vv);
            reinterpret_cast<f4 *>(po)[i] = pv; reinterpret_cast<f4 *>(m)[i] = mv; reinterpret_cast<f4 *>(v)[i] = vv;
            if (zero_grad) reinterpret_cast<f4 *>(g)[i] = f4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int64_t e = 4 * i; e < n; ++e) {               // (tails: tensors without a regulariser only -- a plane's C is a multiple of 4)
                float pe = p[e];
                adam_update(h, pe, g[e], m[e], v[e]);
                po[e] = pe;
                if (zero_grad) g[e] = 0.0f;
            }
        }
    }
    if (!reg || sums == nullptr) return;
    // fp32 partials widened here, as in plane_reg_multi_kernel; the slot is the caller's absolute sum_slot, not the item's position
    block_add3(s.y, s.x, s.l, sums + 3 * t.sum_slot);
}

// ---- host side.  Grids: blocks_for (at most 2048 blocks of 256) for the single-tensor kernels, at most 1024 x items for the multi forms.
inline unsigned blocks_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 8); }

inline bool plane_shape_ok(int H, int W, int C) { return H > 0 && W > 0 && C > 0 && (C & 3) == 0; }
template <typename... P> inline bool none_null(const P *...p) { return (... && (p != nullptr)); }
template <typename... P> inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15) == 0; }

// one Adam item `t` of entry point `fn` (a string literal), the rest its buffers: size, then null pointers, then alignment
#define REQUIRE_ADAM_ITEM(fn, t, ...)                                                                     \
    do {                                                                                                  \
        TN_REQUIRE((t).n >= 0, TN_E_SIZE, fn ": negative size");                                          \
        TN_REQUIRE((t).n == 0 || none_null(__VA_ARGS__), TN_E_NULL, fn ": null pointer");                 \
        TN_REQUIRE(aligned16(__VA_ARGS__), TN_E_ALIGN, fn ": buffers must be 16-byte aligned");           \
    } while (0)

inline int64_t float4s(const tn_plane_reg_item &t) { return (int64_t)t.H * t.W * (t.C / 4); }
template <typename Item> inline int64_t float4s(const Item &t) { return (t.n + 3) / 4; }

// The multi entry points' loop: the items go to the kernel by value, in chunks of what a Pack holds.  check(item) validates one item (a
// non-zero return ends the call: the chunks before it have been launched); launch(pack, grid, base) starts the kernel on a chunk and
// returns check_launch's code.  A chunk of empty items is not launched.
template <typename Pack, typename Item, typename Check, typename Launch>
int for_chunks(const Item *items, int n_items, Check check, Launch launch)
{
    constexpr int MAXI = (int)(sizeof(Pack) / sizeof(Item));
    for (int base = 0; base < n_items; base += MAXI) {
        Pack pack;
        const int cnt = std::min(MAXI, n_items - base);
        int64_t largest = 0;
        for (int i = 0; i < cnt; ++i) {
            if (int rc = check(items[base + i])) return rc;
            pack.it[i] = items[base + i];
            largest = std::max(largest, float4s(items[base + i]));
        }
        if (largest == 0) continue;
        if (int rc = launch(pack, dim3(std::min<unsigned>(blocks_for(largest), 1024), (unsigned)cnt), base)) return rc;
    }
    return TN_OK;
}

}  // namespace

extern "C" int tn_plane_reg_fwd(const float *plane, int H, int W, int C, double *sums, void *stream)
{
    TN_REQUIRE(plane_shape_ok(H, W, C), TN_E_SIZE, "tn_plane_reg_fwd: bad shape (C must be a multiple of 4)");
    TN_REQUIRE(plane && sums, TN_E_NULL, "tn_plane_reg_fwd: null pointer");
    TN_REQUIRE(aligned16(plane), TN_E_ALIGN, "tn_plane_reg_fwd: plane must be 16-byte aligned");
    const int64_t n = (int64_t)H * W * (C / 4);
    plane_reg_fwd_kernel<<<dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream>>>(plane, H, W, C / 4, sums);
    return tn::check_launch("plane_reg_fwd_kernel");
}

extern "C" int tn_plane_reg_bwd(const float *plane, int H, int W, int C, float cy, float cx, float cl1, const float *upstream,
                                float *grad, void *stream)
{
    TN_REQUIRE(plane_shape_ok(H, W, C), TN_E_SIZE, "tn_plane_reg_bwd: bad shape (C must be a multiple of 4)");
    TN_REQUIRE(plane && upstream && grad, TN_E_NULL, "tn_plane_reg_bwd: null pointer");
    TN_REQUIRE(aligned16(plane, grad), TN_E_ALIGN, "tn_plane_reg_bwd: buffers must be 16-byte aligned");
    const int64_t n = (int64_t)H * W * (C / 4);
    plane_reg_bwd_kernel<<<dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream>>>(plane, H, W, C / 4, cy, cx, cl1, upstream, grad);
    return tn::check_launch("plane_reg_bwd_kernel");
}

extern "C" int tn_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, int32_t step, int32_t zero_grad, void *stream)
{
    TN_REQUIRE(n >= 0 && step >= 1, TN_E_SIZE, "tn_adam_step: bad size / step");
    if (n == 0) return TN_OK;
    TN_REQUIRE(param && grad && exp_avg && exp_avg_sq, TN_E_NULL, "tn_adam_step: null pointer");
    TN_REQUIRE(aligned16(param, grad, exp_avg, exp_avg_sq), TN_E_ALIGN, "tn_adam_step: buffers must be 16-byte aligned");
    float bc1, bc2_sqrt;
    bias_corrections(beta1, beta2, (double)step, bc1, bc2_sqrt);
    const int64_t n4 = (n + 3) / 4;
    adam_kernel<<<dim3(blocks_for(n4)), dim3(256), 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, n4, n, lr, beta1, beta2, eps,
                                                                             weight_decay, bc1, bc2_sqrt, zero_grad);
    return tn::check_launch("adam_kernel");
}

extern "C" int tn_plane_reg_multi(const tn_plane_reg_item *items, int32_t n_items, float upstream, double *sums, void *stream)
{
    TN_REQUIRE(n_items >= 0, TN_E_SIZE, "tn_plane_reg_multi: negative item count");
    TN_REQUIRE(n_items == 0 || items, TN_E_NULL, "tn_plane_reg_multi: null items");
    return for_chunks<RegItems>(
        items, n_items,
        [](const tn_plane_reg_item &t) -> int {
            TN_REQUIRE(plane_shape_ok(t.H, t.W, t.C), TN_E_SIZE, "tn_plane_reg_multi: bad shape (C must be a multiple of 4)");
            TN_REQUIRE(t.plane, TN_E_NULL, "tn_plane_reg_multi: null plane");
            TN_REQUIRE(aligned16(t.plane, t.grad), TN_E_ALIGN, "tn_plane_reg_multi: buffers must be 16-byte aligned");     // (grad may be null)
            return TN_OK;
        },
        [&](const RegItems &pack, dim3 grid, int base) {
            plane_reg_multi_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(pack, upstream, sums ? sums + 3 * base : nullptr);
            return tn::check_launch("plane_reg_multi_kernel");
        });
}

extern "C" int tn_adam_multi(const tn_adam_item *items, int32_t n_items, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int32_t step, int32_t zero_grad, void *stream)
{
    TN_REQUIRE(n_items >= 0 && step >= 1, TN_E_SIZE, "tn_adam_multi: bad item count / step");
    TN_REQUIRE(n_items == 0 || items, TN_E_NULL, "tn_adam_multi: null items");
    float bc1, bc2_sqrt;
    bias_corrections(beta1, beta2, (double)step, bc1, bc2_sqrt);
    return for_chunks<AdamItems>(
        items, n_items,
        [](const tn_adam_item &t) -> int {
            REQUIRE_ADAM_ITEM("tn_adam_multi", t, t.param, t.grad, t.exp_avg, t.exp_avg_sq);
            return TN_OK;
        },
        [&](const AdamItems &pack, dim3 grid, int) {
            adam_multi_kernel<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(pack, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt,
                                                                                  zero_grad, nullptr, nullptr, nullptr);
            return tn::check_launch("adam_multi_kernel");
        });
}

extern "C" int tn_adam_multi_gated(const tn_adam_item *items, int32_t n_items, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int32_t *step_dev, const float *gate, int32_t zero_grad, void *stream)
{
    TN_REQUIRE(n_items >= 0, TN_E_SIZE, "tn_adam_multi_gated: bad item count");
    TN_REQUIRE((n_items == 0 || items) && step_dev && gate, TN_E_NULL, "tn_adam_multi_gated: null items / step counter / gate");
    adam_gate_kernel<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(step_dev, gate);
    if (int rc = tn::check_launch("adam_gate_kernel")) return rc;
    return for_chunks<AdamItems>(
        items, n_items,
        [](const tn_adam_item &t) -> int {
            REQUIRE_ADAM_ITEM("tn_adam_multi_gated", t, t.param, t.grad, t.exp_avg, t.exp_avg_sq);
            return TN_OK;
        },
        [&](const AdamItems &pack, dim3 grid, int) {
            // zero_grad bit 1: the non-finite flag lives behind the step count.  The bias corrections (1, 1 here) come from that count.
            adam_multi_kernel<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(pack, lr, beta1, beta2, eps, weight_decay, 1.0f, 1.0f, zero_grad & 1,
                                                                                 step_dev, gate, (zero_grad & 2) ? step_dev + 1 : nullptr);
            return tn::check_launch("adam_multi_kernel<gated>");
        });
}

extern "C" int tn_adam_reg_multi(const tn_adam_reg_item *items, int32_t n_items, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, int32_t step, int32_t zero_grad, float upstream, double *sums, void *stream)
{
    TN_REQUIRE(n_items >= 0 && step >= 1, TN_E_SIZE, "tn_adam_reg_multi: bad item count / step");
    TN_REQUIRE(n_items == 0 || items, TN_E_NULL, "tn_adam_reg_multi: null items");
    float bc1, bc2_sqrt;
    bias_corrections(beta1, beta2, (double)step, bc1, bc2_sqrt);
    return for_chunks<AdamRegItems>(
        items, n_items,
        [&](const tn_adam_reg_item &t) -> int {
            REQUIRE_ADAM_ITEM("tn_adam_reg_multi", t, t.param, t.param_out, t.grad, t.exp_avg, t.exp_avg_sq);
            if (t.H > 0) {
                TN_REQUIRE(t.W > 0 && t.C > 0 && (t.C & 3) == 0 && (int64_t)t.H * t.W * t.C == t.n, TN_E_SIZE,
                           "tn_adam_reg_multi: plane shape must match n (C a multiple of 4)");
                TN_REQUIRE(t.param_out != t.param, TN_E_CONFIG, "tn_adam_reg_multi: a regularised plane needs a separate output buffer");
                TN_REQUIRE(sums == nullptr || t.sum_slot >= 0, TN_E_SIZE, "tn_adam_reg_multi: bad sum slot");
            }
            // sharded pass: row1 == 0 means every row; anything else must be a non-empty range inside the plane (a mis-sharded caller
            // would otherwise train with frozen rows and no error)
            TN_REQUIRE(t.row1 == 0 ? t.row0 == 0 : (t.H > 0 && t.row0 >= 0 && t.row0 < t.row1 && t.row1 <= t.H), TN_E_SIZE,
                       "tn_adam_reg_multi: rows [row0, row1) must satisfy 0 <= row0 < row1 <= H (row1 == 0, row0 == 0: every row)");
            return TN_OK;
        },
        [&](const AdamRegItems &pack, dim3 grid, int) {
            adam_reg_multi_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(pack, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, zero_grad,
                                                                               upstream, sums);
            return tn::check_launch("adam_reg_multi_kernel");
        });
}
