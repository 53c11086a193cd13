// Surface normals of a K-Planes or hash-grid density (definition: include/tinynerf_hip.h): the gradient of the sigma
// head's pre-activation y with respect to the sample position, analytically, in one launch per call.
//
//   y(f) = b2 + sum_j w2_j max(0, h_j),  h = W1 f + b1        (VanillaOpacityDecoder, F -> 64 -> 1)
//   g    = dy/df = W1^T (w2 . [h > 0])                        reverse mode: one F-vector per sample
//   grad = sum_c g_c df_c/dx                                  contracted frame;  v = -J^T grad, n = v / |v|  world frame
//
// Mapping (kplanes_device.h / mlp_device.h): a wave owns a 32-sample tile, lane l = (h = l >> 5, j = l & 31) owns sample j and one half
// of the work of that sample -- the channel half [h C/2, (h+1) C/2) of every plane, the levels l = h, h + 2, ... of a hash grid, the
// hidden units [32 h, 32 h + 32) of the head.  Three phases per tile:
//   1  gather the features f (the forward's taps, cells and fma chains) and hand them to both halves through the wave's LDS rows;
//      h accumulates in 32 registers per lane against W1^T in LDS (staged once per workgroup, [feature][hidden]: a lane's 32 hidden
//      units are 8 x ds_read_b128, the same address in all lanes of a half);
//   2  the ReLU bits of the two halves are exchanged with one shuffle; a_k = [h_k > 0] w2_k sits in 64 registers;
//   3  per owned feature c: g_c = <W1^T[c], a>, the taps are gathered AGAIN (they are in cache; keeping 9 planes x (value, d/du, d/dv)
//      alive across the head would take 430 registers) and contracted with g; the halves' partial sums meet in one shuffle.
// Plain FMAs: the head's 2 x 64 x F multiply-adds per sample are small beside the 2 x 36 (K-Planes) / 2 x 8 L (hash grid) gathers.
// fp32 throughout, no fp16 splits: a ReLU bit that moved with the matrix mode would make a normal depend on a flag.
#include "kplanes_device.h"
#include "hashgrid_device.h"
#include <algorithm>

namespace {

using tn::f32x4k;

constexpr int NW = 4;            // waves per workgroup
constexpr int HID = 64;          // the head's hidden width

__device__ __forceinline__ void wave_sync()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

struct HeadArgs {
    const float *w1, *b1, *w2;   // [64][F], [64], [1][64]
    int F;
};

struct FrameArgs {
    int kind;                    // TN_CONTRACT_*
    float scale[3];              // AABB: 2 / (hi - lo)
};

struct KpnArgs {
    int n_scales, C;
    int H[TN_KPLANES_MAX_SCALES], W[TN_KPLANES_MAX_SCALES];
    const float *planes[TN_KPLANES_MAX_SCALES][3];
};

// ------------------------------------------------------------------------------------------------------------------------ the head
// W1^T [F][64], b1 [64], w2 [64] into LDS: conflict-free LDS writes, the strided global reads come out of L2 (24 KB at F = 96)
__device__ __forceinline__ void stage_head(const HeadArgs &hd, float *__restrict__ w1t, float *__restrict__ b1s, float *__restrict__ w2s)
{
    for (int e = threadIdx.x; e < hd.F * HID; e += NW * 64) w1t[e] = hd.w1[(e & (HID - 1)) * hd.F + (e >> 6)];
    if (threadIdx.x < HID) {
        b1s[threadIdx.x] = hd.b1[threadIdx.x];
        w2s[threadIdx.x] = hd.w2[threadIdx.x];
    }
    __syncthreads();
}

// acc[k] += sum_c W1[32 h + k][c0 + c] f[c][j] over the nc feature rows of the wave's stage
__device__ __forceinline__ void hidden_add(float (&acc)[32], const float *__restrict__ w1t, const float *__restrict__ stage, int c0, int nc,
                                           int j, int h)
{
    for (int c = 0; c < nc; ++c) {
        const float fv = stage[c * 32 + j];
        const f32x4k *w = reinterpret_cast<const f32x4k *>(w1t + (c0 + c) * HID + 32 * h);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4k wv = w[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * q + e] = __builtin_fmaf(wv[e], fv, acc[4 * q + e]);
        }
    }
}

// a_k = [h_k > 0] w2_k for all 64 hidden units of the lane's sample (torch's relu backward: 0 at h == 0, and for a NaN)
__device__ __forceinline__ void relu_coefficients(const float (&acc)[32], const float *__restrict__ w2s, int h, float (&a)[HID])
{
    uint32_t own = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) own |= (acc[k] > 0.0f ? 1u : 0u) << k;
    const uint32_t other = (uint32_t)__shfl_xor((int)own, 32, 64);
    const uint32_t lo = h ? other : own, hi = h ? own : other;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        a[k] = (lo >> k) & 1u ? w2s[k] : 0.0f;
        a[32 + k] = (hi >> k) & 1u ? w2s[32 + k] : 0.0f;
    }
}

// g_c = sum_k W1[k][c] a_k
__device__ __forceinline__ float head_g(const float *__restrict__ w1t, int c, const float (&a)[HID])
{
    const f32x4k *w = reinterpret_cast<const f32x4k *>(w1t + c * HID);
    float g = 0.0f;
#pragma unroll
    for (int q = 0; q < HID / 4; ++q) {
        const f32x4k wv = w[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) g = __builtin_fmaf(wv[e], a[4 * q + e], g);
    }
    return g;
}

// ----------------------------------------------------------------------------------------------------------------- the world frame
// v = -J^T grad, J = d(contracted x) / d(world X), from the contracted x alone.  Mip-NeRF 360 (u = 2 x, s = |u|_p in (1, 2),
// X = u / (s (2 - s))): with D = <u, grad>
//   p = inf, k the lowest axis with |u_k| = s:  v_j = -(2 - s)/2 * s grad_j (j != k),
//                                               v_k = -(2 - s)/2 * ((2 - s) grad_k - 2 (s - 1) sign(u_k) (D - u_k grad_k) / s)
//   p = 2, g_par = (D / s^2) u:                 v   = -(2 - s)/2 * (s (grad - g_par) + (2 - s) g_par)
// -- the header's J with the terms that cancel (2/m against 2/m^2 |X_k| ...) taken out on paper, not in fp32.
__device__ __forceinline__ void to_world(const FrameArgs &fr, const float (&x)[3], const float (&g)[3], float (&v)[3])
{
    if (fr.kind == TN_CONTRACT_NONE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = -g[c];
        return;
    }
    if (fr.kind == TN_CONTRACT_AABB) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = -(fr.scale[c] * g[c]);
        return;
    }
    const float u[3] = {2.0f * x[0], 2.0f * x[1], 2.0f * x[2]};
    const bool inf_norm = fr.kind == TN_CONTRACT_MIP360_INF;
    const float s = inf_norm ? fmaxf(fmaxf(fabsf(u[0]), fabsf(u[1])), fabsf(u[2])) : sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const bool nan_in = u[0] != u[0] || u[1] != u[1] || u[2] != u[2];       // (fmaxf drops a NaN)
    if (nan_in || !(s < 2.0f)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = 0.0f;
        return;
    }
    if (s <= 1.0f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = -0.5f * g[c];
        return;
    }
    const float t = 2.0f - s, half_t = -0.5f * t;
    if (inf_norm) {
        const int k = fabsf(u[0]) == s ? 0 : fabsf(u[1]) == s ? 1 : 2;
        float rest = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) rest += c == k ? 0.0f : u[c] * g[c];
        const float uk = k == 0 ? u[0] : k == 1 ? u[1] : u[2];
        const float sign = uk < 0.0f ? -1.0f : 1.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            v[c] = c == k ? half_t * (t * g[c] - 2.0f * (s - 1.0f) * sign * (rest / s)) : half_t * (s * g[c]);
    } else {
        const float D = u[0] * g[0] + u[1] * g[1] + u[2] * g[2], q = D / (s * s);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float par = q * u[c];
            v[c] = half_t * (s * (g[c] - par) + t * par);
        }
    }
}

// n = v / |v| (0 unless |v| is finite and > 0), taken relative to the largest component: no overflow or underflow of the squares
__device__ __forceinline__ void unit_or_zero(const float (&v)[3], float (&n)[3])
{
    const float mx = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fabsf(v[2]));
    const bool ok = mx > 0.0f && mx < __builtin_inff() && v[0] == v[0] && v[1] == v[1] && v[2] == v[2];
    const float w[3] = {v[0] / mx, v[1] / mx, v[2] / mx};
    const float r = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = ok ? w[c] / r : 0.0f;
}

__device__ __forceinline__ bool finite3(const float (&x)[3])
{
    return fabsf(x[0]) < __builtin_inff() && fabsf(x[1]) < __builtin_inff() && fabsf(x[2]) < __builtin_inff();
}

// one row's outputs: grad as it is, the unit world normal; zeros for a gated row, a zero normal for a non-finite x
__device__ __forceinline__ void write_row(int64_t row, bool gated, const FrameArgs &fr, const float (&x)[3], const float (&g)[3],
                                          float *__restrict__ normals, float *__restrict__ grad)
{
    if (grad) {
#pragma unroll
        for (int c = 0; c < 3; ++c) grad[3 * row + c] = gated ? 0.0f : g[c];
    }
    if (normals) {
        float v[3], nrm[3];
        to_world(fr, x, g, v);
        unit_or_zero(v, nrm);
        const bool zero = gated || !finite3(x);
#pragma unroll
        for (int c = 0; c < 3; ++c) normals[3 * row + c] = zero ? 0.0f : nrm[c];
    }
}

// the tile's rows: lane (h, j) -> row 32 tile + j; live = some row of the tile has a gate != 0 (wave-uniform)
struct TileRow {
    int64_t row, rr;             // rr: a row that can be read (the last one for lanes past n)
    bool valid, gated;
};

__device__ __forceinline__ TileRow tile_row(int64_t tile, int j, int64_t n, const float *__restrict__ gate)
{
    TileRow t;
    t.row = tile * 32 + j;
    t.valid = t.row < n;
    t.rr = t.valid ? t.row : n - 1;
    t.gated = gate != nullptr && gate[t.rr] == 0.0f;
    return t;
}

// ------------------------------------------------------------------------------------------------------------------------ K-Planes
// one float4 channel group of one plane: value (plane_gather's chain, the forward's bits), dP/du and dP/dv inside the forward's cell.
// The four loads are unconditional (plane_gather's pattern): an out-of-bounds tap reads texel 0 and is zeroed afterwards.
__device__ __forceinline__ void plane_value_grad(const float *__restrict__ plane, const tn::PlaneTaps &t, const tn::PlaneCell &pc, int c, float su, float sv,
                                                 f32x4k &val, f32x4k &du, f32x4k &dv)
{
    const char *base = reinterpret_cast<const char *>(plane);
    const auto texel = [&](int off) {
        unsigned boff = (unsigned)((off >= 0 ? off : 0) + c) * 4u;
        asm volatile("" : "+v"(boff));
        return *reinterpret_cast<const f32x4k *>(base + boff);
    };
    const f32x4k zero = f32x4k{0.f, 0.f, 0.f, 0.f};
    f32x4k nw = texel(t.off[0]), ne = texel(t.off[1]), sw = texel(t.off[2]), se = texel(t.off[3]);
    nw = t.off[0] >= 0 ? nw : zero; ne = t.off[1] >= 0 ? ne : zero; sw = t.off[2] >= 0 ? sw : zero; se = t.off[3] >= 0 ? se : zero;
    val = nw * t.w[0];                      // plane_gather's chain (a zeroed texel for its zeroed weight: the same sum)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        val[e] = __builtin_fmaf(ne[e], t.w[1], val[e]);
        val[e] = __builtin_fmaf(sw[e], t.w[2], val[e]);
        val[e] = __builtin_fmaf(se[e], t.w[3], val[e]);
    }
    du = ((ne - nw) * pc.gy + (se - sw) * pc.fy) * su;
    dv = ((sw - nw) * pc.gx + (se - ne) * pc.fx) * sv;
}

// NV float4 groups per lane: C = 8 NV, lane half h owns channels [4 NV h, 4 NV (h + 1)); C = 4 (NV = 1): half 0 owns all four
template <int NV>
__global__ __launch_bounds__(NW * 64) void kplanes_normals_kernel(KpnArgs a, HeadArgs hd, FrameArgs fr, const float *__restrict__ x,
                                                                  int64_t x_stride, int64_t n, const float *__restrict__ gate,
                                                                  float *__restrict__ normals, float *__restrict__ grad)
{
    __shared__ __attribute__((aligned(16))) float w1t[TN_KPLANES_MAX_SCALES * 32 * HID];
    __shared__ __attribute__((aligned(16))) float b1s[HID], w2s[HID];
    __shared__ __attribute__((aligned(16))) float stages[NW][32 * 32];
    stage_head(hd, w1t, b1s, w2s);
    const int lane = tn::lane_id(), j = lane & 31, h = lane >> 5;
    float *stage = stages[threadIdx.x >> 6];
    const int C = a.C, c0 = 4 * NV * h;
    const bool own = c0 < C;
    const int64_t n_tiles = (n + 31) >> 5;
    for (int64_t tile = (int64_t)blockIdx.x * NW + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * NW) {
        const TileRow r = tile_row(tile, j, n, gate);
        const float xs[3] = {x[r.rr * x_stride], x[r.rr * x_stride + 1], x[r.rr * x_stride + 2]};
        float g3[3] = {0.f, 0.f, 0.f};
        if (__ballot(r.valid && !r.gated) != 0ull) {             // a tile whose gates are all 0 reads no texel
            float acc[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) acc[k] = b1s[32 * h + k];
            for (int s = 0; s < a.n_scales; ++s) {
                if (own) {
                    f32x4k prod[NV];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        float u, v;
                        tn::pair_uv(xs, p, u, v);
                        const tn::PlaneTaps t = tn::plane_taps(u, v, a.H[s], a.W[s], C);
                        f32x4k val[NV];
                        tn::plane_gather<NV>(a.planes[s][p], t, c0, val);
#pragma unroll
                        for (int q = 0; q < NV; ++q) prod[q] = p == 0 ? val[q] : prod[q] * val[q];      // (1 * p0) * p1 * p2
                    }
#pragma unroll
                    for (int q = 0; q < NV; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) stage[(c0 + 4 * q + e) * 32 + j] = prod[q][e];
                }
                wave_sync();
                hidden_add(acc, w1t, stage, s * C, C, j, h);
                wave_sync();
            }
            float ak[HID];
            relu_coefficients(acc, w2s, h, ak);
            if (own) {
                for (int s = 0; s < a.n_scales; ++s) {
                    const tn::PlaneTaps t0 = tn::plane_taps(xs[0], xs[1], a.H[s], a.W[s], C);      // pair_uv: (0,1), (0,2), (1,2)
                    const tn::PlaneTaps t1 = tn::plane_taps(xs[0], xs[2], a.H[s], a.W[s], C);
                    const tn::PlaneTaps t2 = tn::plane_taps(xs[1], xs[2], a.H[s], a.W[s], C);
                    const tn::PlaneCell k0 = tn::plane_cell(xs[0], xs[1], a.H[s], a.W[s]), k1 = tn::plane_cell(xs[0], xs[2], a.H[s], a.W[s]),
                                        k2 = tn::plane_cell(xs[1], xs[2], a.H[s], a.W[s]);
                    const float su = 0.5f * (float)(a.W[s] - 1), sv = 0.5f * (float)(a.H[s] - 1);
#pragma unroll 1             // (unrolled, the compiler hoists all 12 NV texel loads and runs out of registers)
                    for (int q = 0; q < NV; ++q) {
                        f32x4k P[3], U[3], V[3];
                        plane_value_grad(a.planes[s][0], t0, k0, c0 + 4 * q, su, sv, P[0], U[0], V[0]);
                        plane_value_grad(a.planes[s][1], t1, k1, c0 + 4 * q, su, sv, P[1], U[1], V[1]);
                        plane_value_grad(a.planes[s][2], t2, k2, c0 + 4 * q, su, sv, P[2], U[2], V[2]);
                        // pairs (0,1), (0,2), (1,2): x0 is u of planes 0 and 1, x1 is v of plane 0 and u of plane 2, x2 is v of planes 1 and 2
                        const f32x4k d0 = U[0] * P[1] * P[2] + P[0] * U[1] * P[2];
                        const f32x4k d1 = V[0] * P[1] * P[2] + P[0] * P[1] * U[2];
                        const f32x4k d2 = P[0] * V[1] * P[2] + P[0] * P[1] * V[2];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float gc = head_g(w1t, s * C + c0 + 4 * q + e, ak);
                            g3[0] = __builtin_fmaf(gc, d0[e], g3[0]);
                            g3[1] = __builtin_fmaf(gc, d1[e], g3[1]);
                            g3[2] = __builtin_fmaf(gc, d2[e], g3[2]);
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) g3[c] += __shfl_xor(g3[c], 32, 64);
        }
        if (r.valid && h == 0) write_row(r.row, r.gated, fr, xs, g3, normals, grad);
    }
}

// ----------------------------------------------------------------------------------------------------------------------- hash grid
template <int F>
struct HgCell {
    uint32_t idx[8];
    float f[3];
    bool live[3];                // the clamp does not act on this axis
};

template <int F>
__device__ __forceinline__ HgCell<F> hg_cell(const tn::HgArgs &a, int l, const float (&xs)[3])
{
    HgCell<F> c;
    const int N = a.res[l];
    const uint32_t S = (uint32_t)N + 1u;
    int i[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        tn::hg_axis_cell(xs[d], N, i[d], c.f[d]);
        const float p = tn::hg_axis_pos(xs[d], N);
        c.live[d] = p >= 0.0f && p <= (float)N;                  // false for a NaN
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        c.idx[k] = tn::hg_node_index(a.hashed[l] != 0, a.mask[l], S, (uint32_t)(i[0] + (k & 1)), (uint32_t)(i[1] + ((k >> 1) & 1)),
                                     (uint32_t)(i[2] + (k >> 2)));
    return c;
}

template <int F>
__global__ __launch_bounds__(NW * 64) void hashgrid_normals_kernel(tn::HgArgs a, HeadArgs hd, FrameArgs fr, const float *__restrict__ x,
                                                                   int64_t x_stride, int64_t n, const float *__restrict__ gate,
                                                                   float *__restrict__ normals, float *__restrict__ grad)
{
    typedef typename tn::HgEntry<F>::type entry_t;
    __shared__ __attribute__((aligned(16))) float w1t[TN_HASHGRID_MAX_LEVELS * 4 * HID];
    __shared__ __attribute__((aligned(16))) float b1s[HID], w2s[HID];
    __shared__ __attribute__((aligned(16))) float stages[NW][TN_HASHGRID_MAX_LEVELS * 4 * 32];
    stage_head(hd, w1t, b1s, w2s);
    const int lane = tn::lane_id(), j = lane & 31, h = lane >> 5;
    float *stage = stages[threadIdx.x >> 6];
    const int64_t n_tiles = (n + 31) >> 5;
    for (int64_t tile = (int64_t)blockIdx.x * NW + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * NW) {
        const TileRow r = tile_row(tile, j, n, gate);
        const float xs[3] = {x[r.rr * x_stride], x[r.rr * x_stride + 1], x[r.rr * x_stride + 2]};
        float g3[3] = {0.f, 0.f, 0.f};
        if (__ballot(r.valid && !r.gated) != 0ull) {             // a tile whose gates are all 0 reads no entry
            for (int l = h; l < a.n_levels; l += 2) {            // the forward's sum, corner by corner
                const HgCell<F> c = hg_cell<F>(a, l, xs);
                const entry_t *tab = reinterpret_cast<const entry_t *>(a.table) + a.offset[l];
                entry_t e[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = tab[c.idx[k]];
                float feat[F];
#pragma unroll
                for (int ch = 0; ch < F; ++ch) feat[ch] = 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float w = ((k & 1) ? c.f[0] : 1.0f - c.f[0]) * ((k & 2) ? c.f[1] : 1.0f - c.f[1]) * ((k & 4) ? c.f[2] : 1.0f - c.f[2]);
                    float v[F];
                    tn::hg_unpack<F>(e[k], v);
#pragma unroll
                    for (int ch = 0; ch < F; ++ch) feat[ch] = fmaf(w, v[ch], feat[ch]);
                }
#pragma unroll
                for (int ch = 0; ch < F; ++ch) stage[(l * F + ch) * 32 + j] = feat[ch];
            }
            wave_sync();
            float acc[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) acc[k] = b1s[32 * h + k];
            hidden_add(acc, w1t, stage, 0, a.feat_dim, j, h);
            wave_sync();
            float ak[HID];
            relu_coefficients(acc, w2s, h, ak);
            for (int l = h; l < a.n_levels; l += 2) {
                const HgCell<F> c = hg_cell<F>(a, l, xs);
                const entry_t *tab = reinterpret_cast<const entry_t *>(a.table) + a.offset[l];
                entry_t e[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = tab[c.idx[k]];
                float d[3][F];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                    for (int ch = 0; ch < F; ++ch) d[ax][ch] = 0.0f;
                const float w0[2] = {1.0f - c.f[0], c.f[0]}, w1[2] = {1.0f - c.f[1], c.f[1]}, w2[2] = {1.0f - c.f[2], c.f[2]};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int b0 = k & 1, b1 = (k >> 1) & 1, b2 = k >> 2;
                    const float s0 = (b0 ? 1.0f : -1.0f) * (w1[b1] * w2[b2]);
                    const float s1 = (b1 ? 1.0f : -1.0f) * (w0[b0] * w2[b2]);
                    const float s2 = (b2 ? 1.0f : -1.0f) * (w0[b0] * w1[b1]);
                    float v[F];
                    tn::hg_unpack<F>(e[k], v);
#pragma unroll
                    for (int ch = 0; ch < F; ++ch) {
                        d[0][ch] = fmaf(s0, v[ch], d[0][ch]);
                        d[1][ch] = fmaf(s1, v[ch], d[1][ch]);
                        d[2][ch] = fmaf(s2, v[ch], d[2][ch]);
                    }
                }
                const float half_n = 0.5f * (float)a.res[l];
#pragma unroll
                for (int ch = 0; ch < F; ++ch) {
                    const float gc = head_g(w1t, l * F + ch, ak);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) g3[ax] = fmaf(gc, c.live[ax] ? half_n * d[ax][ch] : 0.0f, g3[ax]);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) g3[c] += __shfl_xor(g3[c], 32, 64);
        }
        if (r.valid && h == 0) write_row(r.row, r.gated, fr, xs, g3, normals, grad);
    }
}

// ----------------------------------------------------------------------------------------------------------------------- host side
int kpn_make_args(const tn_kplanes_desc *d, KpnArgs &a)
{
    TN_REQUIRE(d, TN_E_NULL, "tn_kplanes_normals: null descriptor");
    TN_REQUIRE(d->n_scales >= 1 && d->n_scales <= TN_KPLANES_MAX_SCALES, TN_E_CONFIG, "tn_kplanes_normals: n_scales out of range");
    TN_REQUIRE(d->channels == 4 || d->channels == 8 || d->channels == 16 || d->channels == 32, TN_E_CONFIG,
               "tn_kplanes_normals: channels must be 4, 8, 16 or 32");
    a.n_scales = d->n_scales; a.C = d->channels;
    for (int s = 0; s < d->n_scales; ++s) {
        TN_REQUIRE(d->height[s] > 0 && d->width[s] > 0, TN_E_SIZE, "tn_kplanes_normals: bad plane resolution");
        TN_REQUIRE((int64_t)d->height[s] * d->width[s] * d->channels < (1ll << 30), TN_E_SIZE, "tn_kplanes_normals: plane too large (2^30 elements)");
        a.H[s] = d->height[s]; a.W[s] = d->width[s];
        for (int p = 0; p < 3; ++p) {
            TN_REQUIRE(d->planes[s][p], TN_E_CONFIG, "tn_kplanes_normals: all three planes of every scale must be present");
            TN_REQUIRE(((uintptr_t)d->planes[s][p] & 15) == 0, TN_E_ALIGN, "tn_kplanes_normals: planes must be 16-byte aligned");
            a.planes[s][p] = d->planes[s][p];
        }
    }
    return TN_OK;
}

int head_args(const tn_mlp_desc *m, int F, HeadArgs &hd)
{
    TN_REQUIRE(m, TN_E_NULL, "normals: null head descriptor");
    TN_REQUIRE(m->n_layers == 2 && m->encoding == TN_ENC_NONE && m->in_dim == F && m->dims[0] == F && m->dims[1] == HID && m->dims[2] == 1,
               TN_E_CONFIG, "normals: the sigma head must be 2 layers, dims {F, 64, 1}, TN_ENC_NONE, F the field's feature width");
    TN_REQUIRE(m->weights[0] && m->biases[0] && m->weights[1], TN_E_NULL, "normals: null head parameter");
    hd.w1 = m->weights[0]; hd.b1 = m->biases[0]; hd.w2 = m->weights[1]; hd.F = F;
    return TN_OK;
}

int frame_args(const tn_normal_frame *f, FrameArgs &fr)
{
    fr.kind = f ? f->contraction : TN_CONTRACT_NONE;
    fr.scale[0] = fr.scale[1] = fr.scale[2] = 1.0f;
    TN_REQUIRE(fr.kind == TN_CONTRACT_AABB || fr.kind == TN_CONTRACT_MIP360_INF || fr.kind == TN_CONTRACT_MIP360_L2 || fr.kind == TN_CONTRACT_NONE,
               TN_E_CONFIG, "normals: unknown frame");
    if (fr.kind == TN_CONTRACT_AABB)
        for (int c = 0; c < 3; ++c) {
            const float ext = f->aabb[3 + c] - f->aabb[c];
            TN_REQUIRE(ext > 0.0f && ext < __builtin_inff(), TN_E_CONFIG, "normals: the frame's box needs finite hi > lo on every axis");
            fr.scale[c] = 2.0f / ext;
        }
    return TN_OK;
}

int call_args(const float *x, int64_t x_stride, int64_t n, const float *normals, const float *grad, bool &done)
{
    TN_REQUIRE(n >= 0 && x_stride >= 3, TN_E_SIZE, "normals: n < 0 or x_stride < 3");
    TN_REQUIRE(n < (1ll << 40), TN_E_SIZE, "normals: too many samples for one launch");
    done = n == 0;
    if (done) return TN_OK;
    TN_REQUIRE(x && (normals || grad), TN_E_NULL, "normals: null x, or neither normals nor grad asked for");
    return TN_OK;
}

inline unsigned tile_blocks(int64_t n) { return (unsigned)std::min<int64_t>(((n + 31) / 32 + NW - 1) / NW, 256 * 8); }

}  // namespace

extern "C" int tn_kplanes_normals(const tn_kplanes_desc *f, const float *x, int64_t x_stride, int64_t n, const tn_mlp_desc *head,
                                  const tn_normal_frame *frame, const float *gate, float *normals, float *grad, void *stream)
{
    KpnArgs a;
    HeadArgs hd;
    FrameArgs fr;
    bool done;
    if (int rc = kpn_make_args(f, a)) return rc;
    if (int rc = head_args(head, a.n_scales * a.C, hd)) return rc;
    if (int rc = frame_args(frame, fr)) return rc;
    if (int rc = call_args(x, x_stride, n, normals, grad, done)) return rc;
    if (done) return TN_OK;
    const dim3 grid(tile_blocks(n)), block(NW * 64);
    hipStream_t s = (hipStream_t)stream;
    switch (a.C) {
    case 4:
    case 8: kplanes_normals_kernel<1><<<grid, block, 0, s>>>(a, hd, fr, x, x_stride, n, gate, normals, grad); break;
    case 16: kplanes_normals_kernel<2><<<grid, block, 0, s>>>(a, hd, fr, x, x_stride, n, gate, normals, grad); break;
    default: kplanes_normals_kernel<4><<<grid, block, 0, s>>>(a, hd, fr, x, x_stride, n, gate, normals, grad); break;
    }
    return tn::check_launch("kplanes_normals_kernel");
}

extern "C" int tn_hashgrid_normals(const tn_hashgrid_desc *f, const float *x, int64_t x_stride, int64_t n, const tn_mlp_desc *head,
                                   const tn_normal_frame *frame, const float *gate, float *normals, float *grad, void *stream)
{
    tn::HgArgs a;
    HeadArgs hd;
    FrameArgs fr;
    bool done;
    if (int rc = tn::hg_make_args(f, a)) return rc;
    if (int rc = head_args(head, a.feat_dim, hd)) return rc;
    if (int rc = frame_args(frame, fr)) return rc;
    if (int rc = call_args(x, x_stride, n, normals, grad, done)) return rc;
    if (done) return TN_OK;
    const dim3 grid(tile_blocks(n)), block(NW * 64);
    hipStream_t s = (hipStream_t)stream;
    if (f->features == 2) hashgrid_normals_kernel<2><<<grid, block, 0, s>>>(a, hd, fr, x, x_stride, n, gate, normals, grad);
    else hashgrid_normals_kernel<4><<<grid, block, 0, s>>>(a, hd, fr, x, x_stride, n, gate, normals, grad);
    return tn::check_launch("hashgrid_normals_kernel");
}
