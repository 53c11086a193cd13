// Multiresolution hash-grid field (Instant-NGP, Mueller et al. 2022; definition: include/tinynerf_hip.h): per level one
// trilinear lookup of the contracted point into a dense or hashed table of F-float entries, levels concatenated.  The level plan
// (resolutions, dense / hashed, offsets) is made on the host and arrives as integers; no kernel computes a resolution.
//
// Mapping, both directions: lane = packed sample (consecutive lanes are neighbours along a ray), blockIdx.y = level.  The hardware
// hands out workgroups x-fastest, so the workgroups in flight at any time work on ONE level (two at a boundary) and that level's table
// -- 4 MB at F = 2, T = 2^19 -- is what the caches hold, not all sixteen.  An entry is one 8- or 16-byte load.
#include "tn_common.h"
#include <stdlib.h>
#include <string.h>

namespace {

struct HgArgs {
    int n_levels, feat_dim;
    int res[TN_HASHGRID_MAX_LEVELS], hashed[TN_HASHGRID_MAX_LEVELS];
    uint32_t mask[TN_HASHGRID_MAX_LEVELS];          // hashed: T - 1
    int64_t offset[TN_HASHGRID_MAX_LEVELS];         // entries
    const float *table;
    float *gtable;
};

template <int F> struct EntryT;
template <> struct EntryT<2> { typedef float2 type; };
template <> struct EntryT<4> { typedef float4 type; };

template <int F> __device__ __forceinline__ void unpack(const typename EntryT<F>::type &e, float (&v)[F]);
template <> __device__ __forceinline__ void unpack<2>(const float2 &e, float (&v)[2]) { v[0] = e.x; v[1] = e.y; }
template <> __device__ __forceinline__ void unpack<4>(const float4 &e, float (&v)[4]) { v[0] = e.x; v[1] = e.y; v[2] = e.z; v[3] = e.w; }
template <int F> __device__ __forceinline__ typename EntryT<F>::type pack(const float (&v)[F]);
template <> __device__ __forceinline__ float2 pack<2>(const float (&v)[2]) { return make_float2(v[0], v[1]); }
template <> __device__ __forceinline__ float4 pack<4>(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }

// cell and fractions of one axis: ONE fused rounding, then a clamp that sends a NaN to 0 and keeps every read inside the table
__device__ __forceinline__ void axis_cell(float xv, int N, int &i, float &f)
{
    const float nf = (float)N, h = 0.5f * nf;        // exact: N <= 2^24
    float p = fmaf(xv, h, h);
    p = p > 0.0f ? p : 0.0f;                         // NaN > 0 is false
    p = p < nf ? p : nf;
    const int ip = (int)p;
    i = ip < N - 1 ? ip : N - 1;
    f = p - (float)i;                                // exact in fp32
}

__device__ __forceinline__ uint32_t node_index(bool hashed, uint32_t mask, uint32_t S, uint32_t ix, uint32_t iy, uint32_t iz)
{
    return hashed ? ((ix ^ (iy * 2654435761u) ^ (iz * 805459861u)) & mask) : ix + S * (iy + S * iz);
}

// MERGE (backward only): lanes of a wave that follow each other INSIDE ONE CELL (samples of a ray on a coarse level) share all eight
// entries.  Their contributions are summed towards the run's first lane with a segmented shuffle reduction and that lane alone issues
// the atomics.  Taken per wave, where at least half of the lanes would drop out; the other waves scatter lane by lane.
template <int F, bool BWD, bool MERGE>
__global__ __launch_bounds__(256) void hashgrid_kernel(HgArgs a, const float *__restrict__ x, int64_t x_stride, int64_t n,
                                                       float *__restrict__ feat, const float *__restrict__ gfeat)
{
    typedef typename EntryT<F>::type entry_t;
    const int l = (int)blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    const int64_t r = valid ? i : n - 1;
    const int N = a.res[l];
    const bool hashed = a.hashed[l] != 0;
    const uint32_t mask = a.mask[l], S = (uint32_t)N + 1u;
    const int FD = a.feat_dim;
    int c0[3];
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) axis_cell(x[r * x_stride + c], N, c0[c], f[c]);
    const float wx[2] = {1.0f - f[0], f[0]}, wy[2] = {1.0f - f[1], f[1]}, wz[2] = {1.0f - f[2], f[2]};
    uint32_t idx[8];
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        idx[k] = node_index(hashed, mask, S, (uint32_t)(c0[0] + dx), (uint32_t)(c0[1] + dy), (uint32_t)(c0[2] + dz));
        w[k] = wx[dx] * wy[dy] * wz[dz];
    }
    if constexpr (!BWD) {
        if (!valid) return;
        const entry_t *tab = reinterpret_cast<const entry_t *>(a.table) + a.offset[l];
        entry_t e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = tab[idx[k]];
        float acc[F];
#pragma unroll
        for (int c = 0; c < F; ++c) acc[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v[F];
            unpack<F>(e[k], v);
#pragma unroll
            for (int c = 0; c < F; ++c) acc[c] = fmaf(w[k], v[c], acc[c]);
        }
        *reinterpret_cast<entry_t *>(feat + i * FD + l * F) = pack<F>(acc);
    } else {
        float g[F];
        {
            entry_t ge = *reinterpret_cast<const entry_t *>(gfeat + r * FD + l * F);
            unpack<F>(ge, g);
        }
        float *gt = a.gtable + a.offset[l] * F;
        bool issue = valid;
        float v[8][F];
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int c = 0; c < F; ++c) v[k][c] = valid ? w[k] * g[c] : 0.0f;
        if constexpr (MERGE) {
            const int lane = tn::lane_id();
            // a lane past n is a run of its own (its cell is not compared), with nothing to add
            const int p0 = __shfl_up(c0[0], 1, 64), p1 = __shfl_up(c0[1], 1, 64), p2 = __shfl_up(c0[2], 1, 64);
            const int pv = __shfl_up((int)valid, 1, 64);
            const bool head = lane == 0 || !valid || !pv || p0 != c0[0] || p1 != c0[1] || p2 != c0[2];
            const uint64_t heads = __ballot(head);
            if (2 * __popcll(heads) <= 64) {                         // wave-uniform
                const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
                const int dist = above ? __builtin_ctzll(above) : 63 - lane;       // lanes behind this one in its run
#pragma unroll 1
                for (int o = 1; o < 64; o <<= 1) {
                    if (__ballot(o <= dist) == 0ull) break;           // wave-uniform: no run is longer
#pragma unroll
                    for (int k = 0; k < 8; ++k)
#pragma unroll
                        for (int c = 0; c < F; ++c) {
                            const float t = __shfl_down(v[k][c], o, 64);
                            v[k][c] += o <= dist ? t : 0.0f;
                        }
                }
                issue = valid && head;
            }
        }
        if (issue) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int c = 0; c < F; ++c) atomicAdd(gt + (int64_t)idx[k] * F + c, v[k][c]);
        }
    }
}

int make_args(const tn_hashgrid_desc *d, HgArgs &a)
{
    TN_REQUIRE(d, TN_E_NULL, "hashgrid: null descriptor");
    TN_REQUIRE(d->n_levels >= 1 && d->n_levels <= TN_HASHGRID_MAX_LEVELS, TN_E_CONFIG, "hashgrid: n_levels must be in [1, 16]");
    TN_REQUIRE(d->features == 2 || d->features == 4, TN_E_CONFIG, "hashgrid: features must be 2 or 4");
    a.n_levels = d->n_levels;
    a.feat_dim = d->n_levels * d->features;
    for (int l = 0; l < d->n_levels; ++l) {
        TN_REQUIRE(d->res[l] >= 1 && d->res[l] <= (1 << 24), TN_E_CONFIG, "hashgrid: a level's resolution must be in [1, 2^24]");
        const int64_t e = d->entries[l];
        if (d->hashed[l]) {
            TN_REQUIRE(e >= 1 && e <= (1ll << 32) && (e & (e - 1)) == 0, TN_E_CONFIG,
                       "hashgrid: a hashed level's entries must be a power of two (<= 2^32)");
            a.mask[l] = (uint32_t)(e - 1);
        } else {
            const int64_t s = (int64_t)d->res[l] + 1;
            TN_REQUIRE(s <= 1290 && e >= s * s * s, TN_E_CONFIG, "hashgrid: a dense level needs entries >= (res + 1)^3 (< 2^31)");
            a.mask[l] = 0;
        }
        TN_REQUIRE(d->offset[l] >= 0 && d->offset[l] <= (1ll << 40), TN_E_CONFIG, "hashgrid: bad level offset");
        for (int m = 0; m < l; ++m)
            TN_REQUIRE(d->offset[l] + e <= d->offset[m] || d->offset[m] + d->entries[m] <= d->offset[l], TN_E_CONFIG,
                       "hashgrid: levels overlap in the table");
        a.res[l] = d->res[l]; a.hashed[l] = d->hashed[l] ? 1 : 0; a.offset[l] = d->offset[l];
    }
    TN_REQUIRE(d->table, TN_E_NULL, "hashgrid: null table");
    TN_REQUIRE(((uintptr_t)d->table & 15) == 0, TN_E_ALIGN, "hashgrid: table must be 16-byte aligned");
    a.table = d->table;
    a.gtable = nullptr;
    return TN_OK;
}

// TN_HASHGRID_SCATTER=plain / merged in the environment: A/B of the two scatter forms (LABNOTES); anything else: the default
bool merged_scatter()
{
    static const int mode = [] {
        const char *e = getenv("TN_HASHGRID_SCATTER");
        return e && !strcmp(e, "plain") ? 0 : 1;
    }();
    return mode != 0;
}

int check_call(const char *who, const float *x, int64_t x_stride, int64_t n)
{
    (void)who; (void)x;
    TN_REQUIRE(n >= 0 && x_stride >= 3, TN_E_SIZE, "hashgrid: n < 0 or x_stride < 3");
    TN_REQUIRE((n + 255) / 256 < (1ll << 31), TN_E_SIZE, "hashgrid: too many samples for one launch");
    return TN_OK;
}

}  // namespace

extern "C" int tn_hashgrid_fwd(const tn_hashgrid_desc *desc, const float *x, int64_t x_stride, int64_t n, float *feat, void *stream)
{
    HgArgs a;
    if (int rc = make_args(desc, a)) return rc;
    if (int rc = check_call("tn_hashgrid_fwd", x, x_stride, n)) return rc;
    if (n == 0) return TN_OK;
    TN_REQUIRE(x && feat, TN_E_NULL, "tn_hashgrid_fwd: null pointer");
    TN_REQUIRE(((uintptr_t)feat & 15) == 0, TN_E_ALIGN, "tn_hashgrid_fwd: feat must be 16-byte aligned");
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)a.n_levels), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (desc->features == 2) hashgrid_kernel<2, false, false><<<grid, block, 0, s>>>(a, x, x_stride, n, feat, nullptr);
    else hashgrid_kernel<4, false, false><<<grid, block, 0, s>>>(a, x, x_stride, n, feat, nullptr);
    return tn::check_launch("tn_hashgrid_fwd");
}

extern "C" int tn_hashgrid_bwd(const tn_hashgrid_desc *desc, const float *x, int64_t x_stride, int64_t n, const float *grad_feat,
                               float *grad_table, void *stream)
{
    HgArgs a;
    if (int rc = make_args(desc, a)) return rc;
    if (int rc = check_call("tn_hashgrid_bwd", x, x_stride, n)) return rc;
    TN_REQUIRE(grad_table, TN_E_NULL, "tn_hashgrid_bwd: null grad_table");
    TN_REQUIRE(((uintptr_t)grad_table & 15) == 0, TN_E_ALIGN, "tn_hashgrid_bwd: grad_table must be 16-byte aligned");
    if (n == 0) return TN_OK;
    TN_REQUIRE(x && grad_feat, TN_E_NULL, "tn_hashgrid_bwd: null pointer");
    TN_REQUIRE(((uintptr_t)grad_feat & 15) == 0, TN_E_ALIGN, "tn_hashgrid_bwd: grad_feat must be 16-byte aligned");
    a.gtable = grad_table;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)a.n_levels), block(256);
    hipStream_t s = (hipStream_t)stream;
    const bool merge = merged_scatter();
    if (desc->features == 2) {
        if (merge) hashgrid_kernel<2, true, true><<<grid, block, 0, s>>>(a, x, x_stride, n, nullptr, grad_feat);
        else hashgrid_kernel<2, true, false><<<grid, block, 0, s>>>(a, x, x_stride, n, nullptr, grad_feat);
    } else {
        if (merge) hashgrid_kernel<4, true, true><<<grid, block, 0, s>>>(a, x, x_stride, n, nullptr, grad_feat);
        else hashgrid_kernel<4, true, false><<<grid, block, 0, s>>>(a, x, x_stride, n, nullptr, grad_feat);
    }
    return tn::check_launch("tn_hashgrid_bwd");
}
