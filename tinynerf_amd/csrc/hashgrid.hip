// Multiresolution hash-grid field (Instant-NGP, Mueller et al. 2022; definition: include/tinynerf_hip.h): per level one
// trilinear lookup of the contracted point into a dense or hashed table of F-float entries, levels concatenated.  The level plan
// (resolutions, dense / hashed, offsets) is made on the host and arrives as integers; no kernel computes a resolution.
//
// Mapping, both directions: lane = packed sample (consecutive lanes are neighbours along a ray), blockIdx.y = level.  The hardware
// hands out workgroups x-fastest, so the workgroups in flight at any time work on ONE level (two at a boundary) and that level's table
// -- 4 MB at F = 2, T = 2^19 -- is what the caches hold, not all sixteen.  An entry is one 8- or 16-byte load.
#include "hashgrid_device.h"
#include <stdlib.h>
#include <string.h>

namespace {

using tn::HgArgs;
template <int F> using EntryT = tn::HgEntry<F>;

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
    for (int c = 0; c < 3; ++c) tn::hg_axis_cell(x[r * x_stride + c], N, c0[c], f[c]);
    const float wx[2] = {1.0f - f[0], f[0]}, wy[2] = {1.0f - f[1], f[1]}, wz[2] = {1.0f - f[2], f[2]};
    uint32_t idx[8];
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        idx[k] = tn::hg_node_index(hashed, mask, S, (uint32_t)(c0[0] + dx), (uint32_t)(c0[1] + dy), (uint32_t)(c0[2] + dz));
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
            tn::hg_unpack<F>(e[k], v);
#pragma unroll
            for (int c = 0; c < F; ++c) acc[c] = fmaf(w[k], v[c], acc[c]);
        }
        *reinterpret_cast<entry_t *>(feat + i * FD + l * F) = tn::hg_pack<F>(acc);
    } else {
        float g[F];
        {
            entry_t ge = *reinterpret_cast<const entry_t *>(gfeat + r * FD + l * F);
            tn::hg_unpack<F>(ge, g);
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

inline int make_args(const tn_hashgrid_desc *d, HgArgs &a) { return tn::hg_make_args(d, a); }

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
