// Hash-grid position and index arithmetic (definition: include/tinynerf_hip.h), shared by the field's forward / backward
// (hashgrid.hip) and the density-gradient kernel (normals.hip): one text, so the cell a derivative is taken in is the cell the
// forward interpolated in.
#pragma once
#include "tn_common.h"

namespace tn {

template <int F> struct HgEntry;
template <> struct HgEntry<2> { typedef float2 type; };
template <> struct HgEntry<4> { typedef float4 type; };

template <int F> __device__ __forceinline__ void hg_unpack(const typename HgEntry<F>::type &e, float (&v)[F]);
template <> __device__ __forceinline__ void hg_unpack<2>(const float2 &e, float (&v)[2]) { v[0] = e.x; v[1] = e.y; }
template <> __device__ __forceinline__ void hg_unpack<4>(const float4 &e, float (&v)[4]) { v[0] = e.x; v[1] = e.y; v[2] = e.z; v[3] = e.w; }
template <int F> __device__ __forceinline__ typename HgEntry<F>::type hg_pack(const float (&v)[F]);
template <> __device__ __forceinline__ float2 hg_pack<2>(const float (&v)[2]) { return make_float2(v[0], v[1]); }
template <> __device__ __forceinline__ float4 hg_pack<4>(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }

// position of one axis before the clamp: ONE fused rounding
__device__ __forceinline__ float hg_axis_pos(float xv, int N)
{
    const float h = 0.5f * (float)N;                 // exact: N <= 2^24
    return fmaf(xv, h, h);
}

// cell and fractions of one axis: the fused rounding, then a clamp that sends a NaN to 0 and keeps every read inside the table
__device__ __forceinline__ void hg_axis_cell(float xv, int N, int &i, float &f)
{
    const float nf = (float)N;
    float p = hg_axis_pos(xv, N);
    p = p > 0.0f ? p : 0.0f;                         // NaN > 0 is false
    p = p < nf ? p : nf;
    const int ip = (int)p;
    i = ip < N - 1 ? ip : N - 1;
    f = p - (float)i;                                // exact in fp32
}

__device__ __forceinline__ uint32_t hg_node_index(bool hashed, uint32_t mask, uint32_t S, uint32_t ix, uint32_t iy, uint32_t iz)
{
    return hashed ? ((ix ^ (iy * 2654435761u) ^ (iz * 805459861u)) & mask) : ix + S * (iy + S * iz);
}

// the level plan as the kernels take it
struct HgArgs {
    int n_levels, feat_dim;
    int res[TN_HASHGRID_MAX_LEVELS], hashed[TN_HASHGRID_MAX_LEVELS];
    uint32_t mask[TN_HASHGRID_MAX_LEVELS];          // hashed: T - 1
    int64_t offset[TN_HASHGRID_MAX_LEVELS];         // entries
    const float *table;
    float *gtable;
};

// descriptor checks of every hash-grid entry point (TN_E_* as the header lists them) and the kernel arguments
inline int hg_make_args(const tn_hashgrid_desc *d, HgArgs &a)
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

}  // namespace tn
