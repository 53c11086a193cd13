// Shared pieces of the layer-by-layer kernels of the wide stacks, each written once for the three arithmetic forms
// (mlp_bwd_layers.hip: exact fp32 MFMA; mlp_b3_layers.hip: bf16 MFMA with exact three-way operand splits; mlp_f2_layers.hip: fp16
// MFMA with two-term splits and power-of-two scales).  The forms keep their own kernels, k loops, staging and waits; what they
// share lives here:
//   * the argument structs of a layer's forward, data gradient and weight gradient;
//   * the [feature][32-sample] row helpers in the SGPR-base form (urow, wreg_*), request_rows (LDS-direct staging);
//   * TileWalk: lane / wave / stream split of a workgroup and the tiles its streams visit;
//   * read_weight_rows / read_weight_cols: the eight weights a lane feeds to a k step of its block;
//   * emit_last_narrow / emit_last_full: the epilogues of the last layer;
//   * the weight-gradient kernels' chunk tables, half-tile bases, operand offsets, flush_tiles and flush_bias;
//   * for_width and stream_blocks: run-time width -> instantiation, grid of a stream kernel (launched through tn::mlp::launch);
//   * the entry points of the bf16x3 / f16x2 files and of the cross-layer launches (mlp_fused_f2.hip).
#pragma once
#include "mlp_stage.h"
#include <algorithm>
#include <type_traits>

namespace tn {
namespace layers {

using tn::f32x16;
using tn::f32x4;
using tn::frow;
using tn::mlp::glds16;
using tn::mlp::global_char;
using tn::mlp::wave_uniform_global;

// data gradient of one layer:  Gout = relu'(Hmask) * (W^T Gin)      (FIRST: grad_x, no mask, row-major out)
struct DgradArgs {
    const float *W;       // [N][K] torch layout
    int N, K;             // rows / columns of W
    int rows_total;       // stash rows per tile: row set at offset `off` of tile t = rows [t rows_total + off, ...) of the workspace
    int64_t off_gin, off_gout, off_mask;    // row offsets (tile-major layout: inside a tile; slab layout: slab base + offset inside the slab's tile, see RowMap)
    int64_t off_bits;                   // >= 0: ReLU bit rows of the mask activation (dgrad_wreg_kernel), else float mask rows
    int enc, in_dim, n_freqs;           // FIRST only: column permutation of layer 0
    int accum_gx;                       // FIRST only: grad_x += (TN_MLP_ACCUM_GRAD_X)
    float *max_in = nullptr;            // f16x2: receives the largest |value| of the rows at off_gin (atomic max; scale of the layer's weight gradient)
};

// forward of one layer on workspace rows
struct FwdLayerArgs {
    const float *W, *B;   // [N][K] torch layout, [N]
    int N, K;
    int Kp;               // input rows present in the workspace (K for hidden layers, K0_pad for the encoded first layer)
    int rows_total;
    int64_t off_in, off_out;
    int out_act;
    int64_t off_bits;     // >= 0: the output activation's ReLU bits go to these rows (2 per 32-feature block), < 0: not wanted
    float *max_in = nullptr;            // f16x2: receives the largest |value| of the rows at off_in (see DgradArgs)
};

// weight gradient of one layer: dW[N][K] += G[N][s] A[K][s]^T over all samples; db[N] += sum_s G
struct WgradArgs {
    float *gW, *gB;
    int N, K, K_pad;
    int rows_total;
    int64_t off_g, off_a, off_e;
    int first, enc, in_dim, n_freqs, xs;
    const float *g_max = nullptr, *a_max = nullptr;       // f16x2: largest |value| of the G rows / of the A rows over ALL tiles
};

// Vector-memory instructions of these kernels use the SGPR-base form (wave-uniform 64-bit base + one 32-bit lane offset +
// immediate): a 64-bit per-lane address costs the SIMD measurably more matrix-pipe time per instruction
// (scripts/microbench/wreg_layer.hip: 84.8 -> 87.8 % busy for the same loads and stores).
__device__ __forceinline__ const float *urow(const float *base, int64_t row) {          // wave-uniform row pointer
    const int64_t o = row * 32;
    return base + (((int64_t)__builtin_amdgcn_readfirstlane((int)(o >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)o));
}
__device__ __forceinline__ float *urow(float *base, int64_t row) { return const_cast<float *>(urow(const_cast<const float *>(base), row)); }

// the 32 rows [32 ob, 32 ob + 32) of a [row][32 samples] tile -> registers (lane (j, h): rows 32 ob + 16 h + 0..15, sample j)
__device__ __forceinline__ void wreg_load_rows(const float *__restrict__ rows, int ob, int j, int h, float (&stage)[16]) {
    const char *p = reinterpret_cast<const char *>(rows + 32 * ob * 32);
    unsigned off = (unsigned)(16 * h * 32 + j) * 4u;
    asm volatile("" : "+v"(off));       // (keeps the zero-extension next to the access: base + zext(off) selects the SGPR-base form)
#pragma unroll
    for (int e = 0; e < 16; ++e) stage[e] = *reinterpret_cast<const float *>(p + off + (unsigned)(e * 128));
}
// D-layout rows of block `ob` (lane (j, h), reg r: row 32 ob + frow(r, h), sample j) from / to [row][32 samples] rows
// (NT: non-temporal stores -- rows that the next launch streams once and nobody re-reads from a cache)
template <bool NT = false>
__device__ __forceinline__ void wreg_store_block(float *__restrict__ rows, int ob, int j, int h, const f32x16 &v) {
    char *p = reinterpret_cast<char *>(rows + 32 * ob * 32);
    unsigned off = (unsigned)(4 * h * 32 + j) * 4u;
    asm volatile("" : "+v"(off));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float *d = reinterpret_cast<float *>(p + off + (unsigned)(((r & 3) + 8 * (r >> 2)) * 128));
        if constexpr (NT) __builtin_nontemporal_store(v[r], d); else *d = v[r];
    }
}
__device__ __forceinline__ void wreg_load_block(const float *__restrict__ rows, int ob, int j, int h, float (&m)[16]) {
    const char *p = reinterpret_cast<const char *>(rows + 32 * ob * 32);
    unsigned off = (unsigned)(4 * h * 32 + j) * 4u;
    asm volatile("" : "+v"(off));
#pragma unroll
    for (int r = 0; r < 16; ++r) m[r] = *reinterpret_cast<const float *>(p + off + (unsigned)(((r & 3) + 8 * (r >> 2)) * 128));
}
// ... -> LDS tile [sample j][feature]: four ds_write_b128
__device__ __forceinline__ void wreg_write_rows(float *__restrict__ tile, int SW, int ob, int j, int h, const float (&stage)[16]) {
    float *p = tile + j * SW + 32 * ob + 16 * h;
#pragma unroll
    for (int v = 0; v < 4; ++v)
        *reinterpret_cast<f32x4 *>(p + 4 * v) = f32x4{stage[4 * v], stage[4 * v + 1], stage[4 * v + 2], stage[4 * v + 3]};
}

// LDS-direct request of NROWS (multiple of 8) rows of a tile, starting at row r0 of `rows` ([row][32 samples]) -> stage
// (lane-linear: one instruction = 8 rows x 128 B = 1 KB, 16 B per lane)
template <int NROWS, bool NT = false>
__device__ __forceinline__ void request_rows(const float *rows, int r0, float *stage, int lane) {
    const float *src = rows + r0 * 32 + 4 * lane;
#pragma unroll
    for (int e = 0; e < NROWS / 8; ++e) glds16<NT>(src + e * 256, stage + e * 256);
}

// A workgroup of STREAMS tile streams with WPS waves each: lane (j, h), wave `wib` of stream `stream`.  Stream s of workgroup b
// visits tiles b STREAMS + s + it * stride; every stream of a workgroup runs `iters` iterations (defined by the workgroup's lowest
// tile), a stream past the end repeats the last tile (same inputs -> same values) rather than branching around its stores.
template <int STREAMS, int WPS>
struct TileWalk {
    int lane, j, h, wave, stream, wib;
    int64_t n_tiles, stride, first, iters;
    __device__ __forceinline__ void init(int64_t n) {
        lane = tn::lane_id(); j = lane & 31; h = lane >> 5;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        stream = wave / WPS; wib = wave % WPS;
        n_tiles = (n + 31) >> 5;
        stride = (int64_t)gridDim.x * STREAMS;
        first = (int64_t)blockIdx.x * STREAMS;
        iters = first < n_tiles ? (n_tiles - first + stride - 1) / stride : 0;
    }
    __device__ __forceinline__ int64_t tile_of(int64_t it) const { const int64_t t = first + stream + it * stride; return t < n_tiles ? t : n_tiles - 1; }
};

// The eight weights lane (i, h) feeds to k step s (of KS) of its 32-row block, handed to use(s, v) step by step:
// by rows (forward): W[row][16 s + 8 h + 0..7], zeros where the row does not exist ...
template <int KS, class F>
__device__ __forceinline__ void read_weight_rows(const float *__restrict__ W, int ldw, int row, bool ok, int h, F use) {
    const float *wr = W + (int64_t)(ok ? row : 0) * ldw + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const f32x4 w0 = *reinterpret_cast<const f32x4 *>(wr + 16 * s), w1 = *reinterpret_cast<const f32x4 *>(wr + 16 * s + 4);
        float v[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
        if (!ok) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.0f;
        }
        use(s, v);
    }
}
// ... and by columns (data gradient, A = W^T): W[16 s + 8 h + e][col]
template <int KS, class F>
__device__ __forceinline__ void read_weight_cols(const float *__restrict__ W, int ldw, int col, int h, F use) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = W[(int64_t)(16 * s + 8 * h + e) * ldw + col];
        use(s, v);
    }
}

// ---- epilogues of the last layer: block `ob` of tile `tile`, acc = the block's pre-activations in the D layout ----
// Output narrower than the stack (N < H; the caller has tested 32 ob < N): pre-activation rows, zero where the sample or the
// feature does not exist, and y = act(pre) as 16-byte stores where N % 4 == 0, else element by element.  Conditional stores: the
// tile's wait counts nothing behind them.
__device__ __forceinline__ void emit_last_narrow(const FwdLayerArgs &a, int64_t n, float *__restrict__ stash, float *__restrict__ y, int64_t tile,
                                                 int ob, int j, int h, const f32x16 &acc) {
    float *outp = stash + (tile * a.rows_total + a.off_out + 32 * ob + 4 * h) * 32 + j;
    const int64_t row = tile * 32 + j;
    const bool valid = row < n;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int f = 32 * ob + 8 * q + 4 * h;
        f32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = valid && f + u < a.N;
            outp[(u + 8 * q) * 32] = ok ? acc[4 * q + u] : 0.0f;
            v[u] = tn::apply_act(acc[4 * q + u], a.out_act);
        }
        if (valid) {
            if ((a.N & 3) == 0) { if (f < a.N) *reinterpret_cast<f32x4 *>(y + row * a.N + f) = v; }
            else {
#pragma unroll
                for (int u = 0; u < 4; ++u) if (f + u < a.N) y[row * a.N + f + u] = v[u];
            }
        }
    }
}
// Full-width output (N == H, the feature stacks): pre-activation rows through the SGPR-base stores (16 per block), then y as four
// 16-byte stores per block -- a FIXED number of vector-memory operations behind the k loop's request (a tile always holds a valid
// sample, so the y stores are issued), which the tile's counted wait relies on.  NULL_Y: y may be null (TN_MLP_ROWS_ONLY: the
// consumer reads the rows); a kernel that counts the y stores in its wait does not take that form.
template <int H, bool NULL_Y>
__device__ __forceinline__ void emit_last_full(const FwdLayerArgs &a, int64_t n, float *__restrict__ stash, float *__restrict__ y, int64_t tile,
                                               int ob, int j, int h, const f32x16 &acc) {
    const int64_t row = tile * 32 + j;
    const bool valid = row < n;
    f32x16 pre;
#pragma unroll
    for (int r = 0; r < 16; ++r) pre[r] = valid ? acc[r] : 0.0f;
    wreg_store_block(urow(stash, tile * a.rows_total + a.off_out), ob, j, h, pre);
    if (NULL_Y && y == nullptr) return;
    float *yr = y + (valid ? row : 0) * H + 32 * ob + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = tn::apply_act(acc[4 * q + u], a.out_act);
        if (valid) *reinterpret_cast<f32x4 *>(yr + 8 * q) = v;
    }
}

// ---- pieces of the weight-gradient kernels of the square hidden layers (wgrad_b3_kernel, wgrad_f2_kernel: half tiles of 16
// samples as split operands [row][RS halfs] in LDS, G rows [0, H), A rows [H, 2 H); flush_tiles: wgrad_lds_kernel too) ----
// this thread's 16-byte chunks (4 samples of a row) of a half tile: chunk id = threadIdx.x + TH c -> row id / 4, samples 4 (id % 4) .. + 3
template <int H, int TH, int RS>
struct WgradChunks {
    static constexpr int NCH = (2 * H * 4) / TH;       // G chunks come first (c < NCH / 2)
    static_assert(NCH * TH == 2 * H * 4 && NCH >= 2 && (NCH & 1) == 0, "the waves own all tiles, every thread holds G and A chunks");
    unsigned src_boff[NCH];                            // byte offset relative to the half tile's G rows / A rows
    int dst_off[NCH];                                  // element offset in an LDS plane
    __device__ __forceinline__ void init() {
        const int qd = threadIdx.x & 3;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int row = (threadIdx.x + TH * c) >> 2;
            src_boff[c] = (unsigned)((row < H ? row : row - H) * 32 + 4 * qd) * 4u;
            dst_off[c] = row * RS + 4 * qd;
        }
    }
};
// The workgroup's tiles (dealt round-robin: blockIdx.x + k gridDim.x, clamped) as half tiles `it`: tile it / 2, samples 16 (it & 1) .. + 15
struct HalfBases { const global_char *g, *a; };                   // wave-uniform: the half tile's G rows and A rows
__device__ __forceinline__ int64_t wgrad_half_tiles(int64_t n_tiles) {
    return (int64_t)blockIdx.x < n_tiles ? 2 * ((n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x) : 0;
}
__device__ __forceinline__ HalfBases half_src(const WgradArgs &a, const float *stash, int64_t n_tiles, int64_t it) {
    int64_t tile = blockIdx.x + (it >> 1) * (int64_t)gridDim.x;
    tile = tile < n_tiles ? tile : n_tiles - 1;
    return HalfBases{wave_uniform_global(stash + (tile * a.rows_total + a.off_g) * 32 + 16 * (it & 1)),
                     wave_uniform_global(stash + (tile * a.rows_total + a.off_a) * 32 + 16 * (it & 1))};
}
// LDS element offsets of lane (i, h)'s operands: samples 8 h .. + 7 of row i of the wave's G blocks tn0 .. / A blocks tk0 ..
template <int H, int RS, int BN, int BK>
__device__ __forceinline__ void wgrad_operand_offsets(int tn0, int tk0, int i, int h, int (&g_off)[BN], int (&a_off)[BK]) {
#pragma unroll
    for (int bn = 0; bn < BN; ++bn) g_off[bn] = (32 * (tn0 + bn) + i) * RS + 8 * h;
#pragma unroll
    for (int bk = 0; bk < BK; ++bk) a_off[bk] = (H + 32 * (tk0 + bk) + i) * RS + 8 * h;
}
// flush of a wave's BN x BK accumulator tiles: gW[n][k] += acc * scale as full-line atomics (lanes = consecutive columns of one
// weight row).  PIN: tn::pin16 on each tile first (see there); kernels that hold the whole accumulator file wait instead.
template <bool PIN, int BN, int BK>
__device__ __forceinline__ void flush_tiles(const WgradArgs &a, int tn0, int tk0, int i, int h, f32x16 (&acc)[BN][BK], float scale) {
#pragma unroll
    for (int bn = 0; bn < BN; ++bn)
#pragma unroll
        for (int bk = 0; bk < BK; ++bk) {
            if constexpr (PIN) tn::pin16(acc[bn][bk]);
            float *col = a.gW + 32 * (tk0 + bk) + i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nn = 32 * (tn0 + bn) + frow(r, h);
                atomicAdd(&col[(int64_t)nn * a.K], acc[bn][bk][r] * scale);
            }
        }
}
// bias gradient summed by the threads that convert G chunks: the four threads of a row (quarters of the 16 samples) are neighbours
template <int TH, int NG>
__device__ __forceinline__ void flush_bias(float *gB, const float (&dbacc)[NG]) {
#pragma unroll
    for (int c = 0; c < NG; ++c) {
        float sgm = dbacc[c];
        sgm += __shfl_xor(sgm, 1, 64);
        sgm += __shfl_xor(sgm, 2, 64);
        const int row = (threadIdx.x + TH * c) >> 2;
        if ((threadIdx.x & 3) == 0) atomicAdd(&gB[row], sgm);
    }
}

// ---- host side ----
// the run-time width of a wide stack -> the <128> / <256> instantiation: f(std::integral_constant<int, H>)
template <class F>
int for_width(int H, const char *else_fail, F f) {
    if (H == 256) return f(std::integral_constant<int, 256>{});
    if (H == 128) return f(std::integral_constant<int, 128>{});
    return tn::fail(TN_E_CONFIG, else_fail);
}
// grid of a stream kernel: `streams` tiles per workgroup and round, one workgroup per CU (n >= 1)
inline int64_t stream_blocks(int64_t n, int streams) { return tn::mlp::grid_blocks(n, streams, 256); }

// ---- bf16x3 forms (mlp_b3_layers.hip); same arguments, same workspace layout, results equal to fp32 rounding ----
int launch_fwd_b3(int H, bool last, const FwdLayerArgs &f, int64_t n, float *stash, float *y, hipStream_t s);
int launch_dgrad_b3(int H, const DgradArgs &d, int64_t n, float *stash, hipStream_t s);
int launch_wgrad_b3(int H, const WgradArgs &w, int64_t n, const float *stash, hipStream_t s);
// ---- f16x2 forms of the forward / data gradient (mlp_f2_layers.hip): two-term fp16 splits with power-of-two scales ----
int launch_fwd_f2(int H, bool last, const FwdLayerArgs &f, int64_t n, float *stash, float *y, hipStream_t s);
int launch_fwd_first_f2(int H, const FwdLayerArgs &f, int64_t n, float *stash, hipStream_t s);
int launch_dgrad_f2(int H, const DgradArgs &d, int64_t n, float *stash, hipStream_t s);
int launch_wgrad_f2(int H, const WgradArgs &w, int64_t n, const float *stash, hipStream_t s);

// ---- all layers of a wide stack in one persistent launch (mlp_fused_f2.hip, round 6): inference forward and training forward ----
struct FusedStash {                 // training forward: where the rows the layer-wise backward reads go (RowMap, slab layout)
    float *rows;                    // workspace base
    int rows_total;
    int64_t off_e;                  // the encoded input rows (written by enc_rows_kernel before the launch)
    int n_run;                      // layers to evaluate: n_layers, or n_layers - 1 under TN_MLP_SKIP_LAST
    int64_t off_out[TN_MLP_MAX_LAYERS], off_bits[TN_MLP_MAX_LAYERS];
    float *tail;                    // tail[l]: largest |input value| of layer l (l >= 1), zeroed by the caller
};
struct FusedChain {                 // data-gradient chain: chain position i = layer top - i
    float *rows; int rows_total;
    int64_t off_in;                 // the gradient it starts from
    int64_t off_out[TN_MLP_MAX_LAYERS], off_bits[TN_MLP_MAX_LAYERS];
    int tail_idx[TN_MLP_MAX_LAYERS];
    float *tail;
};
int launch_fused_chain_f2(int H, const tn::mlp::MlpArgs &a, int top, int64_t n, void *pack_area, hipStream_t s, const FusedChain *spec);
int64_t fused_pack_bytes(int H, int L);
int launch_fused_fwd_f2(int H, const tn::mlp::MlpArgs &a, int64_t n, const float *e_rows, float *y, void *pack_area, hipStream_t s, const FusedStash *spec = nullptr);

}  // namespace layers
}  // namespace tn
