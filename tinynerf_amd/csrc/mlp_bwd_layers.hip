// Backward of WIDE / DEEP fused MLPs (Vanilla feature stack 60->256x9->256, Cobafa 36->128x6), layer by
// layer.  The register-resident form (mlp_bwd2.hip) needs every hidden activation of a tile on
// chip; a 9 x 256 stack does not fit.  This path keeps the same transposed MFMA building blocks but runs
//
//   1 launch   forward that streams every hidden activation H_l to the workspace ([feature][32 samples]
//              rows, as in mlp_bwd2.hip) and leaves the output gradient g = dL/dy * act'(pre) there too;
//   per layer  wgrad (dW_l += G_l H_l^T, sample-reducing MFMA tiles) and dgrad
//              (G_{l-1} = relu'(H_l) * W_l^T G_l, or grad_x for the first layer),
//
// i.e. 2L+1 launches with all activations crossing HBM exactly once in each direction (the reference's
// autograd does the same through cuBLAS with NHW-major activations and separate bias / ReLU kernels).
// Weights are read from L2 (256x256 fp32 = 256 KiB per layer does not fit LDS next to anything else).
#include "mlp_layers.h"
#include <algorithm>

extern "C" int tn_mlp_wgrad_rows(const float *g_rows, int64_t g_stride, int ng, const float *a_rows, int64_t a_stride, int na, float *gW,
                                 int ldw, int col0, int kmax, float *gB, int64_t n, void *stream);

namespace {

using tn::f32x16;
using tn::f32x4;
using namespace tn::mlp;
using namespace tn::layers;

using tn::act_grad;

// D-layout tile -> rows [feature][32 samples], one 64-bit address per lane (tn::mlp::store_rows is the SGPR-base form)
__device__ __forceinline__ void store_rows_lane(float *__restrict__ rows, const f32x16 &t, int ob, int j, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) rows[(32 * ob + frow(r, h)) * 32 + j] = t[r];
}

// behind the last tile of a training workspace: the largest |value| of every layer's input rows ([0, 16): activations, reported
// by the f16x2 forward of layer l; [16, 32): gradients, by its data gradient) -- the scales of the f16x2 weight gradient
constexpr int64_t WS_TAIL_BYTES = 256;
__host__ inline float *ws_tail(float *stash, int64_t total_rows) { return stash + total_rows * 32; }
// behind the tail: the packed weight stream of the cross-layer forward (mlp_fused_f2.hip), 256-byte aligned
__host__ inline int64_t fused_pack_offset(int64_t total_rows) { return (total_rows * 128 + WS_TAIL_BYTES + 255) & ~(int64_t)255; }

__host__ __device__ inline bool plain_x_rows(int H, int n_layers, int enc, int K0_pad, int out_dim) {
    return enc == TN_ENC_NONE && K0_pad <= 64 && H >= 128 && n_layers >= 3 && out_dim > 4 && out_dim <= H;     // (= layer_kernel_path)
}

struct Layout {            // rows (of 32 floats) per 32-sample tile
    int rowsH, rowsE, rowsG, rowsM, total;
    int xs;                // first-layer slots that are plain x columns
};
__host__ __device__ inline Layout make_layout(int H, int n_layers, int enc, int in_dim, int K0_pad, int out_dim) {
    Layout L;
    L.xs = enc == TN_ENC_POSENC ? 0 : in_dim;
    L.rowsH = (n_layers - 1) * H;
    L.rowsE = enc == TN_ENC_NONE ? 0 : K0_pad - L.xs;
    // plain inputs of a stack that runs layer by layer (Cobafa: 36 features into 128 x 6, models.py:239-247): the training forward
    // stages x^T as 64 zero-padded rows (x_rows_kernel) so that the first layer and its weight gradient take the row-operand
    // kernels like every other layer; `xs` keeps its meaning for the generic kernels, which read x row-major
    if (plain_x_rows(H, n_layers, enc, K0_pad, out_dim)) L.rowsE = 64;
    const int outp = (out_dim + 31) & ~31;
    L.rowsG = H > outp ? H : outp;
    // wide stacks (layer kernels): ReLU bit masks of every hidden activation, one dword per lane and 32-feature block = 2 rows
    // per (activation, block), behind the two gradient buffers -- the data-gradient kernel reads ONE dword per lane where the
    // float mask rows cost it 16 row loads per tile (each vector-memory instruction stalls the matrix pipe for ~40 cycles)
    L.rowsM = H >= 128 ? 2 * (H / 32) * (n_layers - 1) : 0;
    L.total = L.rowsH + L.rowsE + 2 * L.rowsG + L.rowsM;
    return L;
}

__device__ __forceinline__ int col0(const MlpArgs &a, int q) { return layer0_col(a, q); }

// ------------------------------------------------------------------------------------------------
// forward with activation stash + output gradient
// ------------------------------------------------------------------------------------------------
// FWD_ONLY (training forward, tn_mlp_fwd_stash on a wide / deep stack): y is written, and buffer A receives the last
// layer's PRE-ACTIVATION instead of the output gradient; out_grad_kernel turns it into the gradient when the backward runs.
template <int H, int WPB, bool FWD_ONLY = false, bool FIRST_ONLY = false>
__global__ __launch_bounds__(WPB * 64) void fwd_stash_kernel(MlpArgs a, const float *__restrict__ x, const float *__restrict__ aux,
                                                             const float *__restrict__ gy, int64_t n, float *__restrict__ stash,
                                                             float *__restrict__ y = nullptr)
{
    constexpr int T = H / 32;
    const int lane = tn::lane_id(), j_ = lane & 31, h_ = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (n + 31) >> 5;
    const int L = a.n_layers, G0 = a.K0_pad >> 3, out = a.out_dim;
    const Layout lay = make_layout(H, L, a.enc, a.in_dim, a.K0_pad, out);
    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WPB) {
        int j = j_, h = h_;
        asm volatile("" : "+v"(j), "+v"(h));
        const int64_t row = tile * 32 + j;
        const bool valid = row < n;
        const float *xrow = x + (valid ? row : 0) * a.in_dim;
        float aux3[3] = {0.f, 0.f, 0.f};
        if (valid) {
            if (a.enc == TN_ENC_POSENC) { aux3[0] = xrow[0]; aux3[1] = xrow[1]; aux3[2] = xrow[2]; }
            else if (a.enc == TN_ENC_DIR_CAT) { aux3[0] = aux[3 * row]; aux3[1] = aux[3 * row + 1]; aux3[2] = aux[3 * row + 2]; }
        }
        float *st = stash + tile * (int64_t)lay.total * 32;
        float *stE = st + lay.rowsH * 32;
        float *stG = stE + lay.rowsE * 32;               // buffer A: receives the output gradient
        f32x16 act[T];
#pragma unroll
        for (int ob = 0; ob < T; ++ob) act[ob] = tn::bias_tile(a.B[0], ob, h);
#pragma clang loop unroll(disable)
        for (int g = 0; g < G0; ++g) {
            const f32x4 b = fetch_input(a, xrow, aux3, valid, g, h);
            f32x4 w[T];
#pragma unroll
            for (int ob = 0; ob < T; ++ob)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = 8 * g + 4 * h + u;
                    w[ob][u] = q < a.K0 ? a.W[0][(int64_t)(32 * ob + j) * a.K0 + col0(a, q)] : 0.0f;
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int ob = 0; ob < T; ++ob) act[ob] = tn::mfma32(w[ob][u], b[u], act[ob]);
            if (a.enc != TN_ENC_NONE && 8 * g + 4 * h + 3 >= lay.xs) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = 8 * g + 4 * h + u;
                    if (q >= lay.xs) stE[(q - lay.xs) * 32 + j] = b[u];
                }
            }
        }
#pragma unroll
        for (int ob = 0; ob < T; ++ob) {
            tn::pin16(act[ob]);
            act[ob] = tn::relu16(act[ob]);
            store_rows_lane(st, act[ob], ob, j, h);
        }
        if constexpr (FIRST_ONLY) {                // the remaining layers run as layer-kernel launches
            // ReLU bits of this activation where the layer kernels keep them (two rows per 32-feature block), so that the data
            // gradient of layer 1 can take its mask from 256 B instead of 32 activation rows
            unsigned *bits = reinterpret_cast<unsigned *>(st + (lay.rowsH + lay.rowsE + 2 * lay.rowsG) * 32);
#pragma unroll
            for (int ob = 0; ob < T; ++ob) bits[2 * ob * 32 + lane] = relu_bits(act[ob]);
            continue;
        }
        for (int l = 1; l + 1 < L; ++l) {
            tn::hidden_layer<H>(a.W[l], a.B[l], H, act, j, h);
#pragma unroll
            for (int ob = 0; ob < T; ++ob) store_rows_lane(st + l * H * 32, act[ob], ob, j, h);
        }
        // output layer -> g = gy * act'(pre) as rows [out feature][32 samples]
        const float *Wf = a.W[L - 1];
        const float *Bf = a.B[L - 1];
        if (out <= 4) {
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                float g = 0.0f;
                if (o < out) {
                    const float pre = tn::small_out<H>(Wf + o * H, Bf[o], act, h);
                    if constexpr (FWD_ONLY) {
                        g = valid ? pre : 0.0f;
                        if (valid && h == 0) y[row * out + o] = tn::apply_act(pre, a.out_act);
                    } else g = valid ? gy[row * out + o] * act_grad(pre, a.out_act) : 0.0f;
                }
                if (h == 0) stG[o * 32 + j] = g;
            }
            // rows 4..31 of the first tile are read as zeros by the consumers (they clamp to `out`)
        } else {
            const int n_ob = (out + 31) >> 5;
            for (int ob = 0; ob < n_ob; ++ob) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) { const int f = 32 * ob + frow(r, h); acc[r] = f < out ? Bf[f] : 0.f; }
                const int arow = 32 * ob + j;
#pragma unroll
                for (int kb = 0; kb < T; ++kb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4 w = {0.f, 0.f, 0.f, 0.f};
                        if (arow < out) w = *reinterpret_cast<const f32x4 *>(Wf + (int64_t)arow * H + 32 * kb + 8 * q + 4 * h);
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc = tn::mfma32(w[u], act[kb][4 * q + u], acc);
                    }
                tn::pin16(acc);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * ob + frow(r, h);
                    if constexpr (FWD_ONLY) {
                        stG[f * 32 + j] = (valid && f < out) ? acc[r] : 0.0f;
                        if (valid && f < out) y[row * out + f] = tn::apply_act(acc[r], a.out_act);
                    } else stG[f * 32 + j] = (valid && f < out) ? gy[row * out + f] * act_grad(acc[r], a.out_act) : 0.0f;
                }
            }
        }
    }
}

// buffer A: pre-activation rows (written by the FWD_ONLY forward) -> output gradient  g = gy * act'(pre)
__global__ __launch_bounds__(256) void out_grad_kernel(const float *__restrict__ gy, int64_t n, int out, int out_act, int rows_total,
                                                       int64_t off_g, float *__restrict__ stash)
{
    // [32 samples][out] block of gy -> [out][32 samples] rows through LDS: both sides of the transposition are coalesced
    // (16-byte loads along a sample's row when `out` allows it, no integer division in the index arithmetic)
    constexpr int TS = 260;                                 // row stride (floats): 16-byte aligned, 4 (mod 64) banks apart
    __shared__ __attribute__((aligned(16))) float t[32 * TS];
    const int64_t n_tiles = (n + 31) >> 5;
    const int j = threadIdx.x & 31, sub = threadIdx.x >> 5;                 // 8 row slots per block
    const bool vec = (out & 3) == 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        float *g = stash + (tile * (int64_t)rows_total + off_g) * 32;
        const int64_t r0 = tile * 32;
        for (int c0 = 0; c0 < out; c0 += 256) {                   // 256 output columns per pass through the LDS tile
            const int cw = min(out - c0, 256);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int r = sub + 8 * rr;
                const bool rok = r0 + r < n;
                const float *src = gy + (r0 + (rok ? r : 0)) * out + c0;
                for (int c = 4 * j; c < cw; c += 128) {
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (vec) { if (rok) v = *reinterpret_cast<const f32x4 *>(src + c); }
                    else {
#pragma unroll
                        for (int u = 0; u < 4; ++u) if (rok && c + u < cw) v[u] = src[c + u];
                    }
                    *reinterpret_cast<f32x4 *>(t + r * TS + c) = v;
                }
            }
            __syncthreads();
            for (int f = sub; f < cw; f += 8) {
                float v = t[j * TS + f];
                if (out_act != TN_ACT_NONE) v *= act_grad(g[(c0 + f) * 32 + j], out_act);       // buffer A holds the pre-activation
                g[(c0 + f) * 32 + j] = v;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// data gradient of one layer:  Gout = relu'(Hmask) * (W^T Gin)      (FIRST: grad_x, no mask, row-major out)
// ------------------------------------------------------------------------------------------------

template <int H, bool FIRST, int WPB>
__global__ __launch_bounds__(WPB * 64) void dgrad_layer_kernel(DgradArgs a, int64_t n, float *__restrict__ stash, float *__restrict__ gx)
{
    constexpr int T = H / 32;
    const int lane = tn::lane_id(), j_ = lane & 31, h_ = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (n + 31) >> 5;
    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WPB) {
        int j = j_, h = h_;
        asm volatile("" : "+v"(j), "+v"(h));
        float *st = stash + tile * (int64_t)a.rows_total * 32;
        // an output layer wider than H (N > 32 T, e.g. the 3 x 96 basis of KPlanesExplicitColorDecoder on a 128-wide stack) is
        // consumed in chunks of H rows; the chunks' contributions to the input gradient add up
        for (int n0 = 0; n0 < a.N; n0 += H) {
        const float *gin = st + (a.off_gin + n0) * 32;
        const int Nc = min(a.N - n0, H);
        const int TN = (Nc + 31) >> 5, ng = (Nc + 7) >> 3;
        f32x16 G[T];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nn = 32 * t + frow(r, h);
                G[t][r] = (t < TN && nn < Nc) ? gin[nn * 32 + j] : 0.0f;
            }
        const int n_kt = FIRST ? (a.in_dim + 31) >> 5 : T;
#pragma clang loop unroll(disable)
        for (int kt = 0; kt < n_kt; ++kt) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            const int k = 32 * kt + j;
            int kc = k;
            bool kok = true;
            if (FIRST) {
                kok = k < a.in_dim;
                kc = a.enc == TN_ENC_DIR_CAT ? 6 * a.n_freqs + 3 + k : k;
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (4 * t + q < ng) {
                        float w[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int nn = 32 * t + 8 * q + 4 * h + u;
                            w[u] = (nn < Nc && kok) ? a.W[(int64_t)(n0 + nn) * a.K + kc] : 0.0f;
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc = tn::mfma32(w[u], G[t][4 * q + u], acc);
                    }
                }
            }
            tn::pin16(acc);
            if (FIRST) {
                const int64_t row = tile * 32 + j;
                if (row < n) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int f = 32 * kt + frow(r, h);
                        if (f < a.in_dim) gx[row * a.in_dim + f] = (a.accum_gx || n0 > 0) ? gx[row * a.in_dim + f] + acc[r] : acc[r];
                    }
                }
            } else {
                const float *hm = st + a.off_mask * 32;
                float *gout = st + a.off_gout * 32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * kt + frow(r, h);
                    const float v = hm[f * 32 + j] > 0.0f ? acc[r] : 0.0f;
                    gout[f * 32 + j] = n0 > 0 ? gout[f * 32 + j] + v : v;
                }
            }
        }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// data gradient of a wide hidden layer (H = 128 / 256, K == H) with the weights in LDS.
// The generic kernel above reads W from L2 once per MFMA group (5.5 ms per 256x256 layer and 2^20 samples where the
// MFMAs need 0.9).  Here a workgroup stages the 32*NKT columns of W it is responsible for (all of them for H = 128, one
// half for H = 256: 133 KB) once, TRANSPOSED, and every wave walks its 32-sample tiles with the input gradient in registers
// and one conflict-free ds_read_b128 per four MFMAs.  blockIdx.y selects the column group.
// ------------------------------------------------------------------------------------------------
template <int H, int NKT, int WPB>
__global__ __launch_bounds__(WPB * 64) void dgrad_lds_kernel(DgradArgs a, int64_t n, float *__restrict__ stash)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int T = H / 32;
    constexpr int SW = H + 4;                             // LDS row stride (floats): W^T, one row per input feature k
    const int kt0 = blockIdx.y * NKT;
    for (int e = threadIdx.x; e < H * 32 * NKT; e += blockDim.x) {      // coalesced read of W, transposed into LDS (once)
        const int nn = e / (32 * NKT), c = e - nn * (32 * NKT);
        lds[c * SW + nn] = nn < a.N ? a.W[(int64_t)nn * a.K + 32 * kt0 + c] : 0.0f;
    }
    __syncthreads();
    const int lane = tn::lane_id(), j_ = lane & 31, h_ = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (n + 31) >> 5;
    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WPB) {
        int j = j_, h = h_;
        asm volatile("" : "+v"(j), "+v"(h));
        float *st = stash + tile * (int64_t)a.rows_total * 32;
        const float *gin = st + a.off_gin * 32;
        const float *hm = st + a.off_mask * 32;
        float *gout = st + a.off_gout * 32;
        f32x16 G[T];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nn = 32 * t + frow(r, h);
                const float v = gin[(nn < a.N ? nn : a.N - 1) * 32 + j];     // unconditional load, zeroed afterwards
                G[t][r] = nn < a.N ? v : 0.0f;
            }
#pragma clang loop unroll(disable)
        for (int ktl = 0; ktl < NKT; ++ktl) {
            const int kt = kt0 + ktl;
            float m[16];                                   // ReLU mask source of this output block: requested before the MFMAs
#pragma unroll
            for (int r = 0; r < 16; ++r) m[r] = hm[(32 * kt + frow(r, h)) * 32 + j];
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            const float *wl = lds + (32 * ktl + j) * SW + 4 * h;
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 w = *reinterpret_cast<const f32x4 *>(wl + 32 * t + 8 * q);     // W[n .. n+3][k]: one ds_read_b128
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = tn::mfma32(w[u], G[t][4 * q + u], acc);
                }
            }
            tn::pin16(acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) gout[(32 * kt + frow(r, h)) * 32 + j] = m[r] > 0.0f ? acc[r] : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// training forward of the FIRST layer of a wide stack (positional-encoding inputs, K0_pad <= 64) with the weights in LDS:
// a workgroup stages all H weight rows (zero-padded to 64 columns) once, every wave walks its tiles with the encoded
// inputs (workspace rows written by enc_rows_kernel, already in B-operand layout) in registers and one ds_read_b128 per
// four MFMAs.  The hidden and output layers run as fwd_wreg_kernel launches (below).
// ------------------------------------------------------------------------------------------------
// positional-encoding inputs of a tile as workspace rows [slot][32 samples] (the E rows of the layout)
// (slots: rows written -- K0_pad for the encodings, 64 for plain inputs: slots past the input width are zero rows)
__global__ __launch_bounds__(256) void enc_rows_kernel(MlpArgs a, const float *__restrict__ x, int64_t n, float *__restrict__ stash,
                                                       int rows_total, int64_t off_e, int slots)
{
    const int lane = tn::lane_id(), j = lane & 31, h = lane >> 5;
    const int64_t n_tiles = (n + 31) >> 5;
    const int G0 = slots >> 3;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t row = tile * 32 + j;
        const bool valid = row < n;
        const float *xrow = x + (valid ? row : 0) * a.in_dim;
        float aux3[3] = {0.f, 0.f, 0.f};
        if (a.enc == TN_ENC_POSENC) { aux3[0] = xrow[0]; aux3[1] = xrow[1]; aux3[2] = xrow[2]; }
        float *stE = stash + (tile * (int64_t)rows_total + off_e) * 32 + j;
        for (int g = 0; g < G0; ++g) {
            const f32x4 b = fetch_input(a, xrow, aux3, valid, g, h);
#pragma unroll
            for (int u = 0; u < 4; ++u) stE[(8 * g + 4 * h + u) * 32] = b[u];
        }
    }
}


// T = 32-row blocks of the layer input: 2 for the positional-encoding first layer, whose encoded inputs (<= 64 slots)
// enc_rows_kernel has written as workspace rows (the rows the weight gradient reads anyway)
template <int H, int T, int NOT, int WPB>
__global__ __launch_bounds__(WPB * 64) void fwd_lds_kernel(FwdLayerArgs a, int64_t n, float *__restrict__ stash, float *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SW = 32 * T + 4;                         // LDS row stride (floats): b128 reads of 16 rows hit 64 banks
    const int ot0 = blockIdx.y * NOT;
    if (a.K == 32 * T) {
        for (int e = threadIdx.x; e < 32 * NOT * (8 * T); e += blockDim.x) {
            const int o = e / (8 * T), c = (e - o * (8 * T)) * 4;
            const int nn = 32 * ot0 + o;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (nn < a.N) v = *reinterpret_cast<const f32x4 *>(a.W + (int64_t)nn * a.K + c);
            *reinterpret_cast<f32x4 *>(lds + o * SW + c) = v;
        }
    } else {                                               // ragged K (first layer): zero padded
        for (int e = threadIdx.x; e < 32 * NOT * 32 * T; e += blockDim.x) {
            const int o = e / (32 * T), c = e - o * (32 * T);
            const int nn = 32 * ot0 + o;
            lds[o * SW + c] = (nn < a.N && c < a.K) ? a.W[(int64_t)nn * a.K + c] : 0.0f;
        }
    }
    __syncthreads();
    const int lane = tn::lane_id(), j_ = lane & 31, h_ = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (n + 31) >> 5;
    const int n_ot = min(NOT, ((a.N + 31) >> 5) - ot0);
    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WPB) {
        int j = j_, h = h_;
        asm volatile("" : "+v"(j), "+v"(h));
        float *st = stash + tile * (int64_t)a.rows_total * 32;
        const float *in = st + a.off_in * 32;
        float *outp = st + a.off_out * 32;
        f32x16 A[T];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = 32 * t + frow(r, h);
                if constexpr (32 * T == H) A[t][r] = in[k * 32 + j];          // hidden layer: K == H rows, immediate offsets
                else {
                    const float v = in[(k < a.Kp ? k : 0) * 32 + j];
                    A[t][r] = k < a.Kp ? v : 0.0f;                            // rows past Kp belong to another buffer
                }
            }
#pragma clang loop unroll(disable)
        for (int otl = 0; otl < n_ot; ++otl) {
            const int ot = ot0 + otl;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) { const int f = 32 * ot + frow(r, h); acc[r] = a.B[f < a.N ? f : 0]; }
            const float *wl = lds + (32 * otl + j) * SW + 4 * h;
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 w = *reinterpret_cast<const f32x4 *>(wl + 32 * t + 8 * q);
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = tn::mfma32(w[u], A[t][4 * q + u], acc);
                }
            }
            tn::pin16(acc);
            acc = tn::relu16(acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) outp[(32 * ot + frow(r, h)) * 32 + j] = acc[r];
            if (a.off_bits >= 0) reinterpret_cast<unsigned *>(st + (a.off_bits + 2 * ot) * 32)[lane] = relu_bits(acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Hidden layers of the wide stacks (N == K == H = 128 / 256), weights in REGISTERS, activations through LDS.
//
// The LDS-weight form (dgrad_lds_kernel above; its forward twin was removed) keeps half a layer's weights in LDS and a
// tile's 128 input values per lane in registers: every wave reads its own tile from HBM (two column groups -> every input
// row twice), pays ~3 VALU instructions of address arithmetic per row load, and stalls on a full memory latency per tile
// whenever its SIMD partner does too (measured: matrix pipes 71-77 % busy; this form 78-88 %).  Here the roles are swapped: wave `ob` of a workgroup owns output block `ob` of the
// layer and holds W[32 ob .. 32 ob + 31][0 .. H) as A operands in 4 H / 32 registers for the whole launch; the H / 32 waves
// of a tile stream share each 32-sample input tile through LDS, [sample][feature] with a 4-float pad, so that the B operand
// of four consecutive MFMAs is one conflict-free ds_read_b128.  A wave brings in 32 of the tile's H rows (16 row loads per
// lane with immediate offsets, 4 ds_write_b128).  Three LDS tile buffers and ONE barrier per tile, placed in the middle of
// the tile's MFMAs: tile it+1 is written at the top of iteration it (requested a whole iteration earlier), read from the top
// of iteration it+1, and its buffer is reused for tile it+4 only after the barrier of iteration it+2 -- no wave ever waits
// at the barrier unless it is half a tile ahead of the slowest one.  Same MFMA steps in the same order as the LDS-weight
// kernels: bit-identical results.  What is left of the idle time is the vector-memory instructions themselves (ablation in
// scripts/microbench/wreg_layer.hip: no loads and no stores -> 97.6 % busy; staggering the two waves of a SIMD, spreading
// the instructions between the MFMAs, LDS-direct loads with ds_read_b32 operands and wide accesses through LDS transposes
// were all measured and are not faster).
// ------------------------------------------------------------------------------------------------
template <int H> struct WregGeom {
    static constexpr int T = H / 32;               // 32-row blocks of the layer's input and of its output
    static constexpr int STREAMS = 8 / T;          // tile streams per 8-wave workgroup
    static constexpr int SW = H + 4;               // LDS tile row stride (floats)
    static constexpr int TILE = 32 * SW;           // floats per tile buffer
    static constexpr size_t lds_bytes = (size_t)STREAMS * 3 * TILE * sizeof(float);
};

// MFMAs of reduction groups [G0, G1) (group g = 8 in-features: B operand = one ds_read_b128 at bt + 8 g) with the operands of
// the next PAIR of groups requested before the current pair's eight MFMAs are issued (left alone, hipcc sinks each read to
// just in front of its first use: read -> wait -> MFMAs -> read ...; both waves of a SIMD then wait at the same time)
template <int G0, int G1, int T>
__device__ __forceinline__ void wreg_mfma_run(f32x16 &acc, const f32x4 (&W)[T][4], const float *__restrict__ bt, f32x4 (&b)[2]) {
#pragma unroll
    for (int g = G0; g < G1; g += 2) {
        f32x4 nb[2];
        if (g + 2 < G1) {
            nb[0] = *reinterpret_cast<const f32x4 *>(bt + 8 * (g + 2));
            nb[1] = *reinterpret_cast<const f32x4 *>(bt + 8 * (g + 3));
        }
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = tn::mfma32(W[(g + e) >> 2][(g + e) & 3][u], b[e][u], acc);
        __builtin_amdgcn_sched_barrier(0);
        if (g + 2 < G1) { b[0] = nb[0]; b[1] = nb[1]; }
    }
}
__device__ __forceinline__ void wreg_first_pair(const float *__restrict__ bt, int g, f32x4 (&b)[2]) {
    b[0] = *reinterpret_cast<const f32x4 *>(bt + 8 * g);
    b[1] = *reinterpret_cast<const f32x4 *>(bt + 8 * (g + 1));
}

template <int H, bool LAST>
__global__ __launch_bounds__(512) void fwd_wreg_kernel(FwdLayerArgs a, int64_t n, float *__restrict__ stash, float *__restrict__ y)
{
    using G = WregGeom<H>;
    constexpr int T = G::T, SW = G::SW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    TileWalk<G::STREAMS, T> tw;
    tw.init(n);
    const int lane = tw.lane, j = tw.j, h = tw.h, ob = tw.wib;
    float *buf = lds + tw.stream * 3 * G::TILE;
    const int64_t iters = tw.iters;
    if (iters == 0) return;
    // A operands: W[32 ob + j][32 t + 8 q + 4 h .. + 3]
    f32x4 W[T][4];
    {
        const int nn = 32 * ob + j;
        const float *wrow = a.W + (int64_t)(nn < a.N ? nn : 0) * a.K + 4 * h;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(wrow + 32 * t + 8 * q);
                W[t][q] = nn < a.N ? w : f32x4{0.f, 0.f, 0.f, 0.f};
            }
    }
    f32x16 bias;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const int f = 32 * ob + frow(r, h); bias[r] = a.B[f < a.N ? f : 0]; }
    float stage[16];
    wreg_load_rows(urow(stash, tw.tile_of(0) * a.rows_total + a.off_in), ob, j, h, stage);
    wreg_write_rows(buf, SW, ob, j, h, stage);
    wreg_load_rows(urow(stash, tw.tile_of(1) * a.rows_total + a.off_in), ob, j, h, stage);
    __syncthreads();
    // results of a tile: [feature][32 samples] rows (+ y for the last layer).  A stream past the end recomputes the last tile
    // (same inputs -> same values) rather than branching around its stores.
    auto emit = [&](int64_t tile, f32x16 acc) {
        if (!LAST || 32 * ob < a.N) {
            if constexpr (!LAST) {
                wreg_store_block(urow(stash, tile * a.rows_total + a.off_out), ob, j, h, acc);
                if (a.off_bits >= 0) {                  // (wave-uniform) ReLU bits of this block for the data-gradient kernel
                    unsigned *bits = reinterpret_cast<unsigned *>(urow(stash, tile * a.rows_total + a.off_bits + 2 * ob));
                    bits[lane] = relu_bits(acc);
                }
            } else emit_last_narrow(a, n, stash, y, tile, ob, j, h, acc);
        }
    };
    int cur = 0;
    f32x16 res;
#pragma unroll
    for (int r = 0; r < 16; ++r) res[r] = 0.0f;
#pragma clang loop unroll(disable)
    for (int64_t it = 0; it < iters; ++it) {
        const int nxt = cur == 2 ? 0 : cur + 1;
        wreg_write_rows(buf + nxt * G::TILE, SW, ob, j, h, stage);              // tile it+1 (requested a whole iteration ago)
        // VMEM queue order: the PREVIOUS tile's stores, then the requests for tile it+2 -- the s_waitcnt vmcnt in front of the
        // next iteration's ds_write then waits for exactly these loads (stores issued after them would have to drain first:
        // vmcnt counts loads and stores in one in-order queue on gfx9)
        if (it > 0) emit(tw.tile_of(it - 1), res);
        wreg_load_rows(urow(stash, tw.tile_of(it + 2) * a.rows_total + a.off_in), ob, j, h, stage);
        __builtin_amdgcn_sched_barrier(0);
        const float *bt = buf + cur * G::TILE + j * SW + 4 * h;
        f32x16 acc = bias;
        f32x4 b[2];
        wreg_first_pair(bt, 0, b);
        wreg_mfma_run<0, 2 * T, T>(acc, W, bt, b);
        __syncthreads();
        wreg_first_pair(bt, 2 * T, b);
        wreg_mfma_run<2 * T, 4 * T, T>(acc, W, bt, b);
        tn::pin16(acc);
        if constexpr (!LAST) res = tn::relu16(acc); else res = acc;
        cur = nxt;
    }
    emit(tw.tile_of(iters - 1), res);
}

// data gradient twin: wave `kb` owns input-feature block kb and holds W[0 .. H)[32 kb .. 32 kb + 31] (W^T rows) in registers
template <int H>
__global__ __launch_bounds__(512) void dgrad_wreg_kernel(DgradArgs a, int64_t n, float *__restrict__ stash)
{
    using G = WregGeom<H>;
    constexpr int T = G::T, SW = G::SW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    TileWalk<G::STREAMS, T> tw;
    tw.init(n);
    const int lane = tw.lane, j = tw.j, h = tw.h, kb = tw.wib;
    float *buf = lds + tw.stream * 3 * G::TILE;
    const int64_t iters = tw.iters;
    if (iters == 0) return;
    // A operands: W[32 t + 8 q + 4 h + u][32 kb + j]   (N == K == H)
    f32x4 W[T][4];
    {
        const float *wcol = a.W + (int64_t)(4 * h) * a.K + 32 * kb + j;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int u = 0; u < 4; ++u) W[t][q][u] = wcol[(int64_t)(32 * t + 8 * q + u) * a.K];
    }
    float stage[16];
    wreg_load_rows(urow(stash, tw.tile_of(0) * a.rows_total + a.off_gin), kb, j, h, stage);
    wreg_write_rows(buf, SW, kb, j, h, stage);
    wreg_load_rows(urow(stash, tw.tile_of(1) * a.rows_total + a.off_gin), kb, j, h, stage);
    __syncthreads();
    auto emit = [&](int64_t tile, const f32x16 &g) {
        wreg_store_block(urow(stash, tile * a.rows_total + a.off_gout), kb, j, h, g);
    };
    int cur = 0;
    f32x16 res;
#pragma unroll
    for (int r = 0; r < 16; ++r) res[r] = 0.0f;
#pragma clang loop unroll(disable)
    for (int64_t it = 0; it < iters; ++it) {
        const int nxt = cur == 2 ? 0 : cur + 1;
        wreg_write_rows(buf + nxt * G::TILE, SW, kb, j, h, stage);
        // VMEM queue order (see fwd_wreg_kernel): previous tile's stores, this tile's ReLU-mask rows, requests for tile it+2
        if (it > 0) emit(tw.tile_of(it - 1), res);
        const int64_t tile = tw.tile_of(it);
        float m[16];
        unsigned mbits = 0;
        if (a.off_bits >= 0) mbits = reinterpret_cast<const unsigned *>(urow(stash, tile * a.rows_total + a.off_bits + 2 * kb))[lane];
        else wreg_load_block(urow(stash, tile * a.rows_total + a.off_mask), kb, j, h, m);
        wreg_load_rows(urow(stash, tw.tile_of(it + 2) * a.rows_total + a.off_gin), kb, j, h, stage);
        __builtin_amdgcn_sched_barrier(0);
        const float *bt = buf + cur * G::TILE + j * SW + 4 * h;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        f32x4 b[2];
        wreg_first_pair(bt, 0, b);
        wreg_mfma_run<0, 2 * T, T>(acc, W, bt, b);
        __syncthreads();
        wreg_first_pair(bt, 2 * T, b);
        wreg_mfma_run<2 * T, 4 * T, T>(acc, W, bt, b);
        tn::pin16(acc);
        if (a.off_bits >= 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r] = mask_keep(acc[r], mbits, r);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r] = m[r] > 0.0f ? acc[r] : 0.0f;
        }
        cur = nxt;
    }
    emit(tw.tile_of(iters - 1), res);
}

template <int H, bool LAST>
int launch_fwd_wreg(const FwdLayerArgs &f, int64_t n, float *stash, float *y, hipStream_t s)
{
    using G = WregGeom<H>;
    return launch(fwd_wreg_kernel<H, LAST>, 8, G::lds_bytes, stream_blocks(n, G::STREAMS), s, "mlp_fwd: fwd_wreg_kernel", f, n, stash, y);
}

template <int H>
int launch_dgrad_wreg(const DgradArgs &d, int64_t n, float *stash, hipStream_t s)
{
    using G = WregGeom<H>;
    return launch(dgrad_wreg_kernel<H>, 8, G::lds_bytes, stream_blocks(n, G::STREAMS), s, "mlp_bwd: dgrad_wreg_kernel", d, n, stash);
}

// ------------------------------------------------------------------------------------------------
// weight gradient of one layer: dW[N][K] += G[N][s] A[K][s]^T over all samples; db[N] += sum_s G
// ------------------------------------------------------------------------------------------------

template <int MAXS>
__global__ __launch_bounds__(512) void wgrad_layer_kernel(WgradArgs a, const float *__restrict__ x, int64_t n,
                                                          const float *__restrict__ stash)
{
    const int lane = tn::lane_id(), i = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (n + 31) >> 5;
    const int Tn = (a.N + 31) >> 5, Tk = (a.K_pad + 31) >> 5;
    const int total = Tn * Tk;
    f32x16 acc[MAXS];
    float dbacc[MAXS];
    int ttn[MAXS], ttk[MAXS];
#pragma unroll
    for (int m = 0; m < MAXS; ++m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;
        dbacc[m] = 0.0f;
        const int id = wave + 8 * m;
        ttn[m] = id < total ? id / Tk : -1;
        ttk[m] = id < total ? id - (id / Tk) * Tk : 0;
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const float *st = stash + tile * (int64_t)a.rows_total * 32;
#pragma unroll
        for (int m = 0; m < MAXS; ++m) {
            if (ttn[m] < 0) continue;
            const int nrow = 32 * ttn[m] + i;
            f32x4 gv[4], av[4];
            {
                const f32x4 *p = reinterpret_cast<const f32x4 *>(st + (a.off_g + (nrow < a.N ? nrow : 0)) * 32 + 16 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) { const f32x4 v = p[e]; gv[e] = nrow < a.N ? v : f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
            const int q0 = 32 * ttk[m], q = q0 + i;
            if (a.first) {
#pragma unroll
                for (int e = 0; e < 4; ++e) av[e] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (q0 < a.xs) {
                    const int qx = q < a.xs ? q : 0;
                    const int64_t r0 = tile * 32 + 16 * h;
                    float xv[16];
#pragma unroll
                    for (int t = 0; t < 16; ++t) { const int64_t rc = r0 + t < n ? r0 + t : n - 1; xv[t] = x[rc * a.in_dim + qx]; }
#pragma unroll
                    for (int t = 0; t < 16; ++t) av[t >> 2][t & 3] = (q < a.xs && r0 + t < n) ? xv[t] : 0.0f;
                }
                if (a.enc != TN_ENC_NONE && q0 + 31 >= a.xs) {
                    const bool ise = q >= a.xs && q < a.K_pad;
                    const f32x4 *p = reinterpret_cast<const f32x4 *>(st + (a.off_e + (ise ? q - a.xs : 0)) * 32 + 16 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const f32x4 v = p[e]; if (ise) av[e] = v; }
                }
            } else {
                const f32x4 *p = reinterpret_cast<const f32x4 *>(st + (a.off_a + (q < a.K ? q : 0)) * 32 + 16 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) { const f32x4 v = p[e]; av[e] = q < a.K ? v : f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m] = tn::mfma32(gv[e][u], av[e][u], acc[m]);
            if (ttk[m] == 0) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) s += (gv[e][0] + gv[e][1]) + (gv[e][2] + gv[e][3]);
                dbacc[m] += s;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MAXS; ++m) {
        if (ttn[m] < 0) continue;
        tn::pin16(acc[m]);
        const int k = 32 * ttk[m] + i;
        const bool kok = k < a.K;
        int kc = k;
        if (a.first && a.enc == TN_ENC_DIR_CAT) { const int pe = 6 * a.n_freqs + 3; kc = k < a.in_dim ? pe + k : k - a.in_dim; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int nn = 32 * ttn[m] + frow(r, h);
            if (kok && nn < a.N) atomicAdd(&a.gW[(int64_t)nn * a.K + kc], acc[m][r]);
        }
        if (ttk[m] == 0) {
            float s = dbacc[m];
            s += __shfl_xor(s, 32, 64);
            const int nn = 32 * ttn[m] + i;
            if (h == 0 && nn < a.N) atomicAdd(&a.gB[nn], s);
        }
    }
}

// Hidden layers of the wide stacks (N == K == H = 128 / 256: H/32 x H/32 output tiles of 32 x 32): a wave owns a BN x BK block
// of tiles (2 x 4 for H = 256: 128 accumulator registers), so a 32-sample tile costs it BN + BK operand blocks for
// 16 BN BK MFMAs.  The workgroup brings a tile's 2 H rows (G_l and H_{l-1}, [feature][32 samples]) in ONCE, LDS-direct
// (global_load_lds_dwordx4: no staging registers, no ds_write; H / 32 instructions per wave and tile), double-buffered with
// one barrier per tile, and the operands are ds_read_b128.  (Each wave requesting its own operand blocks from L2 -- 24
// 16-byte loads per lane and tile, every block fetched by 2-4 waves -- ran the matrix pipes at 74 %: a vector-memory
// instruction costs its SIMD ~40-90 pipe cycles, scripts/microbench/wreg_layer.hip; this form: 84 %.)  The LDS image of an
// LDS-direct load is lane-linear (no row padding possible), so the 16-byte chunks of a row are XOR-swizzled through the
// SOURCE address: slot p of row r holds chunk p ^ ((r >> 1) & 7), which spreads the 16 rows of a ds_read_b128 phase over
// all 64 banks.
// (LDS-direct loads: glds16, mlp_stage.h.)
template <int H, int BN, int BK>
__global__ __launch_bounds__(512) void wgrad_lds_kernel(WgradArgs a, int64_t n, const float *__restrict__ stash)
{
    constexpr int TILE = 2 * H * 32;                      // floats per buffer: G rows [0, H), A rows [H, 2H)
    constexpr int NI = H / 32;                            // LDS-direct loads per wave and tile (8 rows each)
    constexpr int WK = (H / 32) / BK;                     // waves along k
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = tn::lane_id(), i = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (n + 31) >> 5;
    const int tn0 = (wave / WK) * BN, tk0 = (wave % WK) * BK;
    f32x16 acc[BN][BK];
    float dbacc[BN];
#pragma unroll
    for (int bn = 0; bn < BN; ++bn) {
        dbacc[bn] = 0.0f;
#pragma unroll
        for (int bk = 0; bk < BK; ++bk)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bn][bk][r] = 0.0f;
    }
    // this lane's part of a tile fetch: rows 8 (wave NI + e) + (lane >> 3), chunk slot lane & 7
    int src_off[NI];
#pragma unroll
    for (int e = 0; e < NI; ++e) {
        const int row = 8 * (wave * NI + e) + (lane >> 3);
        src_off[e] = (row < H ? row : row - H) * 32 + 4 * ((lane & 7) ^ ((row >> 1) & 7));       // relative to the G rows / the A rows of the tile
    }
    auto fetch = [&](int64_t tile, float *buf) {
        const float *stg = urow(stash, tile * a.rows_total + a.off_g), *sta = urow(stash, tile * a.rows_total + a.off_a);
#pragma unroll
        for (int e = 0; e < NI; ++e)
            glds16((8 * (wave * NI + e) < H ? stg : sta) + src_off[e], buf + 256 * (wave * NI + e));      // (wave-uniform choice: 8 rows per request)
    };
    // operand chunk e (samples 16 h + 4 e .. + 3) of row r: slot (4 h + e) ^ ((r >> 1) & 7)
    int g_off[BN], a_off[BK];
#pragma unroll
    for (int bn = 0; bn < BN; ++bn) g_off[bn] = (32 * (tn0 + bn) + i) * 32;
#pragma unroll
    for (int bk = 0; bk < BK; ++bk) a_off[bk] = (H + 32 * (tk0 + bk) + i) * 32;
    const int swz = (i >> 1) & 7;                          // rows 32 b + i: (r >> 1) & 7 == (i >> 1) & 7
    if ((int64_t)blockIdx.x < n_tiles) fetch(blockIdx.x, lds);
    __syncthreads();
    int cur = 0;
#pragma clang loop unroll(disable)
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const float *buf = lds + cur * TILE;
        if (tile + gridDim.x < n_tiles) fetch(tile + gridDim.x, lds + (cur ^ 1) * TILE);
        f32x4 gv[BN][4];
#pragma unroll
        for (int bn = 0; bn < BN; ++bn)
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[bn][e] = *reinterpret_cast<const f32x4 *>(buf + g_off[bn] + 4 * ((4 * h + e) ^ swz));
        if (tk0 == 0) {
#pragma unroll
            for (int bn = 0; bn < BN; ++bn) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) s += (gv[bn][e][0] + gv[bn][e][1]) + (gv[bn][e][2] + gv[bn][e][3]);
                dbacc[bn] += s;
            }
        }
        // (measured and not kept: the barrier in front of the LAST k block's MFMAs, whose operands are in registers by then, so
        // that an early wave still has MFMAs to issue behind it -- 1.043 ms per layer against 1.015 with the barrier at the end)
#pragma unroll
        for (int bk = 0; bk < BK; ++bk) {
            f32x4 av[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) av[e] = *reinterpret_cast<const f32x4 *>(buf + a_off[bk] + 4 * ((4 * h + e) ^ swz));
#pragma unroll
            for (int bn = 0; bn < BN; ++bn)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[bn][bk] = tn::mfma32(gv[bn][e][u], av[e][u], acc[bn][bk]);
        }
        __syncthreads();                                   // (drains this wave's LDS-direct loads: the next tile is in place)
        cur ^= 1;
    }
    flush_tiles<true>(a, tn0, tk0, i, h, acc, 1.0f);
    if (tk0 == 0) {
#pragma unroll
        for (int bn = 0; bn < BN; ++bn) {
            float s = dbacc[bn];
            s += __shfl_xor(s, 32, 64);
            if (h == 0) atomicAdd(&a.gB[32 * (tn0 + bn) + i], s);
        }
    }
}

template <int H, int BN, int BK>
int launch_wgrad_lds(const WgradArgs &w, int64_t n, const float *stash, hipStream_t s)
{
    constexpr size_t lds_bytes = (size_t)2 * 2 * H * 32 * sizeof(float);
    return launch(wgrad_lds_kernel<H, BN, BK>, 8, lds_bytes, grid_blocks(n, 1, 256), s, "mlp_bwd: wgrad_lds_kernel", w, n, stash);
}

// ------------------------------------------------------------------------------------------------
// d loss / d x of the FIRST layer of a wide stack on narrow plain inputs (in_dim <= 64: Cobafa's 36 gathered features,
// reference models.py:239-247, whose gradient goes on into the grid scatter):  gx[s][k] (+)= sum_n W_0[n][k] G_0[n][s].
// The layer-kernel form of fwd_lds_kernel with the roles swapped: W_0^T ([64 slots][H], zero padded) is staged in LDS once
// per workgroup, a wave holds its tile's H gradient rows as B operands (16 H / 32 registers) and produces the <= 2 blocks of 32
// input slots with one ds_read_b128 per four MFMAs; results leave as 16-byte stores into the row-major gx the grid kernels
// read.  Replaces dgrad_layer_kernel<H, true, 4> (every weight operand a scalar global load, 256 VGPRs + 188 AGPRs, one wave
// per SIMD: 0.55 ms per 2^20 samples at H = 128).
// ------------------------------------------------------------------------------------------------
template <int H, int WPB>
__global__ __launch_bounds__(WPB * 64) void dgrad_first_kernel(DgradArgs a, int64_t n, const float *__restrict__ stash, float *__restrict__ gx)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int T = H / 32, SW = H + 4;
    for (int e = threadIdx.x; e < 64 * H; e += blockDim.x) {          // lds[slot k][hidden n] = W_0[n][k]
        const int k = e / H, nn = e - k * H;
        lds[k * SW + nn] = k < a.K ? a.W[(int64_t)nn * a.K + k] : 0.0f;
    }
    __syncthreads();
    const int lane = tn::lane_id(), j_ = lane & 31, h_ = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_tiles = (n + 31) >> 5;
    const int n_kt = (a.in_dim + 31) >> 5;
    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WPB) {
        int j = j_, h = h_;
        asm volatile("" : "+v"(j), "+v"(h));
        const float *gin = urow(stash, tile * (int64_t)a.rows_total + a.off_gin);
        f32x16 G[T];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) G[t][r] = gin[(32 * t + frow(r, h)) * 32 + j];
        const int64_t row = tile * 32 + j;
#pragma clang loop unroll(disable)
        for (int kt = 0; kt < n_kt; ++kt) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            const float *wl = lds + (32 * kt + j) * SW + 4 * h;
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 w = *reinterpret_cast<const f32x4 *>(wl + 32 * t + 8 * q);
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = tn::mfma32(w[u], G[t][4 * q + u], acc);
                }
            tn::pin16(acc);
            if (row < n) {
                float *gr = gx + row * a.in_dim + 32 * kt + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int f0 = 32 * kt + 8 * q + 4 * h;
                    if (f0 + 3 < a.in_dim && (a.in_dim & 3) == 0) {
                        f32x4 v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                        if (a.accum_gx) v += *reinterpret_cast<const f32x4 *>(gr + 8 * q);
                        *reinterpret_cast<f32x4 *>(gr + 8 * q) = v;
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (f0 + u < a.in_dim) gr[8 * q + u] = a.accum_gx ? gr[8 * q + u] + acc[4 * q + u] : acc[4 * q + u];
                    }
                }
            }
        }
    }
}

template <int H>
int launch_dgrad_first(const DgradArgs &d, int64_t n, const float *stash, float *gx, hipStream_t s)
{
    constexpr int WPB = 8;
    constexpr size_t lds_bytes = (size_t)64 * (H + 4) * sizeof(float);
    return launch(dgrad_first_kernel<H, WPB>, WPB, lds_bytes, grid_per_cu(n, WPB, lds_bytes), s, "mlp_bwd: dgrad_first_kernel", d, n, stash, gx);
}

template <int H, int T, int NOT>
int launch_fwd_lds(const FwdLayerArgs &f, int64_t n, float *stash, float *y, hipStream_t s)
{
    constexpr int WL = 8;
    constexpr size_t lds_bytes = (size_t)32 * NOT * (32 * T + 4) * 4;
    const int groups = (((f.N + 31) / 32) + NOT - 1) / NOT;                  // blockIdx.y: NOT output blocks each
    const int per_cu = lds_bytes * 2 <= (size_t)LDS_LIMIT_BYTES ? 2 : 1;
    return launch(fwd_lds_kernel<H, T, NOT, WL>, WL, lds_bytes, dim3((unsigned)grid_blocks(n, WL, (256 * per_cu) / groups), (unsigned)groups), s,
                  "mlp_fwd: fwd_lds_kernel", f, n, stash, y);
}

// ------------------------------------------------------------------------------------------------
// host side: the plan of one pass over a wide / deep stack
// ------------------------------------------------------------------------------------------------
// make_plan takes every decision of a pass once: the workspace layout and size, the forward's form, where the backward's
// d loss / d y comes from, and each layer's weight- and data-gradient kernel with its row offsets and tail slots.  run_fwd and
// run_bwd turn the plan into launches, one launch per step, in order.  Each eligibility rule is one predicate here.

// the layer-kernel path: the first layer, then one launch per layer, [feature][32-sample] rows between them
__host__ inline bool layer_kernel_path(int H, const MlpArgs &a) { return H >= 128 && a.n_layers >= 3 && a.out_dim > 4 && a.out_dim <= H; }
// ... whose first layer reads its (encoded) inputs as workspace rows: positional encoding with <= 64 slots, or <= 64 plain inputs
// (plain_x_rows); these stacks train on the slab layout
__host__ inline bool input_rows(int H, const MlpArgs &a) {
    return layer_kernel_path(H, a) && (a.enc == TN_ENC_POSENC || a.enc == TN_ENC_NONE) && a.K0_pad <= 64;
}
// ... and can run the cross-layer f16x2 launches of mlp_fused_f2.hip: the data-gradient chain (all its layers H x H) and, without an
// output activation, the forward in one launch.  Only these workspaces hold the chain's gradient slabs and the packed weight stream.
__host__ inline bool cross_layer(int H, const MlpArgs &a) { return input_rows(H, a) && a.f2 && !a.layerwise && a.out_dim == H; }
__host__ inline bool fused_fwd(int H, const MlpArgs &a) { return cross_layer(H, a) && a.out_act == TN_ACT_NONE; }
// TN_MLP_SKIP_LAST: the training forward stops at the last hidden activation (its consumers took the last layer over)
__host__ inline bool skip_last_ok(int H, const MlpArgs &a) { return input_rows(H, a) && a.f2 && a.out_dim == H; }

// `inference`: no backward follows, so the hidden activations need not survive: two ping-pong buffers of H rows each (plus the
// encoded-input rows) instead of one buffer per layer -- (2 H + rowsE) * 128 B per 32 samples (2.3 KB per sample for the
// Vanilla stack against 11.5 KB of training workspace).
__host__ inline int infer_rows_total(int H, const Layout &lay) { return 2 * H + lay.rowsE; }
__host__ inline int64_t infer_ws_rows_bytes(int H, const Layout &lay, int64_t n_tiles) {       // (256-byte multiple: the packed stream of the fused form follows)
    return ((n_tiles * (int64_t)std::max(infer_rows_total(H, lay), 64) * 32 * (int64_t)sizeof(float)) + 255) & ~(int64_t)255;
}

// Where the row sets of a training workspace live; every kernel addresses  row = tile * rows_total + off.
//   * tile-major (make_layout; what the general-shape kernels compute for themselves): a tile holds all its row sets back to back,
//     rows_total = lay.total, off = the set's offset inside the tile.
//   * slab (round 5; the layer-kernel path whose first layer takes row operands, i.e. every launch gets its offsets as arguments):
//     every row set is contiguous over the tiles -- slab s = rows [s n_tiles H, (s + 1) n_tiles H), tile t of it at t H -- so
//     rows_total = H and off = s n_tiles H (+ the set's place inside a shared slab: the E rows and the bit rows are packed together).
//     A launch then streams two or three dense arrays instead of 32 KB pieces 300 - 400 KB apart: the same copy of 1 KB + 1 KB per
//     sample runs at 5.5 TB/s (6.0 with nt hints) instead of 4.98 (scripts/microbench/row_copy.hip) -- the layer kernels sat AT
//     that 4.98.
struct RowMap {
    bool slab;
    int rows_total, H, L;
    int64_t sl;                                  // rows per slab
    Layout lay;
    int64_t e_off, m_off[TN_MLP_MAX_LAYERS];
    int64_t gc_off;                              // slab layout: first of the L - 1 slabs of the fused data-gradient chain (round 6)
    int n_slabs;
    int64_t offH(int l) const { return slab ? l * sl : (int64_t)l * H; }                 // activation l (output of layer l), l < L - 1
    int64_t offE() const { return slab ? e_off : lay.rowsH; }
    int64_t offGA() const { return slab ? (L - 1) * sl : lay.rowsH + lay.rowsE; }
    int64_t offGB() const { return slab ? L * sl : lay.rowsH + lay.rowsE + lay.rowsG; }
    int64_t offM(int l) const { return slab ? m_off[l] : lay.rowsH + lay.rowsE + 2 * lay.rowsG + 2 * (H / 32) * l; }   // bit rows of activation l
    int64_t offGC(int l) const { return gc_off + l * sl; }      // slab layout: d loss / d (pre-activation of hidden layer l), kept for its weight gradient
    int64_t total_rows(int64_t n_tiles) const { return slab ? n_slabs * sl : n_tiles * lay.total; }
};
// `chain`: + the L - 1 slabs of the cross-layer data-gradient chain, behind every other slab
__host__ inline RowMap make_rowmap(int H, const MlpArgs &a, int64_t n_tiles, bool slab, bool chain) {
    RowMap m;
    const int L = a.n_layers;
    m.lay = make_layout(H, L, a.enc, a.in_dim, a.K0_pad, a.out_dim);
    m.slab = slab; m.H = H; m.L = L; m.sl = n_tiles * H;
    m.rows_total = slab ? H : m.lay.total;
    m.e_off = 0; m.n_slabs = 0; m.gc_off = 0;
    for (int l = 0; l < TN_MLP_MAX_LAYERS; ++l) m.m_off[l] = 0;
    if (slab) {
        int64_t sidx = L + 1;                      // slabs 0 .. L - 2: activations, L - 1 / L: buffers A / B
        int within = 0;
        m.e_off = sidx * m.sl; within = m.lay.rowsE;
        const int mr = 2 * (H / 32);
        for (int l = 0; l + 1 < L; ++l) {
            if (within + mr > H) { ++sidx; within = 0; }
            m.m_off[l] = sidx * m.sl + within;
            within += mr;
        }
        m.n_slabs = (int)sidx + 1;
        // the cross-layer data-gradient chain (mlp_fused_f2.hip) writes every layer's gradient once and the weight-gradient launches read
        // them afterwards: one slab per hidden layer instead of the two ping-pong buffers
        m.gc_off = (int64_t)m.n_slabs * m.sl;
        if (chain) m.n_slabs += L - 1;
    }
    return m;
}

// The training workspace: rows, the tail (WS_TAIL_BYTES), and for cross_layer stacks the packed weight stream.  tn_mlp_fwd_stash and
// tn_mlp_bwd of one step must agree on it -- the f16x2 weight gradient reads the maxima the forward left in the tail -- so it depends
// on the shape, the encoding, the arithmetic and TN_MLP_LAYERWISE only.
struct Workspace {
    RowMap rm;              // what a stashing forward leaves: slab layout for input_rows stacks, else tile-major
    int64_t rows;           // rows in front of the tail: room for either layout (an unstashed backward runs tile-major)
    int64_t pack_off;       // byte offset of the packed weight stream (cross_layer)
    int64_t bytes;
};
__host__ inline Workspace workspace(int H, const MlpArgs &a, int64_t n_tiles) {
    Workspace w;
    w.rm = make_rowmap(H, a, n_tiles, input_rows(H, a), cross_layer(H, a));
    w.rows = std::max<int64_t>(n_tiles * w.rm.lay.total, w.rm.total_rows(n_tiles));
    w.pack_off = fused_pack_offset(w.rows);
    w.bytes = cross_layer(H, a) ? w.pack_off + fused_pack_bytes(H, a.n_layers) : w.rows * 32 * (int64_t)sizeof(float) + WS_TAIL_BYTES;
    return w;
}

enum class Pass { INFER_FWD, TRAIN_FWD, BWD };
enum class Fwd { GENERAL, LAYERS, FUSED };          // general-shape kernel / one launch per layer / one persistent launch (mlp_fused_f2.hip)
enum class First { ENC_F2, ENC_LDS, STASH };        // Fwd::LAYERS' first layer: enc_rows_kernel + fwd_first_f2 / fwd_lds, or fwd_stash_kernel
enum class GradY { ROWS, OUT_GRAD, RECOMPUTE };     // d loss / d y: rows from the consumer (TN_MLP_GRAD_Y_ROWS), from the stash, or a forward
enum class Wgrad { F2, B3, LDS, ROWS, TILES2, TILES8 };
enum class Dgrad { NONE, F2, B3, WREG, LDS, GENERAL, FIRST, FIRST_GENERAL };
// (the general-shape kinds -- First::STASH, Fwd::GENERAL, Wgrad::TILES8, Dgrad::GENERAL / FIRST_GENERAL -- say so once on a width-128 /
//  256 stack: tn::warn_once ids 0 - 4)

struct LayerStep {          // backward of layer l: its kinds and their arguments (run_bwd adds the gradient and tail pointers)
    Wgrad wgrad;
    Dgrad dgrad;            // Dgrad::F2 launches before the weight gradient: it reports the largest |gradient| that one scales by
    WgradArgs w;
    DgradArgs d;
    int max_a, max_g;       // f16x2 tail slots of the largest |input| / |gradient| of the layer, -1: none
};

struct Plan {
    Pass pass;
    Workspace ws;
    RowMap rm;              // the rows this pass addresses
    // forward
    Fwd fwd;
    First first;
    int rows_total, first_kp, n_run;    // rows per tile; input rows of the first layer; layers evaluated (TN_MLP_SKIP_LAST: L - 1)
    int64_t off_e, off_out[TN_MLP_MAX_LAYERS], off_bits[TN_MLP_MAX_LAYERS];     // layer l reads off_out[l - 1]
    int64_t pack_off;       // Fwd::FUSED: byte offset of the packed weight stream
    bool tail;              // f16x2 training forward: clears the tail and reports the layers' input maxima to it
    bool no_y;              // the f16x2 forms leave y as workspace rows only (TN_MLP_ROWS_ONLY, TN_MLP_SKIP_LAST)
    // backward
    GradY grad_y;
    bool chain;             // the data gradients of layers top .. 1 in one launch (mlp_fused_f2.hip)
    int top;                // highest layer the backward walks (TN_MLP_SKIP_LAST: L - 2)
    LayerStep step[TN_MLP_MAX_LAYERS];
};

int make_plan(const MlpArgs &a, int H, int64_t n, Pass pass, Plan &p, bool stashed = false, bool gy_rows = false, bool want_gx = false)
{
    const int L = a.n_layers, out = a.out_dim;
    const int64_t n_tiles = (n + 31) / 32;
    const bool train = pass != Pass::INFER_FWD;
    p.pass = pass;
    p.ws = workspace(H, a, n_tiles);
    // (the slab layout is what the stashing forward of the same configuration left behind)
    p.rm = pass == Pass::TRAIN_FWD || stashed ? p.ws.rm : make_rowmap(H, a, n_tiles, false, false);
    const RowMap &rm = p.rm;
    if (pass != Pass::BWD) {
        TN_REQUIRE(!a.skip_last || (train && skip_last_ok(H, a)), TN_E_CONFIG,
                   "tn_mlp_fwd_stash: TN_MLP_SKIP_LAST needs the f16x2 training forward of a slab-layout stack whose output is as wide as its hidden layers");
        TN_REQUIRE(train || input_rows(H, a), TN_E_CONFIG, "tn_mlp_fwd_ws: configuration without a layer-by-layer inference forward");
        p.fwd = !layer_kernel_path(H, a) ? Fwd::GENERAL : fused_fwd(H, a) && (!train || rm.lay.rowsE == 64) ? Fwd::FUSED : Fwd::LAYERS;
        p.first = !input_rows(H, a) ? First::STASH : a.f2 ? First::ENC_F2 : First::ENC_LDS;
        p.first_kp = a.enc == TN_ENC_NONE ? 64 : a.K0_pad;
        p.n_run = L - (a.skip_last ? 1 : 0);
        p.tail = train && a.f2 && p.fwd != Fwd::GENERAL;
        p.no_y = train && a.f2 && out == H && a.out_act == TN_ACT_NONE && (a.rows_only || a.skip_last);
        p.pack_off = train ? p.ws.pack_off : infer_ws_rows_bytes(H, rm.lay, n_tiles);
        if (train) {
            p.rows_total = rm.rows_total; p.off_e = rm.offE();
        } else if (p.fwd == Fwd::FUSED) {        // 64 encoded-input rows per tile, contiguous over the tiles
            p.rows_total = 64; p.off_e = 0;
        } else {
            p.rows_total = infer_rows_total(H, rm.lay); p.off_e = 2 * H;
        }
        for (int l = 0; l < TN_MLP_MAX_LAYERS; ++l) {
            p.off_out[l] = !train ? (l & 1) * H : l + 1 < L ? rm.offH(l) : rm.offGA();
            p.off_bits[l] = train && l + 1 < L ? rm.offM(l) : -1;
        }
        return TN_OK;
    }
    if (a.skip_last) TN_REQUIRE(gy_rows && stashed && skip_last_ok(H, a), TN_E_CONFIG, "tn_mlp_bwd: TN_MLP_SKIP_LAST needs TN_MLP_STASHED | TN_MLP_GRAD_Y_ROWS on the f16x2 slab-layout stack");
    // TN_MLP_GRAD_Y_ROWS: the consumers of y (the heads' data-gradient chains) have written d loss / d y as rows into buffer B
    // (tn_mlp_rows_view): nothing to transpose, the walk starts from B and ping-pongs into A
    if (gy_rows) TN_REQUIRE(stashed && a.out_act == TN_ACT_NONE && (out & 31) == 0, TN_E_CONFIG,
                            "tn_mlp_bwd: TN_MLP_GRAD_Y_ROWS needs TN_MLP_STASHED, no output activation and out_dim % 32 == 0");
    p.grad_y = gy_rows ? GradY::ROWS : stashed ? GradY::OUT_GRAD : GradY::RECOMPUTE;
    p.chain = stashed && cross_layer(H, a);
    p.top = L - 1 - (a.skip_last ? 1 : 0);
    // ReLU bit rows exist for every activation the training forward of the layer-kernel path wrote
    const bool bits = stashed && layer_kernel_path(H, a);
    int64_t cur = gy_rows ? rm.offGB() : rm.offGA(), nxt = gy_rows ? rm.offGA() : rm.offGB();
    for (int l = p.top; l >= 0; --l) {
        LayerStep &st = p.step[l];
        WgradArgs &w = st.w;
        DgradArgs &d = st.d;
        w.N = d.N = a.N[l]; w.K = d.K = a.K[l]; w.K_pad = l == 0 ? a.K0_pad : a.K[l]; w.rows_total = d.rows_total = rm.rows_total;
        w.off_g = d.off_gin = p.chain && l < p.top ? rm.offGC(l) : cur;         // d loss / d (pre-activation of layer l)
        w.off_a = d.off_mask = l > 0 ? rm.offH(l - 1) : 0;                       // the layer's input activation
        w.off_e = rm.offE(); d.off_gout = nxt; d.off_bits = bits && l > 0 ? rm.offM(l - 1) : -1;
        w.first = l == 0; w.enc = d.enc = a.enc; w.in_dim = d.in_dim = a.in_dim; w.n_freqs = d.n_freqs = a.n_freqs; w.xs = rm.lay.xs;
        d.W = a.W[l]; d.accum_gx = a.accum_gx;
        const bool square = H >= 128 && l > 0 && a.N[l] == H;        // (K = H for every l > 0)
        // f16x2: the layer's data gradient first -- it reports the largest |gradient| of the rows both kernels read -- then the weight
        // gradient with that scale and the one the forward pass left for the layer's input rows
        const bool f2 = square && a.f2 && bits;
        st.max_a = f2 ? l : -1;
        st.max_g = f2 ? 16 + l : -1;
        if (f2) st.wgrad = Wgrad::F2;
        else if (square) st.wgrad = a.b3 ? Wgrad::B3 : Wgrad::LDS;
        // first layer on input rows: plain inputs the training forward staged as 64 rows (Cobafa's 36 features), or positional-encoding
        // slots of a width-256 stack (<= 64, all of them E rows of the workspace) -- the row-operand kernel of mlp_wgrad_rows.hip
        else if (l == 0 && H >= 128 && ((stashed && plain_x_rows(H, L, a.enc, a.K0_pad, out)) || (H == 256 && a.enc == TN_ENC_POSENC && a.K0_pad == 64)))
            st.wgrad = Wgrad::ROWS;
        else {
            const int tiles = ((a.N[l] + 31) / 32) * (((l == 0 ? a.K0_pad : a.K[l]) + 31) / 32);
            if (tiles > 64) return tn::fail(TN_E_CONFIG, "mlp_bwd: layer too large for the wgrad tiling");
            st.wgrad = tiles <= 16 ? Wgrad::TILES2 : Wgrad::TILES8;
        }
        if (l > 0) {
            if (f2) st.dgrad = p.chain ? Dgrad::NONE : Dgrad::F2;          // (chain: its launch writes the rows and the maximum)
            else if (square) st.dgrad = a.b3 && bits ? Dgrad::B3 : Dgrad::WREG;
            else if (H >= 128 && a.N[l] <= H) st.dgrad = Dgrad::LDS;      // weights of this layer's column group in LDS
            else st.dgrad = Dgrad::GENERAL;
            std::swap(cur, nxt);
        } else if (want_gx && a.enc != TN_ENC_POSENC) {                     // d loss / d x of a narrow plain input: W_0^T in LDS
            st.dgrad = H >= 128 && a.enc == TN_ENC_NONE && a.in_dim <= 64 ? Dgrad::FIRST : Dgrad::FIRST_GENERAL;
        } else {
            st.dgrad = Dgrad::NONE;
        }
    }
    return TN_OK;
}

template <int H>
int run_fwd(const Plan &p, const MlpArgs &a, const float *x, const float *aux, int64_t n, float *y, float *stash, hipStream_t s)
{
    const int64_t n_tiles = (n + 31) / 32;
    constexpr int WPB = H <= 64 ? 8 : 4;
    if (p.fwd == Fwd::GENERAL) {
        if (H >= 128) tn::warn_once(1, "mlp forward: this width-%d stack (%d layers, %d outputs) is outside the layer-by-layer kernels and runs on "
                                       "the general-shape kernel", H, a.n_layers, a.out_dim);
        fwd_stash_kernel<H, WPB, true><<<dim3((unsigned)std::min<int64_t>((n_tiles + WPB - 1) / WPB, 256 * 2)), dim3(WPB * 64), 0, s>>>(
            a, x, aux, nullptr, n, stash, y);
        return tn::check_launch("fwd_stash_kernel(forward)");
    }
    if constexpr (H >= 128) {
        float *tail = p.tail ? ws_tail(stash, p.ws.rows) : nullptr;
        if (tail) {
            hipError_t me = hipMemsetAsync(tail, 0, WS_TAIL_BYTES, s);
            if (me != hipSuccess) { tn::set_error("mlp_fwd(f16x2): cannot clear the workspace tail: %s", hipGetErrorString(me)); return (int)me; }
        }
        if (p.fwd == Fwd::FUSED || p.first != First::STASH) {          // (encoded) inputs as rows
            enc_rows_kernel<<<dim3((unsigned)std::min<int64_t>((n_tiles + 3) / 4, 256 * 8)), dim3(256), 0, s>>>(a, x, n, stash, p.rows_total, p.off_e,
                                                                                                              p.first_kp);
            if (int rc = tn::check_launch("enc_rows_kernel")) return rc;
        }
        if (p.fwd == Fwd::FUSED) {
            // round 6: the whole stack as ONE persistent launch (mlp_fused_f2.hip); in training, activations stay in registers across the
            // layers and reach the workspace as the rows, bit rows and maxima the layer-wise backward reads -- written once, never read back
            void *pack = reinterpret_cast<unsigned char *>(stash) + p.pack_off;
            float *y_f = p.no_y ? nullptr : y;
            if (p.pass == Pass::INFER_FWD) {
                if (p.first_kp < 64) {               // rows K0_pad .. 63 of every tile are operands too (zero weights, but 0 x NaN = NaN)
                    hipError_t me = hipMemset2DAsync(stash + (size_t)p.first_kp * 32, (size_t)p.rows_total * 128, 0, (size_t)(64 - p.first_kp) * 128,
                                                     (size_t)n_tiles, s);
                    if (me != hipSuccess) { tn::set_error("mlp_fwd(fused): cannot clear the padding rows: %s", hipGetErrorString(me)); return (int)me; }
                }
                return launch_fused_fwd_f2(H, a, n, stash, y_f, pack, s);
            }
            FusedStash sp;
            sp.rows = stash; sp.rows_total = p.rows_total; sp.off_e = p.off_e; sp.n_run = p.n_run; sp.tail = tail;
            for (int l = 0; l < TN_MLP_MAX_LAYERS; ++l) { sp.off_out[l] = 0; sp.off_bits[l] = 0; }
            for (int l = 0; l < p.n_run; ++l) { sp.off_out[l] = p.off_out[l]; sp.off_bits[l] = std::max<int64_t>(p.off_bits[l], 0); }
            return launch_fused_fwd_f2(H, a, n, stash, y_f, pack, s, &sp);
        }
        if (p.first == First::STASH) {
            tn::warn_once(0, "mlp forward: the first layer of this width-%d stack (encoding %d, %d inputs) runs on the general-shape kernel "
                          "(fast forms: positional encoding with <= 64 slots, or <= 64 plain inputs)", H, a.enc, a.in_dim);
            fwd_stash_kernel<H, WPB, true, true><<<dim3((unsigned)std::min<int64_t>((n_tiles + WPB - 1) / WPB, 256 * 4)), dim3(WPB * 64), 0, s>>>(
                a, x, aux, nullptr, n, stash, y);
            if (int rc = tn::check_launch("fwd_stash_kernel(first layer)")) return rc;
        } else {
            FwdLayerArgs f;
            f.W = a.W[0]; f.B = a.B[0]; f.N = a.N[0]; f.K = a.K0; f.Kp = p.first_kp; f.rows_total = p.rows_total;
            f.off_in = p.off_e; f.off_out = p.off_out[0]; f.out_act = a.out_act; f.off_bits = p.off_bits[0];
            if (p.first == First::ENC_F2) { if (int rc = launch_fwd_first_f2(H, f, n, stash, s)) return rc; }
            else if (int rc = launch_fwd_lds<H, 2, H / 32>(f, n, stash, y, s)) return rc;
        }
        for (int l = 1; l < p.n_run; ++l) {
            FwdLayerArgs f;
            f.W = a.W[l]; f.B = a.B[l]; f.N = a.N[l]; f.K = a.K[l]; f.Kp = a.K[l]; f.rows_total = p.rows_total;
            f.off_in = p.off_out[l - 1]; f.off_out = p.off_out[l]; f.out_act = a.out_act; f.off_bits = p.off_bits[l];
            f.max_in = tail ? tail + l : nullptr;
            // hidden layers (K == N == H) and the output layer (K == H, N <= H): weights in registers
            const bool last = l + 1 == a.n_layers;
            int rc;
            if (a.f2) rc = launch_fwd_f2(H, last, f, n, stash, last && p.no_y ? nullptr : y, s);     // fp16 matrix cores, two-term splits, scaled
            else if (a.b3) rc = launch_fwd_b3(H, last, f, n, stash, y, s);                          // bf16 matrix cores, exact 3-way splits
            else rc = last ? launch_fwd_wreg<H, true>(f, n, stash, y, s) : launch_fwd_wreg<H, false>(f, n, stash, y, s);
            if (rc) return rc;
        }
    }
    return TN_OK;
}

template <int H>
int run_bwd(const Plan &p, const MlpArgs &a, const float *x, const float *aux, const float *gy, int64_t n, float *const *gw,
            float *const *gb, float *gx, float *stash, hipStream_t s)
{
    const RowMap &rm = p.rm;
    const int64_t n_tiles = (n + 31) / 32;
    constexpr int WPB = H <= 64 ? 8 : 4;
    float *tail = ws_tail(stash, p.ws.rows);
    if (p.grad_y == GradY::OUT_GRAD) {        // activations and the last pre-activation are in the workspace already (tn_mlp_fwd_stash)
        out_grad_kernel<<<dim3((unsigned)std::min<int64_t>(n_tiles, 256 * 8)), dim3(256), 0, s>>>(gy, n, a.out_dim, a.out_act, rm.rows_total,
                                                                                         rm.offGA(), stash);
        if (int rc = tn::check_launch("out_grad_kernel")) return rc;
    } else if (p.grad_y == GradY::RECOMPUTE) {
        fwd_stash_kernel<H, WPB><<<dim3((unsigned)std::min<int64_t>((n_tiles + WPB - 1) / WPB, 256 * 2)), dim3(WPB * 64), 0, s>>>(a, x, aux, gy, n, stash);
        if (int rc = tn::check_launch("fwd_stash_kernel")) return rc;
    }
    if (p.chain) {
        // round 6: every data gradient of the stack in ONE persistent launch (mlp_fused_f2.hip fused_chain_kernel): the gradients stay in
        // registers between the layers and reach the workspace once, as the rows the weight-gradient launches below read
        FusedChain fc;
        fc.rows = stash; fc.rows_total = rm.rows_total; fc.off_in = p.step[p.top].w.off_g; fc.tail = tail;
        for (int i = 0; i < TN_MLP_MAX_LAYERS; ++i) { fc.off_out[i] = 0; fc.off_bits[i] = 0; fc.tail_idx[i] = -1; }
        for (int i = 0; i < p.top; ++i) {
            const LayerStep &st = p.step[p.top - i];
            fc.off_out[i] = p.step[p.top - i - 1].w.off_g; fc.off_bits[i] = st.d.off_bits; fc.tail_idx[i] = st.max_g;
        }
        if (int rc = launch_fused_chain_f2(H, a, p.top, n, reinterpret_cast<unsigned char *>(stash) + p.ws.pack_off, s, &fc)) return rc;
    }
    for (int l = p.top; l >= 0; --l) {
        const LayerStep &st = p.step[l];
        WgradArgs w = st.w;
        w.gW = gw[l]; w.gB = gb[l];
        if (st.max_g >= 0) { w.g_max = tail + st.max_g; w.a_max = tail + st.max_a; }
        DgradArgs d = st.d;
        if (st.dgrad == Dgrad::F2) {
            d.max_in = tail + st.max_g;
            if (int rc = launch_dgrad_f2(H, d, n, stash, s)) return rc;
        }
        const int64_t wblocks = std::min<int64_t>(n_tiles, 256 * 2);
        int rc = TN_OK;
        switch (st.wgrad) {           // (the kinds that instantiate a kernel per width only occur for H >= 128)
        case Wgrad::F2: rc = launch_wgrad_f2(H, w, n, stash, s); break;
        case Wgrad::B3: rc = launch_wgrad_b3(H, w, n, stash, s); break;
        case Wgrad::LDS: if constexpr (H >= 128) rc = launch_wgrad_lds<H, 2, H == 256 ? 4 : 1>(w, n, stash, s); break;
        case Wgrad::ROWS:
            rc = tn_mlp_wgrad_rows(stash + w.off_g * 32, (int64_t)rm.rows_total * 32, H, stash + rm.offE() * 32, (int64_t)rm.rows_total * 32, 64,
                                   w.gW, w.K, 0, w.K, w.gB, n, s);
            break;
        case Wgrad::TILES2:
            wgrad_layer_kernel<2><<<dim3((unsigned)wblocks), dim3(512), 0, s>>>(w, x, n, stash);
            rc = tn::check_launch("wgrad_layer_kernel");
            break;
        case Wgrad::TILES8:
            if (H >= 128) tn::warn_once(2, "mlp backward: weight gradient of a %d x %d layer on the general-shape kernel (8 tiles per wave, spills)", w.N, w.K);
            wgrad_layer_kernel<8><<<dim3((unsigned)wblocks), dim3(512), 0, s>>>(w, x, n, stash);
            rc = tn::check_launch("wgrad_layer_kernel");
            break;
        }
        if (rc) return rc;
        const int64_t blocks = std::min<int64_t>((n_tiles + WPB - 1) / WPB, 256 * 4);
        switch (st.dgrad) {
        case Dgrad::NONE: case Dgrad::F2: break;
        case Dgrad::B3: rc = launch_dgrad_b3(H, d, n, stash, s); break;
        case Dgrad::WREG: if constexpr (H >= 128) rc = launch_dgrad_wreg<H>(d, n, stash, s); break;
        case Dgrad::LDS:
            if constexpr (H >= 128) {
                constexpr int NKT = 4, WL = 8;
                constexpr size_t lds_bytes = (size_t)32 * NKT * (H + 4) * 4;
                const int groups = (H / 32) / NKT;
                const int per_cu = lds_bytes * 2 <= (size_t)LDS_LIMIT_BYTES ? 2 : 1;
                rc = launch(dgrad_lds_kernel<H, NKT, WL>, WL, lds_bytes, dim3((unsigned)grid_blocks(n, WL, (256 * per_cu) / groups), (unsigned)groups), s,
                            "mlp_bwd: dgrad_lds_kernel", d, n, stash);
            }
            break;
        case Dgrad::GENERAL:
            if (H >= 128) tn::warn_once(3, "mlp backward: data gradient of a %d x %d layer of a width-%d stack on the general-shape kernel", d.N, d.K, H);
            dgrad_layer_kernel<H, false, WPB><<<dim3((unsigned)blocks), dim3(WPB * 64), 0, s>>>(d, n, stash, nullptr);
            rc = tn::check_launch("dgrad_layer_kernel");
            break;
        case Dgrad::FIRST: if constexpr (H >= 128) rc = launch_dgrad_first<H>(d, n, stash, gx, s); break;
        case Dgrad::FIRST_GENERAL:
            if (H >= 128) tn::warn_once(4, "mlp backward: d loss / d x of a width-%d stack with %d inputs (encoding %d) on the general-shape kernel", H, a.in_dim, a.enc);
            dgrad_layer_kernel<H, true, WPB><<<dim3((unsigned)blocks), dim3(WPB * 64), 0, s>>>(d, n, stash, gx);
            rc = tn::check_launch("dgrad_layer_kernel(first)");
            break;
        }
        if (rc) return rc;
    }
    return TN_OK;
}

}  // namespace

// internal entry points used by the dispatcher in mlp_bwd2.hip
extern "C" __attribute__((visibility("hidden"))) int64_t tn_mlp_bwd_layers_workspace_bytes(const tn_mlp_desc *desc, int64_t n)
{
    if (!desc || n <= 0) return 0;
    MlpArgs a;
    int H = 0;
    if (plan(desc, a, H) != TN_OK) return 0;
    if (((a.out_dim + 31) / 32) * (H / 32) > 64) return 0;          // weight-gradient tiling of the output layer (make_plan)
    return workspace(H, a, (n + 31) / 32).bytes;
}

extern "C" __attribute__((visibility("hidden"))) int tn_mlp_bwd_layers(const tn_mlp_desc *desc, const float *x, const float *aux,
                                                                      const float *grad_y, int64_t n, float *const *grad_weights,
                                                                      float *const *grad_biases, float *grad_x, float *workspace,
                                                                      void *stream)
{
    MlpArgs a;
    int H = 0;
    if (int rc = plan(desc, a, H)) return rc;
    TN_REQUIRE(x && (grad_y || (desc->flags & TN_MLP_GRAD_Y_ROWS)) && grad_weights && grad_biases && workspace, TN_E_NULL,
               "tn_mlp_bwd(layers): null pointer");
    TN_REQUIRE(a.enc != TN_ENC_DIR_CAT || aux, TN_E_NULL, "tn_mlp_bwd(layers): dir_cat needs aux");
    for (int l = 0; l < a.n_layers; ++l)
        TN_REQUIRE(grad_weights[l] && grad_biases[l], TN_E_NULL, "tn_mlp_bwd(layers): null gradient pointer");
    Plan p;
    if (int rc = make_plan(a, H, n, Pass::BWD, p, (desc->flags & TN_MLP_STASHED) != 0, (desc->flags & TN_MLP_GRAD_Y_ROWS) != 0, grad_x != nullptr))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (H) {
    case 32: return run_bwd<32>(p, a, x, aux, grad_y, n, grad_weights, grad_biases, grad_x, workspace, s);
    case 64: return run_bwd<64>(p, a, x, aux, grad_y, n, grad_weights, grad_biases, grad_x, workspace, s);
    case 128: return run_bwd<128>(p, a, x, aux, grad_y, n, grad_weights, grad_biases, grad_x, workspace, s);
    default: return run_bwd<256>(p, a, x, aux, grad_y, n, grad_weights, grad_biases, grad_x, workspace, s);
    }
}

extern "C" int tn_mlp_rows_view(const tn_mlp_desc *desc, int64_t n, int64_t *y_rows, int64_t *grad_y_rows, int64_t *tile_stride)
{
    TN_REQUIRE(desc && y_rows && grad_y_rows && tile_stride, TN_E_NULL, "tn_mlp_rows_view: null pointer");
    TN_REQUIRE(n >= 0, TN_E_SIZE, "tn_mlp_rows_view: negative n");
    MlpArgs a;
    int H = 0;
    if (int rc = plan(desc, a, H)) return rc;
    // the configurations whose training forward runs layer by layer and leaves y^T behind (run_fwd), see tn_mlp_fwd_stash
    TN_REQUIRE(layer_kernel_path(H, a) && (a.out_dim & 31) == 0 && a.out_act == TN_ACT_NONE && a.enc != TN_ENC_AUX_CAT, TN_E_CONFIG,
               "tn_mlp_rows_view: only wide stacks evaluated layer by layer (width 128 / 256, >= 3 layers, out % 32 == 0, no output activation) keep row views");
    const RowMap rm = workspace(H, a, (n + 31) / 32).rm;
    *y_rows = rm.offGA() * 32;                 // buffer A: the last layer's (pre-)activation = y
    *grad_y_rows = rm.offGB() * 32;            // buffer B
    *tile_stride = (int64_t)rm.rows_total * 32;
    return TN_OK;
}

extern "C" int tn_mlp_rows_view_hidden(const tn_mlp_desc *desc, int64_t n, int64_t *h_rows, int64_t *grad_h_rows, int64_t *mask_rows,
                                       int64_t *tile_stride)
{
    TN_REQUIRE(desc && h_rows && grad_h_rows && mask_rows && tile_stride, TN_E_NULL, "tn_mlp_rows_view_hidden: null pointer");
    TN_REQUIRE(n >= 0, TN_E_SIZE, "tn_mlp_rows_view_hidden: negative n");
    MlpArgs a;
    int H = 0;
    if (int rc = plan(desc, a, H)) return rc;
    TN_REQUIRE(a.skip_last && skip_last_ok(H, a) && a.out_act == TN_ACT_NONE, TN_E_CONFIG,
               "tn_mlp_rows_view_hidden: TN_MLP_SKIP_LAST | TN_MLP_F16X2 on a slab-layout stack (width 128 / 256, output as wide, no output activation)");
    const int L = a.n_layers;
    const RowMap rm = workspace(H, a, (n + 31) / 32).rm;
    *h_rows = rm.offH(L - 2) * 32;
    *grad_h_rows = rm.offGB() * 32;
    *mask_rows = rm.offM(L - 2) * 32;
    *tile_stride = (int64_t)rm.rows_total * 32;
    return TN_OK;
}

// inference forward of a wide stack on positional-encoding inputs through the layer kernels (88 % of the fp32 matrix rate where the
// register-resident kernel with weights from L2 reaches 67-70 %): workspace = two ping-pong activation buffers + encoded inputs
extern "C" int64_t tn_mlp_fwd_workspace_bytes(const tn_mlp_desc *desc, int64_t n)
{
    if (!desc || n <= 0) return 0;
    MlpArgs a;
    int H = 0;
    if (plan(desc, a, H) != TN_OK || !input_rows(H, a)) return 0;      // positional-encoding inputs, or plain inputs staged as rows (Cobafa's 36 features)
    const Layout lay = make_layout(H, a.n_layers, a.enc, a.in_dim, a.K0_pad, a.out_dim);
    // the layer-wise form's ping-pong rows, then the packed weight stream of the cross-layer form (mlp_fused_f2.hip; 2.4 MB for Vanilla)
    return infer_ws_rows_bytes(H, lay, (n + 31) / 32) + fused_pack_bytes(H, a.n_layers);
}

extern "C" int tn_mlp_fwd_ws(const tn_mlp_desc *desc, const float *x, const float *aux, int64_t n, float *y, void *workspace,
                             int64_t workspace_bytes, void *stream)
{
    TN_REQUIRE(desc, TN_E_NULL, "tn_mlp_fwd_ws: null descriptor");
    if (n <= 0) return n == 0 ? TN_OK : tn::fail(TN_E_SIZE, "tn_mlp_fwd_ws: negative n");
    const int64_t need = tn_mlp_fwd_workspace_bytes(desc, n);
    TN_REQUIRE(need > 0, TN_E_CONFIG, "tn_mlp_fwd_ws: this configuration has no workspace form (tn_mlp_fwd_workspace_bytes == 0): use tn_mlp_fwd");
    TN_REQUIRE(x && y && workspace && workspace_bytes >= need, TN_E_NULL, "tn_mlp_fwd_ws: null pointer or workspace too small");
    TN_REQUIRE((((uintptr_t)workspace | (uintptr_t)y) & 15) == 0, TN_E_ALIGN, "tn_mlp_fwd_ws: workspace / y must be 16-byte aligned");
    MlpArgs a;
    int H = 0;
    if (int rc = plan(desc, a, H)) return rc;
    Plan p;
    if (int rc = make_plan(a, H, n, Pass::INFER_FWD, p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (H == 128) return run_fwd<128>(p, a, x, aux, n, y, (float *)workspace, s);
    return run_fwd<256>(p, a, x, aux, n, y, (float *)workspace, s);
}

// training forward of a stack the layer-by-layer form covers: y + activations + last pre-activation into the workspace
extern "C" __attribute__((visibility("hidden"))) int tn_mlp_fwd_stash_layers(const tn_mlp_desc *desc, const float *x, const float *aux,
                                                                            int64_t n, float *y, float *workspace, void *stream)
{
    MlpArgs a;
    int H = 0;
    if (int rc = plan(desc, a, H)) return rc;
    TN_REQUIRE(x && y && workspace, TN_E_NULL, "tn_mlp_fwd_stash(layers): null pointer");
    TN_REQUIRE(a.enc != TN_ENC_DIR_CAT || aux, TN_E_NULL, "tn_mlp_fwd_stash(layers): dir_cat needs aux");
    TN_REQUIRE(a.enc != TN_ENC_AUX_CAT, TN_E_CONFIG, "tn_mlp_fwd_stash(layers): aux_cat is only implemented for the two-pass form");
    Plan p;
    if (int rc = make_plan(a, H, n, Pass::TRAIN_FWD, p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (H) {
    case 32: return run_fwd<32>(p, a, x, aux, n, y, workspace, s);
    case 64: return run_fwd<64>(p, a, x, aux, n, y, workspace, s);
    case 128: return run_fwd<128>(p, a, x, aux, n, y, workspace, s);
    default: return run_fwd<256>(p, a, x, aux, n, y, workspace, s);
    }
}
