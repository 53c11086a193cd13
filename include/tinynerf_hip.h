/* tinynerf_hip.h -- C ABI of libtinynerf_hip.so, the MI355X (gfx950) implementation of the
 * tinynerf ray-marching hot path.
 *
 * This is the drop-in boundary.  In the reference the native boundary is a pybind11 module
 * JIT-built at import time (reference src/core.py:7) with exactly two entry points,
 *     compute_weights_fwd(sigmas, steps, info, threshold) -> weights      (src/cuda.cu:66-95)
 *     compute_weights_bwd(sigmas, steps, info, weights, grad) -> grad_sig (src/cuda.cu:97-132)
 * Everything else on the path is ATen calls made from src/core.py and src/models.py; this
 * library gives each of those call sites one entry point as well (the cited file:line is
 * what the function replaces).
 *
 * Conventions
 *  - plain C: raw device pointers + sizes, no torch types; `stream` is a hipStream_t passed as
 *    void* (NULL = the null stream).  All work is enqueued asynchronously on that stream.
 *  - every function returns 0 on success, a negative TN_E_* code for a rejected argument, or a
 *    positive hipError_t; tn_last_error_string() describes the last failure of the calling thread.
 *  - the caller owns every buffer.  The library never allocates, frees or retains a pointer and
 *    keeps no mutable global state, so calls are re-entrant (the autograd engine calls the
 *    backward entry points from its own thread, reference src/core.py:203-207).
 *  - all tensors are dense row-major fp32 unless stated; `info` is int32 [n_rays,2] = (start,count)
 *    per ray, the reference's packing_info (src/core.py:165-188); rays own disjoint ranges.
 */
#ifndef TINYNERF_HIP_H
#define TINYNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TN_ABI_VERSION 6

enum {
    TN_OK = 0,
    TN_E_NULL = -1,      /* a required pointer is NULL */
    TN_E_SIZE = -2,      /* negative / inconsistent / unsupported size */
    TN_E_CONFIG = -3,    /* unsupported enum or layer configuration */
    TN_E_ALIGN = -4      /* pointer not aligned as the entry point requires */
};

const char *tn_last_error_string(void);
/* Most recent performance warning of the process ("" if none): a VALID call that landed on a general-shape fallback kernel -- a wide
 * stack whose first layer / layer shapes are not those of the reference's configurations (src/run.py:131-150) runs several times
 * slower than they do.  Said once per fallback on stderr as well (TN_QUIET=1 silences that).  Never an error: the results are right. */
const char *tn_last_warning_string(void);
int tn_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * a17  NeRF volume-rendering weights            (reference src/cuda.cu:3-58, core.py:192-207)
 * fwd: per ray T=1; w_k = T*(1-exp(-sigma_k*step_k)); T *= exp(..) while T > threshold; every
 *      sample of the ray after termination gets 0 (the kernel writes the whole range, `weights`
 *      does not need to be zeroed).  bwd: cuda.cu:49-56, no early termination.
 * ------------------------------------------------------------------------------------------ */
int tn_weights_fwd(const float *sigmas, const float *steps, const int32_t *info, float threshold,
                   float *weights, int64_t n_samples, int64_t n_rays, void *stream);
/* tn_weights_fwd that also raises gate[0] to 1.0 when any weight is > 0 (never lowers it: the caller zeroes it).  The
 * harness' device-side form of the reference's "Empty iteration" test (core.py:251-254: `(weights > 0).any()`). */
int tn_weights_fwd_gate(const float *sigmas, const float *steps, const int32_t *info, float threshold,
                        float *weights, float *gate, int64_t n_samples, int64_t n_rays, void *stream);
int tn_weights_bwd(const float *sigmas, const float *steps, const int32_t *info,
                   const float *weights, const float *grad_weights, float *grad_sigmas,
                   int64_t n_samples, int64_t n_rays, void *stream);

/* ------------------------------------------------------------------------------------------
 * a18  per-ray compositing                                     (reference core.py:256-265)
 * rendered[r] = sum_k w_k rgb_k (+ bg*(1-sum_k w_k) if bg != NULL); opacity[r] optional.
 * bwd: grad_rgbs[k] = w_k*g[r];  grad_weights[k] = <rgb_k, g[r]> - <bg, g[r]>.
 * One wave per ray; info must be 8-byte aligned (TN_E_ALIGN otherwise), as for the weights entry points.
 * ------------------------------------------------------------------------------------------ */
int tn_composite_fwd(const float *rgbs, const float *weights, const int32_t *info, const float *bg,
                     float *rendered, float *opacity, int64_t n_samples, int64_t n_rays, void *stream);
int tn_composite_bwd(const float *rgbs, const float *weights, const int32_t *info, const float *bg,
                     const float *grad_rendered, float *grad_rgbs, float *grad_weights,
                     int64_t n_samples, int64_t n_rays, void *stream);
/* Per-ray maps of the rendered weights w_k and sample distances t_k (tn_sample_pack_t) of ray r, k = 0..count-1:
 *   opacity[r]      = sum_k w_k (bit-identical to tn_composite_fwd's opacity: same lane order, same reduction tree);
 *   depth[r]        = sum_k w_k t_k / opacity[r]   (expected depth given a hit), 0 when opacity[r] == 0;
 *   median_depth[r] = t_j of the first j with sum_{k<=j} w_k >= opacity[r] / 2, 0 when opacity[r] == 0.
 * Rays without samples get 0 in all three.  Each output may be NULL; t_values may be NULL when depth and median_depth are.
 * One wave per ray; info must be 8-byte aligned.  No reference call site: the reference computes the opacity only to blend
 * the background (core.py:262-265) and returns neither map. */
int tn_ray_maps(const float *weights, const float *t_values, const int32_t *info, int64_t n_rays, float *opacity,
                float *depth, float *median_depth, void *stream);

/* ------------------------------------------------------------------------------------------
 * a5/a6  occupancy grid                                        (reference core.py:93-156)
 * grid is fp32 [D,H,W]; coords[...,0] indexes W (x), 1 -> H (y), 2 -> D (z), in [-1,1].
 * ------------------------------------------------------------------------------------------ */
/* core.py:147-156: out[i] = trilinear(grid, coords[i]) > threshold, bit-exact w.r.t. ATen's
 * grid_sampler_3d (align_corners=True, zeros padding).  values (optional) receives the taps. */
/* coarse[bz,by,bx] = max of grid over z in [4bz, 4bz+4], y, x likewise (clipped): every tap a point whose floor cell lies
 * in block (bz,by,bx) can read.  Rebuild after every change of the grid. */
int tn_occupancy_coarsen(const float *grid, int D, int H, int W, float *coarse, void *stream);
int tn_occupancy_query(const float *grid, int D, int H, int W, const float *coords, int64_t n,
                       float threshold, uint8_t *out, float *values, void *stream);
/* core.py:136: jittered voxel centres of depth slice `slice`: out[h*W+w] =
 * -1 + 2*((w,h,slice) + jitter)/(D,H,W) (the reference divides the flipped (x,y,z) index by the
 * un-flipped size vector; reproduced).  jitter [H,W,3] may be NULL: then a counter-based RNG
 * keyed by (seed, slice, h, w, c) supplies U[0,1). */
int tn_occupancy_slice_coords(int D, int H, int W, int slice, const float *jitter, uint64_t seed,
                              float *coords, void *stream);
/* core.py:138-143: alpha = 1-exp(-sigma*step); grid = alpha > thr ? 1 : decay*grid, over `n`
 * consecutive cells starting at grid_cells. */
int tn_occupancy_apply(float *grid_cells, const float *sigmas, int64_t n, float step_size,
                       float threshold, float decay, void *stream);
/* core.py:121-123,144: stats[0] = sum(grid) (fp64), stats[1] = #(grid > threshold) as fp64.
 * stats is a device buffer of 2 doubles, overwritten. */
int tn_occupancy_stats(const float *grid, int64_t n, float threshold, double *stats, void *stream);

/* ------------------------------------------------------------------------------------------
 * a1-a4, a7  ray marching + sample packing                    (reference core.py:11-88,158-188)
 * ------------------------------------------------------------------------------------------ */
enum { TN_MARCH_AABB = 0, TN_MARCH_UNBOUNDED = 1 };
enum { TN_CONTRACT_AABB = 0, TN_CONTRACT_MIP360_INF = 1, TN_CONTRACT_MIP360_L2 = 2,
       TN_CONTRACT_NONE = 3 /* tn_normal_frame only: no contraction, J = I */ };

typedef struct tn_sampler_desc {
    int32_t marcher;          /* TN_MARCH_*    (core.py:36-88)                               */
    int32_t contraction;      /* TN_CONTRACT_* (core.py:11-31)                               */
    int32_t n_samples;        /* candidates per ray S                                        */
    int32_t grid_d, grid_h, grid_w;
    float aabb[6];            /* lo xyz, hi xyz (marcher AABB and/or contraction AABB)       */
    float near, far;          /* AABB marcher clamp (core.py:81)                             */
    float step_size;          /* AABB marcher: ||hi-lo||/S as computed by the caller (fp32)  */
    float threshold;          /* occupancy threshold min(base, mean) (core.py:125-127)       */
    const float *t_table;     /* unbounded marcher: t[S] and delta[S] (core.py:52-58)        */
    const float *delta_table;
    const float *grid;        /* occupancy grid [D,H,W]                                      */
    const float *jitter;      /* training: U[0,1) [R,S] (core.py:173) or NULL                */
    uint64_t seed;            /* training with jitter==NULL && use_rng: counter-based RNG    */
    int32_t use_rng;
    int32_t reserved;
    const float *coarse;      /* optional [ceil(D/4),ceil(H/4),ceil(W/4)] block maxima written by tn_occupancy_coarsen:
                               * candidates whose 2x2x2 taps all lie under a block whose maximum is safely below the
                               * threshold are rejected without reading the taps (same mask, bit for bit); NULL = off */
} tn_sampler_desc;

/* Stand-alone marcher / contraction calls (core.py:47-59,72-88 and core.py:15-31) with the same
 * arithmetic as the fused sampler: t,delta [R,S]; coords_out [n,3], mask [n] (AABB only, else NULL). */
int tn_march_rays(const tn_sampler_desc *desc, const float *rays_o, const float *rays_d, int64_t n_rays,
                  float *t_values, float *step_sizes, void *stream);
int tn_contract(const tn_sampler_desc *desc, const float *coords, int64_t n, float *coords_out,
                uint8_t *mask, void *stream);

/* pass 1: per-ray occupancy bitmask ([R, ceil(S/64)] uint64) and kept-sample count. */
int tn_sample_mask(const tn_sampler_desc *desc, const float *rays_o, const float *rays_d,
                   int64_t n_rays, uint64_t *maskbits, int32_t *counts, void *stream);
/* pass 2: info[r] = (exclusive_scan(counts)[r] + base_offset[0], counts[r]); total[0] = sum.
 * base_offset (device int32, may be NULL = 0) implements run.py:231 `info[:,0] += current_size`. */
int tn_sample_scan(const int32_t *counts, int64_t n_rays, const int32_t *base_offset,
                   int32_t *info, int32_t *total, void *stream);
/* a8 (reference run.py:215-244), device side: the harness draws loader batches of `batch_size` rays until
 * int(cur*(1+1/k)) >= target.  Given the kept-sample counts of n_rays = n_batches*batch_size candidate rays,
 * plan[0] = k (loader batches consumed), plan[1] = N (packed samples), plan[2] = R = k*batch_size rays,
 * plan[3] = 1 if the rule tripped within the supplied rays (else every supplied batch is used). */
int tn_batch_plan(const int32_t *counts, int64_t n_rays, int32_t batch_size, int64_t target, int32_t *plan,
                  void *stream);
/* tn_batch_plan and tn_sample_scan(counts, n_rays, NULL, info, NULL) over ALL candidate rays as one multi-workgroup launch
 * (the training step's form: the harness uses the first plan[2] rows of info once the plan is on the host, so that nothing but
 * tn_sample_pack is left behind the step's read-back; reference run.py:215-244 + core.py:179-181). */
int tn_batch_plan_scan(const int32_t *counts, int64_t n_rays, int32_t batch_size, int64_t target, int32_t *plan,
                       int32_t *info, void *stream);
/* pass 3: packed[start_r - base + j] = (contracted xyz, ray dir, step) for the j-th set bit
 * (core.py:182-186).  ray_ids / steps (optional) receive the ray index and the step size (column 6) of every packed
 * sample as contiguous arrays (what the weights kernels and the per-ray colour-head table index). */
int tn_sample_pack(const tn_sampler_desc *desc, const float *rays_o, const float *rays_d,
                   int64_t n_rays, const uint64_t *maskbits, const int32_t *info,
                   const int32_t *base_offset, float *packed, int32_t *ray_ids, float *steps, int64_t capacity,
                   void *stream);
/* tn_sample_pack that also writes t_values[row] (may be NULL, [capacity]): the ray parameter t at which the packed sample was
 * taken, jitter included -- t_min + k*step (+ jitter*step) for the AABB marcher, t_table[k] (+ jitter*delta_k) for the unbounded
 * one (core.py:84-85, 52-58, 173).  The rays are unit length (data.py), so t is a distance in world units.  Every other output is
 * the same as tn_sample_pack's, bit for bit (the same kernel).  No reference call site: the reference drops t after
 * core.py:174; it feeds tn_ray_maps. */
int tn_sample_pack_t(const tn_sampler_desc *desc, const float *rays_o, const float *rays_d,
                     int64_t n_rays, const uint64_t *maskbits, const int32_t *info,
                     const int32_t *base_offset, float *packed, int32_t *ray_ids, float *steps, float *t_values,
                     int64_t capacity, void *stream);

/* ------------------------------------------------------------------------------------------
 * a9  positional encoding                                      (reference models.py:30-39)
 * out[n, c*2F + f] = sin(x[n,c]*freqs[f]), out[n, c*2F + F + f] = cos(..)
 * ------------------------------------------------------------------------------------------ */
int tn_posenc_fwd(const float *x, int64_t n, int n_channels, const float *freqs, int n_freqs,
                  float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * a10-a14  fused MLP heads on fp32 MFMA                        (reference models.py:7-89)
 * One launch evaluates  act_out( W_L ... relu(W_1 relu(W_0 enc(x) + b_0) + b_1) ... + b_L ).
 * Weights are torch nn.Linear layout [out,in] row-major.
 * ------------------------------------------------------------------------------------------ */
enum { TN_ACT_NONE = 0, TN_ACT_EXP_M1 = 1 /* exp(y-1), models.py:74 */, TN_ACT_SIGMOID = 2,
       TN_ACT_EXP = 3 /* tn_basis_dot_* only: exp(y) with the clamped backward of models.py:42-53 */ };
enum { TN_ENC_NONE = 0,
       TN_ENC_POSENC = 1,       /* input = PE_F(x[:, :3])                      (models.py:67)    */
       TN_ENC_DIR_CAT = 2,      /* input = cat[PE_F(dirs), dirs, x]            (models.py:87)    */
       TN_ENC_AUX_CAT = 3 };    /* input = cat[aux_table[aux_index[row]], x]: the same colour-head input with
                                 * cat[PE_F(d), d] evaluated once per RAY (tn_dir_encode) instead of per sample */
#define TN_MLP_MAX_LAYERS 12
#define TN_MLP_ACCUM_GRAD_X 1   /* tn_mlp_bwd: grad_x += instead of = (two heads sharing one feature tensor) */
#define TN_MLP_STASHED 2        /* tn_mlp_bwd: workspace holds the activations written by tn_mlp_fwd_stash
                                 * (same desc, x, aux, n): no forward recomputation */
#define TN_MLP_CHAIN_ONLY 4     /* tn_mlp_bwd_pair: data gradients only (grad_x and the G rows of the workspace) ...   */
#define TN_MLP_WGRAD_ONLY 8     /* ... weight / bias gradients only, from a workspace a CHAIN_ONLY call completed.  The split
                                 * lets a caller start consuming grad_x (e.g. scatter it and launch a gradient all-reduce)
                                 * while the weight gradients are still being computed. */
#define TN_MLP_GRAD_Y_ROWS 16   /* tn_mlp_bwd of a layer-by-layer configuration (tn_mlp_rows_view): d loss / d y already sits in the
                                 * workspace as [feature][32-sample] rows (a consumer's grad_x_rows); grad_y is ignored */

#define TN_MLP_BF16X3 32        /* wide stacks evaluated layer by layer (width 128 / 256): matrix products on the bf16 matrix cores with
                                 * EXACT three-way operand splits (x = hi + mid + lo in bf16, six of the nine partial products,
                                 * fp32 accumulate: every product good to 2^-23, the error of an fp32 product's own rounding) instead
                                 * of v_mfma_f32_32x32x2_f32 -- 2.67 x the matrix rate, results equal to fp32 rounding.  Ignored by
                                 * configurations without such a form. */

#define TN_MLP_F16X2 64         /* as TN_MLP_BF16X3, with the hidden layers on the fp16 matrix cores instead: two-term operand splits
                                 * (x s = hi + lo in fp16: 22 of fp32's 24 significand bits), three partial products, power-of-two scales
                                 * -- per sample column and per layer in the forward / data gradient, per operand and launch in the
                                 * weight gradient -- that are taken out of the fp32 accumulators again: no overflow whatever the
                                 * data, the same distance from an fp64 evaluation as the fp32 MFMA, half the matrix time of bf16x3
                                 * (csrc/mlp_f2_layers.hip).  The workspace's last 256 bytes carry the per-layer maxima between
                                 * the launches of a step.  Default of tinynerf_amd.models. */

#define TN_MLP_ROWS_ONLY 128    /* tn_mlp_fwd_stash of a layer-by-layer stack that offers row views (tn_mlp_rows_view) under TN_MLP_F16X2:
                                 * y is NOT written -- the output exists only as the workspace's [feature][32-sample] rows, which the
                                 * consumer reads through tn_mlp_desc::x_rows (TN_MLP_X_FROM_ROWS).  Saves the 4 * out bytes per
                                 * sample of the row-major copy.  `y` must still be a valid pointer. */
#define TN_MLP_X_FROM_ROWS 256  /* tn_mlp_fwd_stash of a width-64 head: x is read from x_rows ONLY (the producer ran with
                                 * TN_MLP_ROWS_ONLY; `x` is not dereferenced).  TN_E_CONFIG unless the launch is one that reads the row
                                 * view: TN_MLP_F16X2, in_dim 128 or 256, <= 4 outputs.  Without the flag such a launch still
                                 * prefers x_rows when they are set (coalesced 128-byte rows instead of 16 bytes per lane and sample). */

#define TN_MLP_SKIP_LAST 1024   /* a wide stack evaluated layer by layer whose LAST layer is a plain Linear feeding only Linear first layers of
                                 * its consumers (reference models.py:59-89: Linear(256, 256) then Linear(256, 64) twice with nothing in
                                 * between): W_head (W_last h + b_last) + b_head = (W_head W_last) h + (W_head b_last + b_head), so the caller
                                 * merges the two layers' parameters and the stack stops at its last HIDDEN activation.  tn_mlp_fwd_stash
                                 * then runs layers 0 .. L - 2 only (y is not written), tn_mlp_rows_view_hidden says where that activation,
                                 * the slot for its gradient and its ReLU bit rows are, and tn_mlp_bwd (with TN_MLP_STASHED |
                                 * TN_MLP_GRAD_Y_ROWS) starts from that gradient and leaves the last layer's parameter gradients untouched
                                 * (they follow from the merged parameters' gradients by the chain rule).  One layer launch less in the
                                 * forward pass, two less in the backward pass, and the feature tensor never exists. */
#define TN_MLP_LAYERWISE 2048   /* a TN_MLP_F16X2 stack in tn_mlp_fwd_ws / tn_mlp_fwd_stash / tn_mlp_bwd_layers: one launch per layer and direction
                                 * with the activations / gradients crossing HBM as workspace rows (the form of rounds 3 - 5) instead of the
                                 * cross-layer persistent launches of round 6 (csrc/mlp_fused_f2.hip: inference forward, training forward and
                                 * data-gradient chain with the sample columns in registers for the whole stack, weights streamed through
                                 * LDS).  Same results to fp32 rounding, same workspace layout; kept as the parity partner of the fused
                                 * launches in tests and for A / B timing.  The weight-gradient launches are per layer in both forms. */
#define TN_MLP_LEAN 512        /* the paired width-64 heads (tn_mlp_fwd_stash_pair / tn_kplanes_mlp_fwd_pair and their backward twins), round 5:
                                 * the training forward writes only the ReLU bit masks, the last pre-activation and the feature rows --
                                 * NOT the hidden activations H_l (1.3 KB per sample that crossed HBM twice) -- and the weight-gradient
                                 * half of the backward (TN_MLP_WGRAD_ONLY or the full call) rebuilds them from the feature row: a
                                 * wave recomputes its 32 samples' forward on the fp16 matrix cores (the f16x2 arithmetic of the
                                 * forward) in BOTH operand orientations -- out[feature][sample] to feed the next layer,
                                 * out[sample][feature] as the weight gradient's MFMA operand: no transposition through memory --
                                 * and multiplies with the G rows of the data-gradient chain as exact three-way bf16 splits
                                 * (csrc/mlp_wgrad_rc.hip).  Set on BOTH descriptors of BOTH calls; the workspace layout is unchanged
                                 * (its H rows stay unwritten).  Reference: the autograd of src/models.py:7-28,70-89. */

typedef struct tn_mlp_desc {
    int32_t n_layers;                         /* number of Linear layers (>= 1)               */
    int32_t in_dim;                           /* width of x (before encoding)                 */
    int32_t dims[TN_MLP_MAX_LAYERS + 1];      /* dims[0] = encoded input width, dims[l+1] = out of layer l */
    int32_t encoding;                         /* TN_ENC_*                                     */
    int32_t n_freqs;                          /* F for the encodings                          */
    int32_t out_activation;                   /* TN_ACT_*                                     */
    int32_t flags;                            /* TN_MLP_*                                     */
    const float *freqs;                       /* [n_freqs] encoding frequencies (models.py:34); NULL = 2^j*pi */
    const float *weights[TN_MLP_MAX_LAYERS];  /* [dims[l+1], dims[l]]                         */
    const float *biases[TN_MLP_MAX_LAYERS];   /* [dims[l+1]]                                  */
    /* TN_ENC_AUX_CAT: `aux` is a table [n_aux, aux_stride] whose rows hold dims[0]-in_dim values followed by
     * zeros (aux_stride and in_dim multiples of 4); row i of x uses table row aux_index[i] (NULL: row i). */
    const int32_t *aux_index;
    int32_t aux_stride;
    int32_t reserved;
    /* tn_mlp_fwd only: optional per-row gate [n] (the renderer passes the volume-rendering weights, core.py:246-251: the
     * colour head only matters where w > 0).  A 32-row tile whose gates are all 0 is not evaluated and yields 0. */
    const float *row_gate;
    /* Row views (optional, all NULL / 0 by default): x and grad_x of tn_mlp_bwd as [feature][32-sample] rows per 32-sample
     * tile -- the layout in which a wide stack's layer-by-layer kernels keep activations and gradients in their workspace
     * (tn_mlp_rows_view), so that the heads behind a width-256 feature stack (reference models.py:59-89, core.py:239-249)
     * exchange both with it without a row-major round trip:
     *   x_rows       value of feature f of sample 32 t + j at x_rows[t * x_rows_tile_stride + 32 f + j] (samples >= n: 0).
     *                tn_mlp_bwd (two-pass form, TN_MLP_STASHED) then takes the first layer's weight gradient over the x
     *                columns from these rows; needs in_dim % 32 == 0.  tn_mlp_fwd_stash (f16x2 heads, in_dim 128 / 256) reads
     *                its first-layer operands from them.  x itself is still required unless TN_MLP_X_FROM_ROWS says otherwise.
     *   grad_x_rows  tn_mlp_bwd writes (TN_MLP_ACCUM_GRAD_X: adds) d loss / d x there, same layout, INSTEAD of grad_x. */
    const float *x_rows;
    float *grad_x_rows;
    int64_t x_rows_tile_stride;               /* floats */
    int64_t grad_x_rows_tile_stride;
    /* ReLU bit rows for grad_x_rows (optional; tn_mlp_rows_view_hidden): when the rows a head reads are a HIDDEN activation of the
     * producer (TN_MLP_SKIP_LAST), d loss / d x leaves multiplied by relu'(x) -- bit r of the dword at
     * grad_x_mask_rows[t * grad_x_mask_tile_stride + 64 b + lane] says whether feature 32 b + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of
     * sample 32 t + (lane & 31) was positive (the layer kernels' bit rows, two 128-byte rows per 32-feature block). */
    const void *grad_x_mask_rows;
    int64_t grad_x_mask_tile_stride;          /* dwords */
} tn_mlp_desc;

/* Merged parameters for TN_MLP_SKIP_LAST (reference models.py:59-89, 239-247: Linear(F, F) -> Linear(F [+ other columns], rows), nothing
 * in between).  Per consumer ("head"): weight [rows][ld] whose columns [col0, col0 + F) multiply the stack's output, bias [rows].
 *   tn_linear_merge_fwd: out_weight[:, col0 .. col0 + F) = weight[:, col0 .. col0 + F) w_last, the other columns copied;
 *                        out_bias = bias + weight[:, col0 .. col0 + F) b_last.
 *   tn_linear_merge_bwd: grad_merged_* = gradients of those merged parameters; ADDS the gradients of the original parameters to
 *                        out_weight / out_bias (now: gradient buffers of weight / bias) and to grad_w_last [F][F] / grad_b_last [F]. */
#define TN_MERGE_MAX_HEADS 4
typedef struct tn_merge_head {
    const float *weight, *bias;
    int32_t rows, ld, col0, reserved;
    float *out_weight, *out_bias;
    const float *grad_merged_weight, *grad_merged_bias;       /* tn_linear_merge_bwd only */
} tn_merge_head;
int tn_linear_merge_fwd(int32_t n_heads, const tn_merge_head *heads, const float *w_last, const float *b_last, int32_t F, void *stream);
int tn_linear_merge_bwd(int32_t n_heads, const tn_merge_head *heads, const float *w_last, const float *b_last, int32_t F,
                        float *grad_w_last, float *grad_b_last, void *stream);

/* One plain Linear (reference src/models.py:183-191: KPlanesExplicitOpacityDecoder.net = torch.nn.Linear(96, 96), the only
 * Linear on the reference's path outside an MLP stack): y [n, out] = x [n, in] weight^T + bias (bias may be NULL), weight
 * [out, in] row-major as torch.nn.Linear holds it, 1 <= in, out <= 128, fp32 MFMA. */
int tn_linear_fwd(const float *x, const float *weight, const float *bias, int64_t n, int32_t in_features,
                  int32_t out_features, float *y, void *stream);
/* ... and its backward: grad_x [n, in] = grad_y weight (written; NULL: skipped), grad_weight [out, in] += grad_y^T x and
 * grad_bias [out] += column sums of grad_y (both ACCUMULATED, as autograd does into .grad; NULL: skipped -- each on its own:
 * x may be NULL when grad_weight is). */
int tn_linear_bwd(const float *x, const float *weight, const float *grad_y, int64_t n, int32_t in_features,
                  int32_t out_features, float *grad_x, float *grad_weight, float *grad_bias, void *stream);

/* Row views into the workspace of tn_mlp_fwd_stash(desc, ..., n) for a layer-by-layer configuration without output
 * activation (the Vanilla 256 x 10 and Cobafa 128 x 6 feature stacks): offsets in floats from the workspace base of
 *   y_rows       y as [feature][32-sample] rows -- valid until this stack's tn_mlp_bwd runs;
 *   grad_y_rows  where tn_mlp_bwd with TN_MLP_GRAD_Y_ROWS expects d loss / d y in that layout;
 * and the tile stride (floats per 32 samples) of both.  TN_E_CONFIG when the configuration has no such views. */
int tn_mlp_rows_view(const tn_mlp_desc *desc, int64_t n, int64_t *y_rows, int64_t *grad_y_rows, int64_t *tile_stride);
/* ... of a stack that ran / will run with TN_MLP_SKIP_LAST: the last hidden activation h (offsets in floats from the workspace
 * base, [feature][32-sample] rows, tile stride as above), the slot where tn_mlp_bwd expects d loss / d h -- ALREADY multiplied by
 * relu'(h): consumers apply tn_mlp_desc::grad_x_mask_rows --, and h's ReLU bit rows (offset in floats = dwords; the bit rows' tile
 * stride equals tile_stride). */
int tn_mlp_rows_view_hidden(const tn_mlp_desc *desc, int64_t n, int64_t *h_rows, int64_t *grad_h_rows, int64_t *mask_rows,
                            int64_t *tile_stride);

/* y [n, dims[n_layers]] = MLP(x [n,in_dim], aux [n,3] (dirs for TN_ENC_DIR_CAT, else NULL)).
 * pre_act (optional, [n, dims[n_layers]]) receives the last layer's output before out_activation. */
int tn_mlp_fwd(const tn_mlp_desc *desc, const float *x, const float *aux, int64_t n, float *y,
               float *pre_act, void *stream);
/* Inference forward with scratch: wide stacks on positional-encoding inputs (the Vanilla feature MLP, models.py:59-68) or on
 * <= 64 plain inputs (Cobafa's 36 gathered features into its 128-wide stack, models.py:239-247: staged as zero-padded rows) run
 * layer by layer through the weight-in-register kernels of the training forward, the activations ping-ponging between two
 * [feature][32-sample] row buffers in `workspace` (tn_mlp_fwd_workspace_bytes(desc, n) bytes: 2.3 KB per sample at width
 * 256; 0 = this configuration has no such form, use tn_mlp_fwd).  Same MFMA steps in the same order as the training
 * forward: identical y.  Used by infer() (run.py:15-50) and the occupancy refresh (core.py:133-145). */
int64_t tn_mlp_fwd_workspace_bytes(const tn_mlp_desc *desc, int64_t n);
int tn_mlp_fwd_ws(const tn_mlp_desc *desc, const float *x, const float *aux, int64_t n, float *y, void *workspace,
                  int64_t workspace_bytes, void *stream);
/* Training forward: y as tn_mlp_fwd, plus the hidden activations, their ReLU bit masks and the last layer's
 * pre-activation into `workspace` (tn_mlp_bwd_workspace_bytes(desc, n) bytes) in the layout tn_mlp_bwd's
 * backward (two-pass or layer-by-layer form) uses; pass the same workspace to tn_mlp_bwd with TN_MLP_STASHED set.
 * Returns TN_E_CONFIG for configurations whose backward takes no workspace (tn_mlp_bwd_workspace_bytes == 0). */
int tn_mlp_fwd_stash(const tn_mlp_desc *desc, const float *x, const float *aux, int64_t n, float *y,
                     void *workspace, int64_t workspace_bytes, void *stream);
/* Training forward of TWO heads on the same x in one launch (x is read from HBM once): `desc` (TN_ENC_NONE or
 * TN_ENC_AUX_CAT) and `partner` (TN_ENC_NONE, same in_dim), both of hidden width 64; workspaces as for tn_mlp_fwd_stash. */
int tn_mlp_fwd_stash_pair(const tn_mlp_desc *desc, const tn_mlp_desc *partner, const float *x, const float *aux, int64_t n,
                          float *y, float *partner_y, void *workspace, int64_t workspace_bytes, void *partner_workspace,
                          int64_t partner_workspace_bytes, void *stream);
/* out[r, :] = [PE_F(dirs[r]) (6F, models.py:36-39 order), dirs[r] (3), 0 ...] with row stride `stride` >= 6F+3:
 * the aux table of TN_ENC_AUX_CAT for the colour head (models.py:87). */
int tn_dir_encode(const float *dirs, int64_t n, const float *freqs, int n_freqs, float *out, int stride, void *stream);
/* Backward of tn_mlp_fwd: recomputes the hidden activations, accumulates (+=) weight/bias
 * gradients into grad_weights[l]/grad_biases[l] (same shapes; must be initialised by the caller)
 * and writes (flags & TN_MLP_ACCUM_GRAD_X: adds to) grad_x [n,in_dim] when non-NULL (TN_ENC_POSENC: no grad_x, coords carry no grad;
 * TN_ENC_DIR_CAT: gradient w.r.t. the feature part x only).
 * workspace (optional, tn_mlp_bwd_workspace_bytes(desc, n) bytes, uninitialised) selects the two-pass
 * form (data-gradient chain with LDS-resident weights, then a sample-reducing weight-gradient kernel);
 * without it, or for configurations the two-pass form does not cover (it returns 0 bytes), the
 * single-kernel form runs. */
int64_t tn_mlp_bwd_workspace_bytes(const tn_mlp_desc *desc, int64_t n);
int tn_mlp_bwd(const tn_mlp_desc *desc, const float *x, const float *aux, const float *grad_y,
               int64_t n, float *const *grad_weights, float *const *grad_biases, float *grad_x,
               void *workspace, int64_t workspace_bytes, void *stream);
/* Backward of TWO heads that read the same x in one data-gradient pass (the K-Planes colour head `desc` and its
 * 2-layer sigma head `partner`, models.py:70-89): grad_x = d/dx of both, written once.  Both descriptors carry
 * TN_MLP_STASHED (workspaces written by tn_mlp_fwd_stash); partner: 2 layers, TN_ENC_NONE, same in_dim (multiple of
 * 32) and hidden width 64.  Parameter gradients accumulate (+=) as in tn_mlp_bwd.
 * With row views on both descriptors (the heads behind a wide stack: the same x_rows / grad_x_rows [/ grad_x_mask_rows], TN_ENC_AUX_CAT on
 * `desc`, grad_x == NULL) and TN_MLP_F16X2, both chains stop at their G_0 rows, grad_x_rows = W_0[:, x]^T G_0 of both heads is one launch
 * on the fp16 matrix cores (two-term splits, 2^-22 relative; the fp32 / bf16x3 modes keep the fp32 MFMA), and both first layers' x-column
 * weight gradients share one launch. */
int tn_mlp_bwd_pair(const tn_mlp_desc *desc, const tn_mlp_desc *partner, const float *x, const float *aux,
                    const float *grad_y, const float *partner_grad_y, int64_t n, float *const *grad_weights,
                    float *const *grad_biases, float *const *partner_grad_weights, float *const *partner_grad_biases,
                    float *grad_x, void *workspace, int64_t workspace_bytes, void *partner_workspace,
                    int64_t partner_workspace_bytes, void *stream);

/* 1 when the pair (`desc` = the 5-layer head, `partner` = the 2-layer head on the same x) can run under TN_MLP_LEAN: the reference's
 * decoders as f16x2 heads (src/run.py:133-139 + TN_MLP_F16X2: colour 147 -> 64 x 4 -> 3 on [PE_8(d), d, x (96)] through a per-ray table,
 * sigma 96 -> 64 -> 1), else 0.  Callers choose the training forward's form with it. */
int tn_mlp_lean_supported(const tn_mlp_desc *desc, const tn_mlp_desc *partner);

/* ------------------------------------------------------------------------------------------
 * a15/a16  K-Planes feature field                              (reference models.py:93-163)
 * Planes are stored channel-last: plane[s][p] is fp32 [H_s, W_s, C] (torch memory_format
 * channels_last of the reference's [1,C,H,W] parameter, so the state_dict shape is unchanged).
 * feat[n, s*C + c] = prod_p bilinear(plane[s][p], x[n, pair_p])[c], pairs (0,1),(0,2),(1,2).
 * planes[s][1] / planes[s][2] may be NULL: that factor is 1 (KPlanesFeaturePlane.forward, models.py:105-113).
 * ------------------------------------------------------------------------------------------ */
#define TN_KPLANES_MAX_SCALES 4
typedef struct tn_kplanes_desc {
    int32_t n_scales;
    int32_t channels;                               /* C, multiple of 4, <= 32              */
    int32_t height[TN_KPLANES_MAX_SCALES];
    int32_t width[TN_KPLANES_MAX_SCALES];
    const float *planes[TN_KPLANES_MAX_SCALES][3];  /* [H,W,C] each                          */
} tn_kplanes_desc;

/* x has row stride x_stride floats (7 when reading packed_samples directly, 3 for [n,3]). */
int tn_kplanes_fwd(const tn_kplanes_desc *desc, const float *x, int64_t x_stride, int64_t n,
                   float *feat, void *stream);
/* grad_planes[s][p] ([H,W,C], += with fp32 atomics; caller initialises) from grad_feat [n, S*C]. */
int tn_kplanes_bwd(const tn_kplanes_desc *desc, const float *x, int64_t x_stride, int64_t n,
                   const float *grad_feat, float *const (*grad_planes)[3], void *stream);

/* ------------------------------------------------------------------------------------------
 * a19  K-Planes regularisers                         (reference models.py:115-121,165-181)
 * One pass per plane ([H,W,C] channel-last) instead of the 4 strided torch passes per plane of
 * the reference.  fwd: sums[0] += sum (p[y+1]-p[y])^2, sums[1] += sum (p[x+1]-p[x])^2,
 * sums[2] += sum |p|  (fp64 device accumulators, caller zeroes them).
 * bwd: grad += upstream[0] * ( cy * d/dp sum_dy + cx * d/dp sum_dx + cl1 * sign(p) ), where
 * upstream is a device scalar (dLoss/dRegulariser) and cy, cx, cl1 fold the means and weights. */
int tn_plane_reg_fwd(const float *plane, int H, int W, int C, double *sums, void *stream);
int tn_plane_reg_bwd(const float *plane, int H, int W, int C, float cy, float cx, float cl1,
                     const float *upstream, float *grad, void *stream);

/* Every plane of the field in one launch, forward and backward fused for a constant upstream gradient
 * (the harness: d(loss * grad_scale)/d(regulariser) is a host scalar): sums[3*i + {0,1,2}] += the three sums
 * of tn_plane_reg_fwd for item i (sums may be NULL), grad_i += upstream * (cy, cx, cl1 terms) (grad may be NULL).
 * `items` is a HOST array. */
#define TN_MULTI_MAX 32
typedef struct tn_plane_reg_item {
    const float *plane;       /* [H,W,C] channel-last */
    float *grad;              /* same layout, += ; NULL = value only */
    int32_t H, W, C;
    float cy, cx, cl1;
} tn_plane_reg_item;
int tn_plane_reg_multi(const tn_plane_reg_item *items, int32_t n_items, float upstream, double *sums, void *stream);

/* ------------------------------------------------------------------------------------------
 * a20  Cobafa factorised field                                  (reference models.py:209-266)
 * feat[n, off_i + c] = trilinear(basis_i, saw_i(x))[c] * trilinear(coef, x)[i],
 * saw_i(x) = 2*((f_i*x) mod 1) - 1 (models.py:213), levels concatenated (models.py:263-265).
 * f_i <= 0 selects saw_i(x) = x: with a 1x1x1 coefficient grid holding 1 this is the plain trilinear
 * lookup of CobafaGrid.forward (models.py:223-232).
 * Grids are channel-last [D,H,W,C] (torch channels_last_3d of the reference's [1,C,D,H,W]).
 * ------------------------------------------------------------------------------------------ */
#define TN_COBAFA_MAX_LEVELS 8
typedef struct tn_cobafa_desc {
    int32_t n_levels;
    int32_t coef_res[3];                           /* D,H,W of the coefficient grid (C = n_levels) */
    int32_t res[TN_COBAFA_MAX_LEVELS][3];          /* D,H,W of basis grid i                        */
    int32_t channels[TN_COBAFA_MAX_LEVELS];        /* <= 8                                         */
    float freqs[TN_COBAFA_MAX_LEVELS];
    const float *coef;                             /* [D,H,W,n_levels]                             */
    const float *basis[TN_COBAFA_MAX_LEVELS];      /* [D,H,W,channels[i]]                          */
} tn_cobafa_desc;
int tn_cobafa_fwd(const tn_cobafa_desc *desc, const float *x, int64_t n, float *feat, void *stream);
/* grad_coef / grad_basis[i]: same layouts as the grids, += with fp32 atomics (caller initialises) */
int tn_cobafa_bwd(const tn_cobafa_desc *desc, const float *x, int64_t n, const float *grad_feat, float *grad_coef,
                  float *const *grad_basis, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multiresolution hash-grid field (Instant-NGP, Mueller et al. 2022).  No reference call site: the reference has three
 * fields (Vanilla, K-Planes, Cobafa; run.py:130-152) and no hash encoding.
 * Level plan, made by the CALLER in float64 and handed over as integers (no kernel computes a resolution): L levels,
 *   b = exp(ln(N_max / N_min) / (L - 1)) (1 for L = 1), N_l = floor(N_min * b^l + 0.5); level l has N_l + 1 nodes per axis.
 *   dense  when (N_l + 1)^3 <= T = 2^log2_T: (N_l + 1)^3 entries, rounded up to a multiple of 8 (the padding is never read);
 *   hashed otherwise: T entries.  offset_l = entries of the levels before l.  One table [sum entries][features], fp32.
 * Position: x in [-1, 1]^3 = columns 0..2 of a row of `x_stride` floats (7: the packed samples, 3: a plain [n, 3] tensor).
 *   Per axis in fp32: p = fmaf(x, 0.5f * N_l, 0.5f * N_l) (one rounding), p = min(max(p, 0), N_l) with a NaN landing on 0,
 *   i = min((int)p, N_l - 1), f = p - i (exact).  Nothing outside the table is ever read, whatever x holds.
 * Index of node (ix, iy, iz): dense ix + (N_l+1) * (iy + (N_l+1) * iz); hashed (ix ^ iy * 2654435761u ^ iz * 805459861u) & (T - 1)
 *   in uint32 arithmetic with wrap-around (the primes of Instant-NGP).
 * Forward:  feat[n, l * F + c] = sum over the 8 corners of w * table[offset_l + idx][c], w = product over the axes of f or 1 - f.
 * Backward: grad_table[offset_l + idx][c] += w * grad_feat[n, l * F + c] with fp32 atomics (the caller initialises grad_table;
 *   two corners of one sample that collide in a hashed level both add).  No gradient goes to x.
 * The tiny-cuda-nn encoding differs (its scale is N_min * b^l - 1 with a +0.5 shift of the position, and b is exp2 of a float):
 *   its tables do not load here.
 * TN_E_CONFIG: n_levels outside 1..16, features not 2 or 4, res < 1, a hashed level whose entries is not a power of two, a dense
 * level with entries < (res + 1)^3, offsets that overlap.  TN_E_SIZE: n < 0 or x_stride < 3.  TN_E_ALIGN: table / grad_table /
 * feat / grad_feat not 16-byte aligned.  n == 0 returns TN_OK without a launch.
 * ------------------------------------------------------------------------------------------ */
#define TN_HASHGRID_MAX_LEVELS 16
typedef struct tn_hashgrid_desc {
    int32_t n_levels, features;                  /* features: 2 or 4 */
    int32_t res[TN_HASHGRID_MAX_LEVELS];         /* N_l */
    int32_t hashed[TN_HASHGRID_MAX_LEVELS];      /* 0 dense, 1 hashed */
    int64_t entries[TN_HASHGRID_MAX_LEVELS];     /* dense: padded node count; hashed: a power of two */
    int64_t offset[TN_HASHGRID_MAX_LEVELS];      /* in entries */
    const float *table;                          /* [sum entries][features], 16-byte aligned */
} tn_hashgrid_desc;
int tn_hashgrid_fwd(const tn_hashgrid_desc *desc, const float *x, int64_t x_stride, int64_t n, float *feat, void *stream);
int tn_hashgrid_bwd(const tn_hashgrid_desc *desc, const float *x, int64_t x_stride, int64_t n, const float *grad_feat,
                    float *grad_table, void *stream);

/* ------------------------------------------------------------------------------------------
 * Surface normals: the analytic gradient of the density with respect to the sample position, for the two fields that sit directly
 * in front of the small sigma head (K-Planes, hash grid).  No reference call site: the reference differentiates with respect to
 * parameters only and renders no normals.  Inference only.
 * Sigma head (reference models.py:70-76, VanillaOpacityDecoder): y(f) = b2 + sum_j w2_j max(0, h_j), h = W1 f + b1, sigma = exp(y - 1).
 *   sigma > 0, so -grad sigma / |grad sigma| = -grad y / |grad y|: neither the activation nor sigma is needed.  With
 *   relu'(h) = [h > 0] (torch's backward: 0 at h == 0):  g = dy/df = W1^T (w2 . [h > 0]), an F-vector per sample.
 * Contracted frame: grad_x y = sum_c g_c df_c/dx, x = columns 0..2 of a row of `x_stride` floats, as the field's forward reads them.
 *   K-Planes: f[s C + c] = P0(x0,x1) P1(x0,x2) P2(x1,x2) per scale -> the product rule over the three planes.  A plane's value and cell
 *     are the forward's (same ix, iy, floor cell, zero padding; u indexes W, v indexes H).  With the cell's texels t_nw, t_ne, t_sw, t_se
 *     (an out-of-bounds tap counts as 0) and fx = ix - floor(ix), gx = 1 - fx, fy, gy likewise:
 *       dP/du = (W - 1)/2 * ((t_ne - t_nw) gy + (t_se - t_sw) fy),    dP/dv = (H - 1)/2 * ((t_sw - t_nw) gx + (t_se - t_ne) fx)
 *     -- the derivative inside the cell the forward chose, right-sided at a node.
 *   Hash grid: per level, p_a, i_a, f_a as defined above;  dfeat/dx_a = (N_l / 2) * sum over the 8 corners of (+1 for the upper corner
 *     on axis a, -1 for the lower) * (the weights of the other two axes) * table[...];  0 on an axis where the clamp acts, i.e. where
 *     fmaf(x, N_l/2, N_l/2) is < 0, > N_l or NaN.
 * World frame: v = -J^T grad_x y, J = d x / d X the Jacobian of the contraction, recovered from the contracted x alone:
 *   TN_CONTRACT_NONE        J = I
 *   TN_CONTRACT_AABB        J = diag(2 / (hi - lo))
 *   TN_CONTRACT_MIP360_INF / _L2 (p = inf / 2): u = 2 x, s = |u|_p;  s <= 1: J = I / 2;  s >= 2 or not finite: v = 0;  otherwise
 *     m = 1 / (2 - s), X = (m / s) u,  J_ij = ((2/m - 1/m^2) delta_ij + X_i (2/m^3 - 2/m^2) dm/dX_j) / 2,
 *     dm/dX_j = sign(X_k) delta_jk with k the lowest axis with |X_k| = m (p = inf), = X_j / m (p = 2).
 * Outputs: normals [n,3] = v / |v| when |v| is finite and > 0, else (0,0,0) -- unit, pointing from dense to empty; also (0,0,0) for a
 *   row whose x is not finite.  grad [n,3] = grad_x y before the frame.  Either may be NULL, not both.  gate [n] (optional; the renderer
 *   passes the volume-rendering weights): a row whose gate is 0 gets zeros in both outputs, and a 32-row tile whose gates are all 0
 *   reads no texel / table entry.  fp32 throughout, no fp16 operand splits whatever head->flags says (a ReLU bit that moved with the
 *   matrix mode would make a normal depend on a flag); head->flags and head->out_activation are ignored, b2 is not read.
 * One launch per call.  TN_E_CONFIG: a head that is not 2 layers with dims {F, 64, 1}, in_dim F, TN_ENC_NONE, F the field's feature
 *   width; an unknown frame, or an AABB frame without finite hi > lo; K-Planes: channels not 4, 8, 16 or 32 (tn_kplanes_fwd's widths
 *   and 4), n_scales out of range or a missing plane (all three planes of every scale must be present); hash grid: as tn_hashgrid_fwd.
 *   TN_E_SIZE: n < 0, x_stride < 3, a bad plane size.  TN_E_NULL: a null descriptor, head parameter or x, or normals == grad == NULL.
 *   TN_E_ALIGN: planes / table not 16-byte aligned.  frame == NULL is the TN_CONTRACT_NONE frame.  Every argument is checked before the
 *   first HIP call; n == 0 returns TN_OK without a launch (after the descriptor checks).
 * ------------------------------------------------------------------------------------------ */
typedef struct tn_normal_frame {
    int32_t contraction;      /* TN_CONTRACT_* (TN_CONTRACT_NONE included) */
    int32_t reserved;
    float aabb[6];            /* TN_CONTRACT_AABB: lo xyz, hi xyz */
} tn_normal_frame;
int tn_kplanes_normals(const tn_kplanes_desc *f, const float *x, int64_t x_stride, int64_t n, const tn_mlp_desc *head,
                       const tn_normal_frame *frame, const float *gate, float *normals, float *grad, void *stream);
int tn_hashgrid_normals(const tn_hashgrid_desc *f, const float *x, int64_t x_stride, int64_t n, const tn_mlp_desc *head,
                        const tn_normal_frame *frame, const float *gate, float *normals, float *grad, void *stream);
/* Ray normal: N_r = sum_k w_k n_k over the ray's samples (weights [N], normals [N,3]: the weights the forward composited with and
 * tn_*_normals' output), out[r] = N_r / |N_r|, or 0 when the norm is 0 or not finite; rays without samples get 0.  One wave per ray,
 * the lane order and reduction tree of tn_ray_maps' first pass; info must be 8-byte aligned.  n_rays == 0 returns TN_OK without a
 * launch.  No reference call site. */
int tn_ray_normals(const float *weights, const float *normals, const int32_t *info, int64_t n_rays, float *out, void *stream);


/* north star: "the K-Planes bilinear grid sample ... fused into the same launch" as the persistent MLP.  tn_kplanes_fwd +
 * tn_mlp_fwd_stash_pair in ONE launch (reference call chain core.py:239-249 -> models.py:153-163 -> models.py:70-89): every
 * wave gathers the 3 x 3 planes x 4 taps of its 32 samples straight into the first-layer MFMA operand registers of both
 * heads; `feat` [n, 96] is written once for the backward (weight gradient of the first layers, plane scatter) and never read
 * here.  Requirements: 3 scales x 32 channels, all planes present, both heads as in tn_mlp_fwd_stash_pair with in_dim 96.
 * Results are bit-identical to the two-launch sequence.
 * Inference form (round 4): workspace == partner_workspace == NULL -- nothing is stashed and `feat` is not written (it may be
 * NULL; coords must then be 16-byte aligned): gather + sigma + colour of EVERY sample in one launch, for renders in which most
 * samples carry weight (the caller composites with tn_render_rays_fwd; samples with w == 0 contribute exactly 0 either way,
 * core.py:243-249).  The gated sequence tn_kplanes_mlp_fwd -> tn_weights_fwd -> tn_mlp_fwd(row_gate) wins when most tiles are dead. */
int tn_kplanes_mlp_fwd_pair(const tn_kplanes_desc *kdesc, const float *coords, int64_t coord_stride, const tn_mlp_desc *desc,
                            const tn_mlp_desc *partner, const float *aux, int64_t n, float *feat, float *y, float *partner_y,
                            void *workspace, int64_t workspace_bytes, void *partner_workspace, int64_t partner_workspace_bytes,
                            void *stream);

/* Inference form: the gather inside the launch of ONE head without encoding (the sigma head; tn_kplanes_fwd + tn_mlp_fwd):
 * y [n, dims[last]] and the feature rows `feat` [n, 96], which the colour head then reads where the weight is not 0. */
int tn_kplanes_mlp_fwd(const tn_kplanes_desc *kdesc, const float *coords, int64_t coord_stride, const tn_mlp_desc *desc, int64_t n,
                       float *feat, float *y, void *stream);

/* Backward twin: tn_mlp_bwd_pair with the plane scatter (tn_kplanes_bwd) inside the data-gradient chain launch.  d(loss)/d(feat)
 * never leaves the registers of the wave that computed it: each wave scatters its 32 samples' three 32-channel blocks into
 * grad_planes[s][p] (+=, fp32 atomics; NULL entries are skipped) while the other waves of its SIMD run their MFMA chains.
 * `grad_feat` may be NULL (it is only written on request).  `feat` is the row-major [n, 96] feature tensor the forward wrote
 * (the weight-gradient kernels read it).  desc->flags: TN_MLP_STASHED required; TN_MLP_CHAIN_ONLY / TN_MLP_WGRAD_ONLY split the
 * call as in tn_mlp_bwd_pair (CHAIN_ONLY leaves the plane gradients final). */
int tn_kplanes_mlp_bwd_pair(const tn_kplanes_desc *kdesc, const float *coords, int64_t coord_stride,
                            float *const (*grad_planes)[3], const tn_mlp_desc *desc, const tn_mlp_desc *partner,
                            const float *feat, const float *aux, const float *grad_y, const float *partner_grad_y, int64_t n,
                            float *const *grad_weights, float *const *grad_biases, float *const *partner_grad_weights,
                            float *const *partner_grad_biases, float *grad_feat, void *workspace, int64_t workspace_bytes,
                            void *partner_workspace, int64_t partner_workspace_bytes, void *stream);

/* Product stage of the explicit K-Planes decoders (models.py:183-205, exercised by the reference's tests/test_models.py:35-69;
 * train() itself uses the Vanilla decoders, run.py:135-139):
 *   out[n,k] = act(sum_c f[n,c] * basis[n,k,c]),   f [n,C], basis [n,K,C] row-major, 1 <= K <= 4.
 * Opacity decoder: basis = Linear(f) (K = 1), act = TN_ACT_EXP_M1 (exp(v - 1) with the truncated exponential's backward clamp,
 * models.py:42-55); colour decoder: basis = MLP([PE(d), d, f]).view(n, 3, C), act = TN_ACT_SIGMOID.
 * Backward: grad_basis [n,K,C] (may be NULL) is written, grad_f [n,C] is written or (accumulate_f) added to: the sum over k is
 * finished first and added to what grad_f held in one addition. */
int tn_basis_dot_fwd(const float *f, const float *basis, int64_t n, int32_t channels, int32_t n_out, int32_t activation,
                     float *out, void *stream);
int tn_basis_dot_bwd(const float *f, const float *basis, const float *grad_out, int64_t n, int32_t channels, int32_t n_out,
                     int32_t activation, float *grad_f, float *grad_basis, int32_t accumulate_f, void *stream);

/* From (packed [N,7], info [R,2]): ray_ids[i] = ray of sample i, steps[i] = packed[i,6] (contiguous, what tn_weights_*
 * take), dirs[r] = packed[start_r, 3:6] (the ray direction every sample of ray r carries, core.py:182-186; 0 for empty
 * rays).  One launch; feeds tn_dir_encode / TN_ENC_AUX_CAT when the sampler's own by-products are not at hand. */
int tn_ray_aux(const float *packed, const int32_t *info, int64_t n_rays, int32_t *ray_ids, float *steps, float *dirs,
               void *stream);

/* Loss of the harness (run.py:252,259): grad[i] = scale * (scale_dev ? scale_dev[0] : 1) * (rendered[i] - target[i]) and
 * sumsq[0] += sum (rendered - target)^2 (fp64, caller zeroes) over n = 3 * rays elements, one pass. */
int tn_mse_grad(const float *rendered, const float *target, int64_t n, float scale, const float *scale_dev, float *grad,
                double *sumsq, void *stream);
/* a17 + a18 of one batch as ONE launch each way (a wave per ray does both): tn_weights_fwd(_gate) + tn_composite_fwd -> weights
 * and rendered (bit-identical to the two calls; gate may be NULL), and tn_composite_bwd + tn_weights_bwd -> grad_rgbs and
 * grad_sigmas without the grad_weights round trip (reference cuda.cu:3-58 + core.py:256-265 and their autograd). */
int tn_render_rays_fwd(const float *sigmas, const float *steps, const float *rgbs, const int32_t *info, const float *bg,
                       float threshold, float *weights, float *rendered, float *gate, int64_t n_samples, int64_t n_rays,
                       void *stream);
int tn_render_rays_bwd(const float *sigmas, const float *steps, const float *rgbs, const int32_t *info, const float *bg,
                       const float *weights, const float *grad_rendered, float *grad_rgbs, float *grad_sigmas,
                       int64_t n_samples, int64_t n_rays, void *stream);
/* tn_mse_grad with the "Empty iteration" gate applied at the source: grad = 0 when !(gate[0] > 0) (core.py:251-254: the
 * image loss then reaches no parameter); sumsq as in tn_mse_grad. */
int tn_mse_grad_gated(const float *rendered, const float *target, int64_t n, float scale, const float *scale_dev,
                      const float *gate, float *grad, double *sumsq, void *stream);

/* Distortion loss of Mip-NeRF 360 on packed rays.  For ray r with samples k = 0..count-1, weights w_k (tn_weights_fwd /
 * tn_render_rays_fwd: what the forward composited with), normalised positions m_k and widths d_k:
 *   L_r       = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
 *   dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i d_i                  (for every sample, also where w_i == 0)
 * m, d follow from t_values (tn_sample_pack_t: the sample's ray parameter, increasing along a ray) and steps through `warp`,
 * x = (t - near) / range:
 *   TN_DIST_LINEAR     m = x,    d = step / range                        (AABB marcher: near 0, range = the box diagonal)
 *   TN_DIST_UNBOUNDED  m = g(x), d = g'(x) step / range, g(x) = x / 2 for x < 1, 1 - 1 / (2 x) otherwise -- the inverse of the
 *                      unbounded marcher's table (core.py:52), near = its near, range = its uniform_range: m is the marcher's
 *                      uniform parameter in [0, 1).
 * Evaluated in O(count) per ray from fp32 prefix sums with m taken relative to the ray's first sample (the loss is shift
 * invariant; unshifted prefixes cancel).  One wave per ray; info must be 8-byte aligned; no gradient flows to t or step.
 * TN_E_CONFIG for an unknown warp or range <= 0.  No reference call site: the reference has no regulariser on the weights
 * (its only one is the planes' total variation, run.py:254-256). */
enum { TN_DIST_LINEAR = 0, TN_DIST_UNBOUNDED = 1 };
/* loss[r] = L_r (0 for rays without samples); sum (may be NULL; one fp64 device scalar, caller zeroes) += sum_r loss[r] */
int tn_distortion_fwd(const float *weights, const float *t_values, const float *steps, const int32_t *info, int64_t n_rays,
                      int32_t warp, float near, float range, float *loss, double *sum, void *stream);
/* grad_weights[i] = c * (grad_loss ? grad_loss[r] : 1) * dL_r/dw_i for every sample a ray owns,
 * c = scale * (scale_dev ? scale_dev[0] : 1) -- the convention of tn_mse_grad */
int tn_distortion_bwd(const float *weights, const float *t_values, const float *steps, const int32_t *info, int64_t n_rays,
                      int32_t warp, float near, float range, const float *grad_loss, float scale, const float *scale_dev,
                      float *grad_weights, void *stream);
/* tn_render_rays_bwd with grad_weights_extra[i] ([n_samples], e.g. tn_distortion_bwd's output) added to sample i's composite
 * gradient -- (d - gbg) + extra, in that order -- before the weights backward (cuda.cu:49-56, no termination: the extra term
 * also acts on samples with w == 0).  With extra == 0 the outputs are tn_render_rays_bwd's bit for bit. */
int tn_render_rays_bwd_dw(const float *sigmas, const float *steps, const float *rgbs, const int32_t *info, const float *bg,
                          const float *weights, const float *grad_rendered, const float *grad_weights_extra, float *grad_rgbs,
                          float *grad_sigmas, int64_t n_samples, int64_t n_rays, void *stream);
/* Single-scale SSIM (Wang et al. 2004) of two images a, b: fp32 [H, W, C] channel last, 1 <= C <= 4, in the form of the NeRF
 * evaluation scripts: 11 x 11 window w(i,j) = g(i) g(j), g(i) = exp(-(i-5)^2 / (2 * 1.5^2)) / sum (fp64, rounded to fp32 once);
 * one value per window that lies wholly inside the image ("valid", no padding) and per channel -> a map of [(H-10), (W-10), C]:
 *   mu_a = sum w a, var_a = sum w (a - mu_a)^2, cov = sum w (a - mu_a)(b - mu_b), c1 = (0.01 L)^2, c2 = (0.03 L)^2, L = data_range
 *   ssim = (2 mu_a mu_b + c1)(2 cov + c2) / ((mu_a^2 + mu_b^2 + c1)(var_a + var_b + c2))
 * mean[0] (device) = plain mean of the map; `map` may be NULL (not written).  Centred moments in fp32 (two passes over the window
 * from LDS): every map entry within 1e-5 of an fp64 evaluation.  Two launches: tiles of 32 x 8 windows write fp64 partial sums into
 * `workspace` (tn_ssim_workspace_bytes, 8-byte aligned), one workgroup adds them in a fixed order -- no atomics, the same bits on
 * every call, with or without `map`.  TN_E_SIZE: a negative size or a side above 65536; TN_E_CONFIG: H < 11, W < 11, C outside
 * 1..4, data_range not a finite number > 0, workspace too small.  No reference call site: the reference's EvalMetrics.ssim is a
 * placeholder that stays 0 (run.py:56-60). */
int tn_ssim_workspace_bytes(int64_t H, int64_t W, int32_t C, int64_t *bytes);          /* host only */
int tn_ssim(const float *a, const float *b, int64_t H, int64_t W, int32_t C, float data_range, float *map, void *workspace,
            int64_t workspace_bytes, float *mean, void *stream);
/* The harness' batch draw (run.py:225-229, the DataLoader's index_select): rows idx[i] of the [N, 3] ray tables -> out_* [n, 3]
 * in one launch; rgbs / out_rgb may be NULL. */
int tn_gather_rays(const float *rays_o, const float *rays_d, const float *rgbs, const int32_t *idx, int64_t n,
                   float *out_o, float *out_d, float *out_rgb, void *stream);
/* The same draw for a photographed scene, without ray tables: the rays are made from a camera table (one pose, lens and size per
 * image) and the 8-bit colours.  Every pointer of the table is a DEVICE pointer, the struct itself lives on the host.
 * Ray i belongs to flat pixel g = first + stride * (idx ? idx[i] : i) of the split (row-major inside an image, images in table
 * order): a shuffled training block (idx = int32 indices, first = rank, stride = world size for a rank's share), a whole image
 * (idx = NULL, first = pixel_offset[img], stride = 1).  The image is found by binary search in pixel_offset.
 *   xd = (u + 0.5 - cx) / fx, yd = (v + 0.5 - cy) / fy                                  (image axes, y down)
 *   model 0 (pinhole):  (x, y) = (xd, yd)
 *   model 1 (OpenCV):   (x, y) solves xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2),
 *                       rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3 + k4 r2^4, r2 = x^2 + y^2   (Newton from (xd, yd), fixed iteration count)
 *   model 2 (fisheye):  theta_d = |(xd, yd)|, theta solves theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8);
 *                       camera direction (xd s, -yd s, -cos theta), s = sin(theta) / theta_d (1 at the centre)
 *   pinhole / OpenCV camera direction (x, -y, -1): OpenGL camera axes (x right, y up, looking down -z) as the reference's
 *   data.py:52-70, which model 0 reproduces.
 * out_d [n,3] = R dir / |R dir| (R = the 3 x 3 of c2w); out_o [n,3] = the translation column, bit for bit; out_rgb [n,3] =
 * float(byte) / 255, correctly rounded (may be NULL; needs cams->rgb otherwise).  A pixel where the lens model is not invertible and
 * the iteration ends non-finite gets its pinhole direction: the outputs are always finite and of unit length.  An idx entry that
 * leads outside the table (not checkable on the host) reads the nearest pixel of the table; nothing is written outside [0, n).
 * TN_E_SIZE: n < 0, n_img < 1, n_pixels < 1, and -- idx == NULL -- first or first + stride * (n - 1) outside [0, n_pixels);
 * n == 0 returns TN_OK without a launch.  No reference call site: the reference stubs its nerfstudio loader (data.py:162-167). */
typedef struct tn_camera_table {
    const float *c2w;            /* [n_img][12]  rows of the 3 x 4 camera-to-world matrix */
    const float *lens;           /* [n_img][10]  fx fy cx cy k1 k2 k3 k4 p1 p2 (pixels) */
    const int32_t *model;        /* [n_img]      0 pinhole, 1 OpenCV radial-tangential, 2 OpenCV fisheye (TN_LENS_*) */
    const int32_t *size;         /* [n_img][2]   w h */
    const int64_t *pixel_offset; /* [n_img + 1]  first flat pixel of every image; pixel_offset[n_img] = n_pixels */
    const uint8_t *rgb;          /* [n_pixels][3] or NULL (pose-only sets) */
    int64_t n_pixels;            /* host copy of pixel_offset[n_img]: the range checks need it without a device read */
    int32_t n_img, reserved;
} tn_camera_table;
enum { TN_LENS_PINHOLE = 0, TN_LENS_OPENCV = 1, TN_LENS_FISHEYE = 2 };
int tn_camera_rays(const tn_camera_table *cams, const int32_t *idx, int64_t first, int64_t stride, int64_t n,
                   float *out_o, float *out_d, float *out_rgb, void *stream);
/* Coloured point cloud of rendered rays: filter, back-projection and order-preserving compaction of per-ray maps (tn_ray_maps'
 * opacity and depth, the composited colour), all on the device.  fp32 throughout, every fused multiply-add an explicit fmaf:
 *   point   p_c = fmaf(depth_i, d_ic, o_ic), c = x, y, z; d is used as given (the harness' rays are unit length: depth is a distance)
 *   ray i is kept when  opacity_i >= min_opacity (false for NaN)  and  depth_i > 0 and finite  and  all three p_c finite  and --
 *           with a box -- lo_c <= p_c <= hi_c on every axis, faces inclusive
 *   colour  the expected colour given a hit, the background taken out again:
 *           u_c = fmaf(-(1 - opacity_i), bg_c, rgb_ic) / opacity_i  (correctly rounded division), c = min(max(u_c, 0), 1) with
 *           NaN -> 0, byte = (uint8_t)fmaf(c, 255.0f, 0.5f); bg == NULL is bg = (0, 0, 0), bit for bit
 * Output order is ray order: the k-th kept ray writes row k of points, colors and src (src = its ray index).  *count = the number
 * of kept rays whatever `capacity` is; rows k >= capacity are not written and no row at or beyond min(count, capacity) is touched;
 * with capacity == 0 the three output pointers may be NULL (count only).  Three launches on `stream` (per-wave ballots, one
 * workgroup scanning the workgroup counts, ranked stores), no atomics: the same bytes on every call.  `workspace`:
 * tn_points_workspace_bytes(n) = 40 ceil(n / 256) bytes (per workgroup of 256 rays 4 waves x 1 ballot of 8 B, then the workgroup
 * counts of 8 B: the layout of the mesh workspaces below), 8-byte aligned like `count` (TN_E_ALIGN otherwise); contents undefined afterwards.
 * Checked before any launch: TN_E_SIZE for n < 0, capacity < 0 or n >= 2^31 (src is int32); TN_E_CONFIG unless min_opacity > 0
 * (NaN included: the division stays defined); TN_E_NULL for a null required pointer (bg and box are optional; the inputs and the
 * workspace are not read for n == 0).  n == 0 writes *count = 0 and returns TN_OK.  No reference call site: the reference renders
 * images and exports no geometry. */
int tn_points_workspace_bytes(int64_t n, int64_t *bytes);                       /* host only */
int tn_points_compact(const float *rays_o, const float *rays_d,                 /* [n,3] each */
                      const float *rgb,                                         /* [n,3] composited colour */
                      const float *opacity, const float *depth,                 /* [n] */
                      const float *bg,                                          /* [3] or NULL (= 0,0,0) */
                      const float *box,                                         /* [6] lo xyz, hi xyz, device; NULL = no crop */
                      float min_opacity, int64_t n, int64_t capacity,
                      float *points,                                            /* [capacity,3] */
                      uint8_t *colors,                                          /* [capacity,3] */
                      int32_t *src,                                             /* [capacity] ray index of each point */
                      int64_t *count,                                           /* device, 1 value */
                      void *workspace, void *stream);
/* Triangle mesh of a scalar field on a regular grid: naive Surface Nets, all on the device.  fp32 throughout.
 * Grid.  nx x ny x nz cells = dims[0..3) and (nx+1)(ny+1)(nz+1) nodes; node (i,j,k) sits at x_c = fmaf((float)idx_c, h_c, lo_c); dims,
 *   lo[3] and h[3] are HOST arrays.  values holds one float per node, i fastest: index i + (nx+1)(j + (ny+1)k).  Cell (i,j,k) has the
 *   linear index c = i + nx(j + ny k) and the corner nodes (i+dx, j+dy, k+dz).  A node is inside when value >= level (false for NaN).
 *   The kernels are field-agnostic (the harness passes the logarithm of the density, level = log sigma).
 * Vertices.  A cell is active when its 8 corners are neither all inside nor all outside.  Its 12 edges are taken in the order axis
 *   a = 0, 1, 2 and within an axis the offsets (o_b, o_c) = (0,0), (1,0), (0,1), (1,1) on the axes b = (a+1)%3, c = (a+2)%3.  An edge
 *   is crossed when its end nodes differ in insideness; its parameter is t = (level - v0) / (v1 - v0) -- two subtractions and a
 *   correctly rounded division -- clamped to [0,1], v0 the end with 0 on axis a; t = 0.5 when either end value is not finite.  The
 *   edge contributes the point (t on axis a, o_b on b, o_c on c).  u = (the contributions added in that order, starting from 0) /
 *   (float)their number, per component; vertex p_c = fmaf((float)idx_c + u_c, h_c, lo_c).  The k-th active cell in cell order writes
 *   vertex row k.  (Keep |values| <= 1e30: beyond, v1 - v0 overflows and t falls on an end of the edge.)
 * Normal.  g_a = (sum over the 4 edges along a of (v1 - v0) w_b w_c) / h_a with w_b = u_b or 1 - u_b for o_b = 1 or 0, w_c likewise:
 *   the gradient at u of the trilinear interpolant of the cell's own 8 corners.  n = -g / |g| when |g| > 0 and finite, else (0,0,0):
 *   it points from inside (dense) to outside, as tn_kplanes_normals' does.
 * Faces.  Cells in cell order, within a cell the axes a = 0, 1, 2: the edge from node (i,j,k) along a emits a quad when it is crossed
 *   and idx_b >= 1 and idx_c >= 1, so that the 4 cells around it exist (all 4 are active).  Its corners q0..q3 are the vertex ids of
 *   the cells at offsets (-1,-1), (0,-1), (0,0), (-1,0) on (b,c): counter-clockwise seen from +a; when the edge's lower node is
 *   outside the order is reversed to (q3,q2,q1,q0).  The quad becomes the triangles (q0,q1,q2) and (q0,q2,q3): the m-th emitted quad
 *   writes face rows 2m and 2m + 1 of 3 int32 each.  A surface that reaches the box is left open there.
 * Counts.  counts[0] = vertices, counts[1] = triangles, whatever the capacities are; rows at or beyond a capacity are not written
 *   and nothing at or beyond min(count, capacity) is touched; with a capacity of 0 that output may be NULL (both 0: counts only, two
 *   launches).  normals may be NULL.  The ids in `faces` are those of the full mesh, whatever vertex_capacity is.
 * tn_mesh_extract: four launches on `stream` (per-wave ballots + per-workgroup counts, one workgroup per count column scanning it,
 *   ranked vertex stores + the cell -> vertex id map, ranked face stores), no atomics: the same bytes on every call.  `workspace`:
 *   tn_mesh_workspace_bytes bytes, 8-byte aligned like `counts` (TN_E_ALIGN otherwise); with
 *   G = ceil(cells / 256) it is G x 4 waves x 4 ballots of 8 B, then 2 x G workgroup counts of 8 B, then `cells` vertex ids of 4 B,
 *   rounded up to 8 B: 144 G + 8 ceil(cells / 2).  After a call with a capacity > 0 the ids are every cell's vertex id in cell order,
 *   -1 for a cell that is not active; the rest is undefined.  Checked before any launch: TN_E_NULL for null dims / lo / h, then TN_E_SIZE for a
 *   negative dim or capacity or 2^31 cells or more (vertex ids are int32), TN_E_CONFIG for a level that is not finite, TN_E_NULL for
 *   another null required pointer (values and the workspace are not read when a dim is 0: counts = 0, 0 and TN_OK), TN_E_ALIGN.
 * tn_grid_nodes: the positions of nodes first .. first + n in node order, out[t] = node (first + t), by the fmaf above -- a field
 *   sampled there is sampled at the very positions the vertices are built from.  One launch.  TN_E_SIZE unless the range lies inside
 *   the grid's nodes.  No reference call site: the reference renders images and exports no geometry. */
int tn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t *bytes);  /* host only */
int tn_grid_nodes(const float *lo, const float *h, const int32_t *dims,         /* host arrays of 3 */
                  int64_t first, int64_t n, float *out /* [n,3] */, void *stream);
int tn_mesh_extract(const float *values,                                        /* [(nx+1)(ny+1)(nz+1)] device */
                    const int32_t *dims, const float *lo, const float *h,       /* host arrays of 3 */
                    float level, int64_t vertex_capacity, int64_t face_capacity,
                    float *vertices,                                            /* [vertex_capacity,3] */
                    float *normals,                                             /* [vertex_capacity,3] or NULL */
                    int32_t *faces,                                             /* [face_capacity,3] */
                    int64_t *counts,                                            /* device, 2 values */
                    void *workspace, void *stream);
/* Connected components of an indexed triangle mesh, and the filter that keeps the large ones: all on the device, integers throughout.
 * Input.  V vertices and F faces, faces [F,3] int32.  A face is valid when its three indices lie in [0, V); an invalid face takes no
 *   part in anything and is always dropped (tn_mesh_extract with a vertex_capacity below its vertex count hands back fewer vertex rows
 *   than its faces name).  A valid face with repeated indices is an ordinary face.
 * Components.  Two vertices are connected when a valid face names both; label[v] is the smallest vertex id of v's component (the
 *   transitive closure); a vertex in no valid face is its own component, label[v] = v.
 * Face counts.  face_count[r] = the number of valid faces whose vertices carry label r -- 0 for every v with label[v] != v.
 *   stats[0] = the number of components (label[v] == v), stats[1] = those with at least one face, stats[2] = the largest face_count.
 * Filter, with a threshold T >= 0.  Vertex v is kept when face_count[label[v]] >= T; a valid face is kept when its component is.
 *   Kept vertices keep their order: the k-th kept vertex becomes row k of out_vertices / out_normals / out_colors -- its rows copied bit
 *   for bit -- and src[k] is its old id.  Kept faces keep their order, their indices renumbered to the new rows.  normals and colors
 *   (uint8 [V,3]) may be NULL; their outputs are then not written.  counts[0] = kept vertices, counts[1] = kept faces, whatever the
 *   capacities are; rows at or beyond a capacity are not written and nothing at or beyond min(count, capacity) is touched; with a
 *   capacity of 0 that side's outputs may be NULL (both 0: counts only, two launches).  The indices in out_faces are those of the whole
 *   filtered mesh, whatever vertex_capacity is.  T = 0 on a mesh with only valid faces is the identity.  labels and face_counts are
 *   tn_mesh_components' outputs for the same faces (a label outside [0, V) drops its vertex).
 * tn_mesh_components: six launches on `stream`, no host read-back and no loop driven from the host -- labels[v] = v and face_counts = 0;
 *   one pass over the faces, a lock-free union-find on `labels` itself (the larger of two roots is linked under the smaller with
 *   atomicCAS, retried after a lost race, paths shortened with atomicMin on the way up); one pass that makes every labels[v] its
 *   root; integer atomicAdd of the valid faces into face_counts[label], one add per label and wave; per-workgroup partial stats;
 *   one workgroup reducing them in a fixed order.  These atomics choose the route, not the result: the smaller id always wins, so
 *   the final root is the component's minimum whatever the interleaving, and integer min and integer sum do not depend on the order
 *   of their operands -- the same bytes on every call, as for the entry points above that use no atomics.  `workspace`:
 *   tn_mesh_components_workspace_bytes = 24 ceil(V / 256) bytes, 8-byte aligned like `stats`; contents undefined afterwards.
 * tn_mesh_filter: four launches, no atomics (per-wave ballots of kept vertices and faces + per-workgroup counts, one workgroup per
 *   count column scanning it, ranked vertex stores + the old -> new map, ranked face stores through the map).  `workspace`:
 *   tn_mesh_filter_workspace_bytes; with G = ceil(max(V, F) / 256) it is G x 4 waves x 2 ballots of 8 B, then 2 x G workgroup counts of
 *   8 B, then V new ids of 4 B (-1: dropped) rounded up to 8 B: 80 G + 8 ceil(V / 2); 8-byte aligned like `counts`.
 * Checked before any launch, for both: TN_E_SIZE for a negative size or capacity or V or F >= 2^31 (ids are int32); TN_E_CONFIG for
 *   threshold < 0; TN_E_NULL for a null required pointer (stats / counts always; with V > 0 labels, face_counts and the workspace,
 *   faces with F > 0; with vertex_capacity > 0 vertices, out_vertices, src and the output of every attribute that is given; with
 *   face_capacity > 0 out_faces); TN_E_ALIGN.  F == 0 gives every vertex its own component.  V == 0 writes stats / counts of 0 and
 *   returns TN_OK: the inputs and the workspace are not read.  No reference call site: the reference exports no geometry. */
int tn_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t *bytes);   /* host only */
int tn_mesh_components(const int32_t *faces,                                    /* [n_faces,3] device */
                       int64_t n_vertices, int64_t n_faces,
                       int32_t *labels,                                         /* [n_vertices] */
                       int32_t *face_counts,                                    /* [n_vertices] */
                       int64_t *stats,                                          /* device, 3 values */
                       void *workspace, void *stream);
int tn_mesh_filter_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t *bytes);       /* host only */
int tn_mesh_filter(const int32_t *faces, const int32_t *labels, const int32_t *face_counts, int64_t threshold,
                   const float *vertices,                                       /* [n_vertices,3] */
                   const float *normals,                                        /* [n_vertices,3] or NULL */
                   const uint8_t *colors,                                       /* [n_vertices,3] or NULL */
                   int64_t n_vertices, int64_t n_faces, int64_t vertex_capacity, int64_t face_capacity,
                   float *out_vertices, float *out_normals, uint8_t *out_colors,  /* [vertex_capacity,3] each */
                   int32_t *src,                                                /* [vertex_capacity] old id of each kept vertex */
                   int32_t *out_faces,                                          /* [face_capacity,3] */
                   int64_t *counts,                                             /* device, 2 values */
                   void *workspace, void *stream);
/* Fusion of depth maps into a truncated signed distance field (TSDF) on tn_mesh_extract's grid, and the mask that keeps the extractor's
 * faces out of cells no view has observed: all on the device, fp32 throughout, every fused multiply-add an explicit fmaf.
 * Grid.  Exactly tn_mesh_extract's: nx x ny x nz cells = dims[0..3), node (i,j,k) at x_c = fmaf((float)idx_c, h_c, lo_c), nodes stored
 *   i fastest: index i + (nx+1)(j + (ny+1)k); dims, lo[3] and h[3] are HOST arrays.
 * State.  Two floats per node: S, the sum of truncated normalised distances, and W, the number of contributions.  The caller zeroes
 *   both before the first call; every call adds to them.
 * Inputs.  A tn_camera_table (its rgb is not read); depth [n_pixels], a distance along the unit ray as tn_ray_maps and
 *   tn_points_compact use it, in the table's flat pixel order; opacity [n_pixels] or NULL, with min_opacity; trunc > 0; the views
 *   view_first .. view_first + view_count of the table.
 * Update of node x, for the views of the range in ASCENDING order -- "skip" means this view adds nothing:
 *   1 camera frame: p = x - t (t the translation column), q = R^T p, z = -q_z (OpenGL axes: the camera looks down -z); skip unless
 *     z > 0; x' = q_x / z, y' = -q_y / z (image axes, y down); the sums are fmaf(R0c, p_0, fmaf(R1c, p_1, R2c * p_2)), the divisions
 *     correctly rounded
 *   2 lens, the forward model of tn_camera_rays' lenses, r^2 = fmaf(x', x', y' * y'), polynomials by Horner's rule in fmaf:
 *     model 0 (pinhole): (xd, yd) = (x', y')
 *     model 1 (OpenCV):  xd = x' rad + 2 p1 x' y' + p2 (r^2 + 2 x'^2), yd = y' rad + 2 p2 x' y' + p1 (r^2 + 2 y'^2),
 *                        rad = 1 + k1 r^2 + k2 r^4 + k3 r^6 + k4 r^8
 *     model 2 (fisheye): theta = atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
 *                        (xd, yd) = (x', y') theta_d / r, and (x', y') itself at r = 0
 *   3 monotonicity guard (models 1 and 2): skip unless 1 + 3 k1 s + 5 k2 s^2 + 7 k3 s^3 + 9 k4 s^4 > 0, s = r^2 for OpenCV and
 *     theta^2 for the fisheye -- where the radial map has turned back the forward model folds far-off points into the image.  LIMIT:
 *     the guard is local.  It looks at the slope at the point itself: a point beyond a fold where the slope is positive again, and a
 *     fold that the tangential terms make, pass it.
 *   4 pixel: u = fmaf(fx, xd, cx), v = fmaf(fy, yd, cy); pixel i covers [i, i + 1) (centres at +0.5, as in tn_camera_rays): skip
 *     unless 0 <= u < w and 0 <= v < h (false for NaN); g = pixel_offset[view] + floor(v) w + floor(u)
 *   5 depth gate: skip unless D = depth[g] is finite and > 0 and -- with opacity -- opacity[g] >= min_opacity (false for NaN)
 *   6 sdf = D - |p|, |p| = sqrt(fmaf(p_0, p_0, fmaf(p_1, p_1, p_2 * p_2))); skip when sdf < -trunc (the node is hidden behind the
 *     surface in this view); otherwise S += min(sdf / trunc, 1) (a correctly rounded division) and W += 1: free space in front of the
 *     surface votes +1.
 *   The result depends on the inputs alone: no atomics, one lane owns a node, and a range of views integrated in one call gives the
 *   same bytes as the same range split over several calls in order -- the host may feed the views in chunks of any size.
 * Mesh field (host): values = -S / W where W > 0, -1 (empty) elsewhere; level 0; inside is value >= 0.
 * tn_tsdf_integrate: one launch on `stream`, one lane per node, 256 per workgroup, the loop over the views inside the kernel; a
 *   view's table row is read with wave-uniform (scalar) loads.  Checked before the launch: TN_E_NULL for null cams / dims / lo / h,
 *   then TN_E_SIZE for a negative dim or count, a view range outside the table or 2^31 nodes or more; TN_E_CONFIG for a trunc that is
 *   not finite or <= 0; TN_E_NULL for another null required pointer (opacity is optional); TN_E_ALIGN (4 bytes).  view_count == 0 or
 *   a dim of 0: TN_OK without a launch, S and W untouched.
 * tn_tsdf_mask_faces: a cell with any corner at W == 0 must produce no geometry -- otherwise every surface gets a second sheet,
 *   trunc behind it, where the field falls from inside to "empty".  cell_ids [cells] is tn_mesh_extract's cell -> vertex id map (its
 *   workspace from byte 144 G on, after a writing call; -1: no vertex), n_vertices its V, faces [n_faces,3] its faces, edited in
 *   place; observed [n_vertices] is scratch of one byte per vertex.  A memset and two launches: per cell with an id in [0, V),
 *   observed[id] = all 8 corner weights > 0 (a vertex no cell names stays unobserved); per face, (-1, -1, -1) when an index lies
 *   outside [0, V) or names an unobserved vertex.  tn_mesh_filter with a threshold >= 1 then drops those faces and the vertices
 *   they orphan.  Checked before any launch: TN_E_NULL for null dims, TN_E_SIZE for a negative dim or count or 2^31 nodes, vertices
 *   or faces, TN_E_NULL, TN_E_ALIGN (4 bytes); n_faces == 0: TN_OK without a launch.
 * No reference call site: the reference renders images and exports no geometry. */
int tn_tsdf_integrate(const tn_camera_table *cams,
                      const float *depth,                                       /* [n_pixels] device */
                      const float *opacity,                                     /* [n_pixels] or NULL */
                      float min_opacity,
                      const int32_t *dims, const float *lo, const float *h,     /* host arrays of 3 */
                      float trunc, int32_t view_first, int32_t view_count,
                      float *S, float *W,                                       /* [(nx+1)(ny+1)(nz+1)] each */
                      void *stream);
int tn_tsdf_mask_faces(const float *W,                                          /* [(nx+1)(ny+1)(nz+1)] */
                       const int32_t *dims,                                     /* host array of 3 */
                       const int32_t *cell_ids,                                 /* [nx ny nz] */
                       int64_t n_vertices,
                       int32_t *faces,                                          /* [n_faces,3], edited in place */
                       int64_t n_faces,
                       uint8_t *observed,                                       /* [n_vertices] scratch */
                       void *stream);
/* The colour half of the TSDF: the rendered images fused into a colour volume on the same grid, and the volume sampled at mesh
 * vertices.  fp32 throughout, every fused multiply-add an explicit fmaf, the divisions and roots correctly rounded.
 * State.  Four floats per node, in tn_tsdf_integrate's node order: C[node] = (sum w r, sum w g, sum w b, sum w).  The caller zeroes C
 *   before the first call; every call adds to it.
 * Inputs.  tn_tsdf_integrate's (table, depth, opacity or NULL with min_opacity, trunc, a range of views) and rgb [n_pixels][3], the
 *   composited colour of every pixel in the table's flat pixel order, with bg [3] on the device, the colour it was composited over
 *   (NULL: (0, 0, 0)).
 * Update of node x, for the views of the range in ASCENDING order.  Steps 1-5 are exactly tn_tsdf_integrate's (camera frame, lens,
 *   monotonicity guard, pixel g, depth gate and opacity gate).  Then sdf = D - |p| as in step 6, and the view contributes when
 *   -trunc <= sdf <= trunc, with the weight w = 1 - |sdf| / trunc (a correctly rounded division): triangular, zero at both edges of
 *   the band, so nothing jumps there; free space in front of the band votes on geometry and says nothing about colour.  The colour
 *   is the expected colour given a hit, the background taken out again, exactly tn_points_compact's:
 *     u_c = fmaf(-(1 - opacity[g]), bg_c, rgb[g][c]) / opacity[g], clamped to [0, 1] with NaN -> 0
 *   (opacity == NULL: the opacity is 1, u_c = rgb[g][c] clamped).  C[node][c] = fmaf(w, u_c, C[node][c]), C[node][3] += w.
 *   No atomics, one lane owns a node: a range of views in one call and the same range split over calls in order give the same bytes.
 * tn_tsdf_integrate_color: one launch on `stream`, one lane per node, 256 per workgroup, i fastest, the loop over the views inside
 *   the kernel; a view's table row is read with wave-uniform (scalar) loads, the node's four accumulators with one 16-byte load
 *   before the loop and one 16-byte store after it.  Checked before the launch: TN_E_NULL for null cams / dims / lo / h, then
 *   TN_E_SIZE for a negative dim or count, a view range outside the table or 2^31 nodes or more; TN_E_CONFIG for a trunc that is not
 *   finite or <= 0 and -- with an opacity map -- unless min_opacity > 0 (NaN included: the division must stay defined); TN_E_NULL for
 *   a null table pointer (cams->rgb is not read) or null depth / rgb / C (opacity and bg are optional); TN_E_ALIGN: 4 bytes for the
 *   maps and bg, 16 for C.  view_count == 0 or a dim of 0: TN_OK without a launch, C untouched.
 * Sampling.  Per point p and axis c: g_c = (p_c - lo_c) / h_c (a subtraction, then a correctly rounded division), i_c =
 *   min(max((int)floor(g_c), 0), n_c - 1), u_c = min(max(g_c - (float)i_c, 0), 1): a point outside the grid is clamped onto it (i_c is clamped as an integer, so it
 *   stays inside the grid on an axis of more than 2^24 cells too, where (float)(n_c - 1) is no longer exact).  The
 *   8 corners k = dx + 2 dy + 4 dz of cell (i_0, i_1, i_2), in that order, have the trilinear weights t_k = (a_0 a_1) a_2 with a_c =
 *   u_c where the corner's d_c = 1 and 1 - u_c where it is 0.  num_c = sum_k t_k C[k][c] and den = sum_k t_k C[k][3], each a chain
 *   fmaf(t_k, C[k][.], sum) in corner order starting from 0.  out = (num_0 / den, num_1 / den, num_2 / den, den) when den > 0, and
 *   (0, 0, 0, 0) when den is not > 0 or a coordinate of p is not finite.  Corners without colour carry the weight 0: they drop out of
 *   the average instead of darkening it.  The interpolant is continuous across cell faces.  The output is float; bytes are the
 *   caller's business (tn_points_compact's rule: (uint8) fmaf(c, 255, 0.5)).
 * tn_tsdf_sample_colors: one launch, one lane per point.  Checked before the launch: TN_E_NULL for null dims / lo / h; TN_E_SIZE for
 *   a negative dim, 2^31 nodes or more, n < 0 or n >= 2^31; TN_E_NULL for null C / points / out; TN_E_ALIGN: 4 bytes for points, 16
 *   for C and out.  n == 0 or a dim of 0: TN_OK without a launch.
 * No reference call site: the reference renders images and exports no geometry. */
int tn_tsdf_integrate_color(const tn_camera_table *cams,
                            const float *depth,                                 /* [n_pixels] device */
                            const float *opacity,                               /* [n_pixels] or NULL */
                            float min_opacity,
                            const float *rgb,                                   /* [n_pixels][3], the composited colour */
                            const float *bg,                                    /* [3] device, or NULL = (0,0,0) */
                            const int32_t *dims, const float *lo, const float *h,   /* host arrays of 3 */
                            float trunc, int32_t view_first, int32_t view_count,
                            float *C,                                           /* [(nx+1)(ny+1)(nz+1)][4] */
                            void *stream);
int tn_tsdf_sample_colors(const float *C,                                       /* [(nx+1)(ny+1)(nz+1)][4] */
                          const int32_t *dims, const float *lo, const float *h, /* host arrays of 3 */
                          const float *points,                                  /* [n,3] */
                          int64_t n,
                          float *out,                                           /* [n][4]: r, g, b, den */
                          void *stream);
/* Taubin (lambda | mu) smoothing of an indexed triangle mesh, the deterministic vertex adjacency it runs on, and the vertex normals of
 * the smoothed faces: all on the device; the adjacency in integers, passes and normals in fp32.
 * Input.  V vertices and F faces, faces [F,3] int32, as tn_mesh_components takes them.  A face TAKES PART when its three indices lie in
 *   [0, V) and are pairwise different -- so neither a (-1,-1,-1) row of tn_tsdf_mask_faces nor a face with a repeated index does; every
 *   other face is ignored everywhere below.  F' = the participating faces.
 * Adjacency.  Vertex v's ROW holds one pair (a, b) for every participating face that names v: the face's other two corners in its
 *   cyclic order after v -- face (v,a,b), (b,v,a) or (a,b,v) all give (a,b) --, the pairs in ascending face id (a face names v at most
 *   once).  d(v) is the row length.  offsets int32 [V+1] = the exclusive prefix sums of d, in pairs: offsets[V] = 3 F'.  pairs int32
 *   [3F,2] holds the rows back to back; rows at or beyond offsets[V] are not written.  pinned uint8 [V] = 1 when d(v) == 0, or when some
 *   id among the row's 2 d(v) entries does not occur exactly twice among them -- an edge at v with one incident face (a boundary) or
 *   more than two (non-manifold) --, else 0.  stats int64 [3] = (F', the vertices with pinned == 0, the largest d).  The result is a
 *   function of the input alone: the same bytes on every call, whatever the workspace held before.
 * One smoothing pass with the factor f, in [V,3] -> out [V,3], out != in.  A vertex MOVES when d(v) > 0 and, with a pinned array,
 *   pinned[v] == 0.  For one that moves: s = the fp32 sum of the 2 d(v) positions in[a], in[b] of its row in row order (a before b,
 *   from 0), c = s / (2 d(v)) (one correctly rounded division), out[v] = fmaf(f, c - in[v], in[v]).  On a closed manifold mesh this is
 *   the uniform umbrella operator with every neighbour counted twice.  A vertex that does not move has its row copied bit for bit.
 *   Positions that are not finite are not special-cased: they propagate.
 * Taubin smoothing, N iterations: N times a pass with f = lambda followed by a pass with f = mu (the usual 0.5 and -0.53: a low-pass
 *   filter that does not shrink the shape as lambda alone does).  tn_mesh_smooth enqueues the 2 N passes itself -- lambda into
 *   `scratch`, mu into `out`, so the result lands in `out` whatever N is -- and gives bit for bit what chaining tn_mesh_smooth_pass
 *   gives; N == 0 copies `vertices` to `out` (no launch).
 * Vertex normals of the faces.  g(v) = the sum over the row, in row order, of (p[a] - p[v]) x (p[b] - p[v]) -- twice the area-weighted
 *   sum of the face normals; each component accumulated with two fmaf per pair.  Faces are counter-clockwise seen from outside
 *   (tn_mesh_extract's are), so g points from dense to empty as the normals of tn_mesh_extract do.  n(v) = g / |g|,
 *   |g| = sqrtf(fmaf(gx, gx, fmaf(gy, gy, gz gz))); where d(v) == 0 or |g| is 0 or not finite, n(v) is row v of `fallback` [V,3], or 0
 *   without one.
 * tn_mesh_adjacency: a memset and nine launches on `stream`, no host read-back and no loop driven from the host -- integer atomicAdd
 *   of the participating corners into per-vertex degrees; per-workgroup sums and one workgroup scanning them (1024 workgroups a
 *   trip); offsets; the corner ids 3 f + k filled through per-vertex cursors (integer atomicAdd chooses the slot) into the workspace;
 *   one lane per slot ranking its corner id among its row's and storing the pair at that rank; one lane per slot counting its pair's
 *   ids over the row and storing pinned = 1 where a count is not 2; per-workgroup partial stats; one workgroup reducing them in a fixed
 *   order.  The atomics choose the route, not the result: integer sums do not depend on the order of their operands, and a row's
 *   corner ids are distinct, so their ranks are the same permutation wherever the cursors put them.  No floating-point atomics.
 *   The degree is unbounded and every degree is handled; ranking and counting read the row once per slot, so the work is QUADRATIC in
 *   the degree (spread over the row's d lanes) -- a closed manifold Surface Nets mesh stays at or below 12, real ones reach 24 where two sheets touch.  `workspace`:
 *   tn_mesh_adjacency_workspace_bytes; with G = ceil(V / 256) it is 24 G + 8 ceil(V / 2) + 8 ceil(3 F / 2) bytes, 8-byte aligned like
 *   `stats`; contents undefined afterwards.
 * tn_mesh_smooth_pass, tn_mesh_vertex_normals: one launch each, one lane per vertex, no atomics.
 * Checked before any launch: TN_E_SIZE for a negative size, V or F >= 2^31, 3 F >= 2^31 (offsets are int32), iterations < 0;
 *   TN_E_CONFIG for a factor / lambda / mu that is not finite, for `out` aliasing `in` (tn_mesh_smooth: vertices, scratch and out
 *   pairwise); TN_E_NULL for a null required pointer (stats always; with V > 0 offsets, pinned and the workspace, faces and pairs with
 *   F > 0; for the others everything but `pinned` / `fallback`, with V > 0); TN_E_ALIGN (8 bytes for workspace and stats, 4 for the
 *   rest).  V == 0 writes stats of 0 and returns TN_OK without reading anything.  F == 0 pins every vertex: offsets all 0.
 * No reference call site: the reference renders images and exports no geometry. */
int tn_mesh_adjacency_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t *bytes);    /* host only */
int tn_mesh_adjacency(const int32_t *faces,                                     /* [n_faces,3] device */
                      int64_t n_vertices, int64_t n_faces,
                      int32_t *offsets,                                         /* [n_vertices+1] */
                      int32_t *pairs,                                           /* [3 n_faces,2] */
                      uint8_t *pinned,                                          /* [n_vertices] */
                      int64_t *stats,                                           /* device, 3 values */
                      void *workspace, void *stream);
int tn_mesh_smooth_pass(const float *in,                                        /* [n_vertices,3] */
                        const int32_t *offsets, const int32_t *pairs,           /* tn_mesh_adjacency's */
                        const uint8_t *pinned,                                  /* [n_vertices] or NULL: every vertex with a row moves */
                        int64_t n_vertices, float factor,
                        float *out,                                             /* [n_vertices,3], not `in` */
                        void *stream);
int tn_mesh_smooth(const float *vertices, const int32_t *offsets, const int32_t *pairs, const uint8_t *pinned, int64_t n_vertices,
                   int32_t iterations, float lambda, float mu,
                   float *scratch,                                              /* [n_vertices,3] */
                   float *out,                                                  /* [n_vertices,3] */
                   void *stream);
int tn_mesh_vertex_normals(const float *vertices, const int32_t *offsets, const int32_t *pairs, int64_t n_vertices,
                           const float *fallback,                               /* [n_vertices,3] or NULL */
                           float *normals,                                      /* [n_vertices,3] */
                           void *stream);

/* ------------------------------------------------------------------------------------------
 * optimizer step of the harness                      (reference run.py:186,258-260: torch.optim.Adam)
 * One pass per parameter tensor: g' = g + wd*p (coupled L2, as torch), m = b1 m + (1-b1) g',
 * v = b2 v + (1-b2) g'^2, p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps); optionally zeroes g for the
 * next step.  28 B/element instead of torch's multi-kernel foreach path. */
int tn_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, int32_t step, int32_t zero_grad, void *stream);

/* the same update for many tensors in one launch (`items` is a HOST array; all tensors share the step count) */
typedef struct tn_adam_item {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int64_t n;
} tn_adam_item;
int tn_adam_multi(const tn_adam_item *items, int32_t n_items, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, int32_t zero_grad, void *stream);

/* tn_adam_multi for parameters that receive NO gradient in an "Empty iteration" (core.py:251-254: every sample masked ->
 * rgbs / weights become fresh leaves, param.grad stays None and torch.optim.Adam skips the parameter, run.py:258-260,
 * including its per-parameter step count).  `gate` is a device scalar (e.g. max_i w_i of the step): gate > 0 -> `step_dev[0]`
 * (device int32 counter of the updates these tensors have received) is incremented and the update of tn_adam_multi runs with
 * that count; gate <= 0 -> parameters, moments and counter are left untouched (gradients are still zeroed if asked).
 * zero_grad: bit 0 = zero the gradients; bit 1 (round 5) = `step_dev` has a SECOND int32, step_dev[1], which is set to 1 when an updated
 * parameter is not finite (never cleared here).  The kernels' ReLU is v_max_f32: a NaN pre-activation becomes 0 where torch.relu
 * (models.py:7-28) hands it on, so a diverged run would train on silently; the harness turns this flag -- and, for K-Planes planes, the
 * regulariser sums of tn_adam_reg_multi, which any non-finite plane value poisons -- into the NaN loss the reference reports. */
int tn_adam_multi_gated(const tn_adam_item *items, int32_t n_items, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int32_t *step_dev, const float *gate, int32_t zero_grad, void *stream);

/* tn_adam_multi with the K-Planes regulariser folded in (run.py:254-260 in one pass): items with H > 0 are [H,W,C]
 * planes whose TV / L1 gradient (coefficients as in tn_plane_reg_multi, times `upstream`) is added to grad before the
 * update; it is built from the values in `param` while the update goes to `param_out` (a second buffer: the caller swaps
 * them), and sums[3*sum_slot + {0,1,2}] receive the regulariser's three sums (may be NULL).  Items with H == 0 are plain
 * Adam (param_out may equal param). */
typedef struct tn_adam_reg_item {
    const float *param;
    float *param_out, *grad, *exp_avg, *exp_avg_sq;
    int64_t n;
    int32_t H, W, C, sum_slot;
    float cy, cx, cl1;
    /* Sharded optimizer pass (round 5, N > 1 with the recipe's batch split over the ranks): rows [row0, row1) of an [H,W,C] plane are this
     * rank's -- only they are updated (their TV gradient still reads the neighbouring rows of `param`, which every rank holds), only their
     * terms go into `sums`; outside them nothing but the gradient zeroing happens (4 B per element instead of 32).  row1 == 0: every row. */
    int32_t row0, row1, reserved;
} tn_adam_reg_item;
int tn_adam_reg_multi(const tn_adam_reg_item *items, int32_t n_items, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int32_t step, int32_t zero_grad, float upstream, double *sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TINYNERF_HIP_H */
