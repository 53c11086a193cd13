// NeRF volume-rendering weights and per-ray compositing for packed variable-length rays.
//
// Replaces reference src/cuda.cu:3-58 (one *thread* per ray, serial loop, swapped launch
// dims) with one *wavefront* per ray: the 64 lanes load 64 consecutive samples of the ray
// coalesced, alpha = exp(-sigma*delta) is evaluated lane-parallel, and the transmittance is a
// wave-wide multiplicative exclusive scan (6 DPP/shuffle steps) carried across 64-sample
// chunks.  HBM-bound: fwd 12 B/sample (+8 B/ray), bwd 20 B/sample (+8 B/ray).
//
// Semantics kept from the reference:
//  fwd (cuda.cu:19-28): w_k = T_k (1-alpha_k) while T_k > threshold, T_k = prod_{j<k} alpha_j;
//      all samples from the first k with T_k <= threshold on get 0.  The product T*(1-alpha) is
//      formed in fp64 and rounded once, as the reference's double literals do (cuda.cu:25).
//  bwd (cuda.cu:49-56): gs_k = delta_k (T_{k+1} g_k - sum_{j>k} w_j g_j), NO termination.
//
// Every piece that two kernels share -- the wave's ray, the scans and their carries, the composite's sums, its upstream gradient, the
// distortion loss' chunk -- is one helper below, so what the tests hold bit for bit between entry points (`rendered` of the fused and
// the two-launch forward, grad_rgbs of the fused backward and tn_composite_bwd, the opacity of tn_ray_maps and tn_composite_fwd) is
// the same code inlined twice, not two texts kept in step under -ffp-contract=fast.
#include "tn_common.h"
#include <algorithm>

namespace {

constexpr int WAVES_PER_BLOCK = 4;

// ---------------------------------------------------------------------------------------------------------------- the wave's ray
struct WaveRay {
    int64_t ray;
    int start, count;        // its samples: [start, start + count) of the packed arrays
};

__device__ __forceinline__ WaveRay read_ray(const int32_t *__restrict__ info, int64_t ray) {
    const int2 sc = reinterpret_cast<const int2 *>(info)[ray];
    return {ray, sc.x, sc.y};
}

// The ray of this wave in the wave-per-ray grid (launch_waves on ray_blocks(n_rays) blocks).  A kernel takes its ray in three lines,
//     const int64_t ray = wave_ray_index();  if (ray >= n_rays) return;  const WaveRay r = read_ray(info, ray);
// with the exit written in the kernel: a helper that also holds the exit has to hand the ray back through a flag, and that leaves a
// branch diamond in front of the kernel's first loads -- they are issued only after `info` has arrived, +1 us of 22 on
// tn_render_rays_bwd with a training batch, most of whose rays are empty.
__device__ __forceinline__ int64_t wave_ray_index() { return (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); }

// The lane's samples of a ray, k = lane, lane + 64, ...: the order in which every per-ray sum of this file takes them before
// tn::wave_sum's tree (a loop over chunks that adds its lane's sample of each chunk takes them in the same order).
template <class F>
__device__ __forceinline__ void for_lane_samples(const WaveRay &r, int lane, F f) {
    for (int k = lane; k < r.count; k += 64) f(r.start + k);
}

// -------------------------------------------------------------------------------------------------------------------- wave scans
// inclusive scan across the wave
template <class Op>
__device__ __forceinline__ float wave_scan(float v, int lane, Op op) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float u = __shfl_up(v, o, 64);
        if (lane >= o) v = op(v, u);
    }
    return v;
}
__device__ __forceinline__ float wave_scan_mul(float v, int lane) { return wave_scan(v, lane, [](float a, float b) { return a * b; }); }
__device__ __forceinline__ float wave_scan_add(float v, int lane) { return wave_scan(v, lane, [](float a, float b) { return a + b; }); }

// exclusive from inclusive: every lane takes its left neighbour's value, lane 0 the carry of the chunks before
__device__ __forceinline__ float wave_excl(float incl, int lane, float carry) {
    const float e = __shfl_up(incl, 1, 64);
    return lane == 0 ? carry : e;
}

// lane 63's value: of an inclusive scan the chunk's total, the carry into the next chunk
__device__ __forceinline__ float wave_last(float v) { return __shfl(v, 63, 64); }

// ----------------------------------------------------------------------------------------------------------------- the composite
// reference core.py:256-265 -- per-ray segmented sum, deterministic (lane-strided partial sums, then a fixed tree).
struct Composite {
    float r = 0.f, g = 0.f, b = 0.f, o = 0.f;

    __device__ __forceinline__ void add(const float *__restrict__ rgbs, int64_t i, float w) {
        if (w != 0.0f) {     // masked samples carry rgb = 0 in the reference (core.py:248-250)
            const float *c = rgbs + 3 * i;
            r += c[0] * w; g += c[1] * w; b += c[2] * w;
        }
        o += w;
    }

    // (opacity: NULL or the [n_rays] output)
    __device__ __forceinline__ void finish(int lane, int64_t ray, const float *__restrict__ bg, float *__restrict__ rendered,
                                           float *__restrict__ opacity) {
        r = tn::wave_sum(r); g = tn::wave_sum(g); b = tn::wave_sum(b); o = tn::wave_sum(o);
        if (lane == 0) {
            if (bg) { r += bg[0] * (1.f - o); g += bg[1] * (1.f - o); b += bg[2] * (1.f - o); }
            rendered[3 * ray + 0] = r; rendered[3 * ray + 1] = g; rendered[3 * ray + 2] = b;
            if (opacity) opacity[ray] = o;
        }
    }
};

// The composite's upstream gradient: of a ray g = d loss / d rendered and gbg = <bg, g>, of a sample w g to its colour and
// <rgb, g> - <bg, g> to its weight.
struct CompositeGrad {
    float g0, g1, g2, gbg;

    __device__ __forceinline__ void load(const float *__restrict__ grad_rendered, const float *__restrict__ bg, int64_t ray) {
        g0 = grad_rendered[3 * ray]; g1 = grad_rendered[3 * ray + 1]; g2 = grad_rendered[3 * ray + 2];
        gbg = bg ? (bg[0] * g0 + bg[1] * g1 + bg[2] * g2) : 0.f;
    }
    __device__ __forceinline__ void write_rgb(float *__restrict__ grad_rgbs, int64_t i, float w) const {
        grad_rgbs[3 * i] = w * g0; grad_rgbs[3 * i + 1] = w * g1; grad_rgbs[3 * i + 2] = w * g2;
    }
    __device__ __forceinline__ float weight(const float *__restrict__ rgbs, int64_t i, float w) const {
        float d = 0.f;
        if (w != 0.0f) d = rgbs[3 * i] * g0 + rgbs[3 * i + 1] * g1 + rgbs[3 * i + 2] * g2;      // (masked: its colour is not read)
        return d - gbg;
    }
};

// COMP: the ray's composite in the same pass -- Composite on the lane's sample of each chunk, which is composite_fwd_kernel's order, so
// `rendered` is bit-identical to the two-launch form.
template <bool COMP>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void weights_fwd_kernel(
    const float *__restrict__ sigmas, const float *__restrict__ steps, const int32_t *__restrict__ info,
    float threshold, float *__restrict__ weights, int64_t n_rays, float *__restrict__ gate,
    const float *__restrict__ rgbs, const float *__restrict__ bg, float *__restrict__ rendered)
{
    Composite comp;
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    const int start = r.start, count = r.count;
    float carry = 1.0f;          // transmittance entering the chunk
    bool alive = true;           // wave-uniform: no lane has terminated yet
    bool positive = false;       // this lane has written a weight > 0
    for (int base = 0; base < count; base += 64) {
        const int k = base + lane;
        const bool valid = k < count;
        float w = 0.0f;
        if (alive) {
            float a = 1.0f;
            if (valid) a = expf(-sigmas[start + k] * steps[start + k]);
            const float incl = wave_scan_mul(a, lane);
            const float T = carry * wave_excl(incl, lane, 1.0f);
            // the reference's while-loop stops at the FIRST k with !(T_k > threshold)
            const uint64_t dead = __ballot(valid && !(T > threshold));
            const int first_dead = dead ? __builtin_ctzll(dead) : 64;
            if (lane < first_dead) w = (float)((double)T * (1.0 - (double)a));      // fp64 product, rounded once (cuda.cu:25)
            carry = carry * wave_last(incl);
            alive = dead == 0;
        }
        if (valid) weights[start + k] = w;
        positive = positive || w > 0.0f;
        if constexpr (COMP) {
            if (valid) comp.add(rgbs, (int64_t)(start + k), w);
        }
    }
    if constexpr (COMP) comp.finish(lane, r.ray, bg, rendered, nullptr);
    // "Empty iteration" flag of the harness (core.py:251-254): raised by every ray that has a weight > 0.  All writers store the
    // same value, so plain stores do (no atomic: 22 000 waves on one address); once it is up the rest only read it.
    if (gate != nullptr && __ballot(positive) != 0 && lane == 0 && gate[0] == 0.0f) gate[0] = 1.0f;
}

// Single pass over HBM for rays of up to 64*MAXC samples: w*g and alpha stay in registers
// between the reduction (pass 1 of cuda.cu:51) and the prefix sweep (pass 2, cuda.cu:52-56); longer rays are read twice.  Unlike the
// forward, neither path terminates: a sample behind the threshold has w = 0 but still passes its alpha on (cuda.cu:49-56).
// COMP: d loss / d weights is not read but formed here from the composite's upstream gradient (CompositeGrad, as composite_bwd_kernel
// below, grad_rgbs written on the way) -- the same arithmetic, one launch and no grad_weights round trip.
// EXTRA (with COMP): a second gradient of the weights -- the distortion loss', distortion_bwd_kernel below -- is added to the composite's.
template <int MAXC, bool COMP, bool EXTRA>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void weights_bwd_kernel(
    const float *__restrict__ sigmas, const float *__restrict__ steps, const int32_t *__restrict__ info,
    const float *__restrict__ weights, const float *__restrict__ grad_w, float *__restrict__ grad_sigmas,
    int64_t n_rays, const float *__restrict__ rgbs, const float *__restrict__ bg,
    const float *__restrict__ grad_rendered, float *__restrict__ grad_rgbs, const float *__restrict__ extra)
{
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    const int start = r.start, count = r.count;
    CompositeGrad up{};
    if constexpr (COMP) up.load(grad_rendered, bg, r.ray);
    // upstream gradient of sample i's weight (w = its weight)
    auto grad_weight = [&](int64_t i, float w) -> float {
        if constexpr (COMP) {
            up.write_rgb(grad_rgbs, i, w);
            const float d = up.weight(rgbs, i, w);
            if constexpr (EXTRA) return d + extra[i];       // added to the finished d - gbg, not into its sum
            return d;
        } else {
            return grad_w[i];
        }
    };
    // sample k of the ray (k < count): w g, alpha, delta and g
    auto load = [&](int k, float &wg, float &al, float &dl, float &gg) {
        const float w = weights[start + k];
        gg = grad_weight(start + k, w);
        dl = steps[start + k];
        al = expf(-sigmas[start + k] * dl);
        wg = w * gg;
    };
    // one chunk of the sweep: acc = -(sum_{j >= chunk} w_j g_j) and T = the transmittance entering the chunk, both carried on
    float acc = 0.f, T = 1.0f;
    auto sweep = [&](int k, float wg, float al, float dl, float gg) {
        const float ps = wave_scan_add(wg, lane);
        const float pt = wave_scan_mul(al, lane);
        if (k < count) grad_sigmas[start + k] = dl * ((acc + ps) + (T * pt) * gg);
        acc += wave_last(ps);
        T *= wave_last(pt);
    };
    float total = 0.0f;
    if (count <= 64 * MAXC) {
        float wg[MAXC], al[MAXC], dl[MAXC], gg[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int k = c * 64 + lane;
            wg[c] = 0.f; al[c] = 1.f; dl[c] = 0.f; gg[c] = 0.f;         // behind the ray's end: the scans' identities
            if (c * 64 < count && k < count) load(k, wg[c], al[c], dl[c], gg[c]);
            total += wg[c];
        }
        acc = -tn::wave_sum(total);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c * 64 < count) sweep(c * 64 + lane, wg[c], al[c], dl[c], gg[c]);
    } else {
        for_lane_samples(r, lane, [&](int64_t i) { const float w = weights[i]; total += w * grad_weight(i, w); });
        acc = -tn::wave_sum(total);
        for (int base = 0; base < count; base += 64) {
            const int k = base + lane;
            float wg = 0.f, al = 1.f, dl = 0.f, gg = 0.f;
            if (k < count) load(k, wg, al, dl, gg);
            sweep(k, wg, al, dl, gg);
        }
    }
}

__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void composite_fwd_kernel(
    const float *__restrict__ rgbs, const float *__restrict__ weights, const int32_t *__restrict__ info,
    const float *__restrict__ bg, float *__restrict__ rendered, float *__restrict__ opacity, int64_t n_rays)
{
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    Composite comp;
    for_lane_samples(r, lane, [&](int64_t i) { comp.add(rgbs, i, weights[i]); });
    comp.finish(lane, r.ray, bg, rendered, opacity);
}

// grad_rgbs, grad_weights: either may be NULL (a caller that needs one of them); the fused weights_bwd_kernel<COMP> writes the first
// and consumes the second.
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void composite_bwd_kernel(
    const float *__restrict__ rgbs, const float *__restrict__ weights, const int32_t *__restrict__ info,
    const float *__restrict__ bg, const float *__restrict__ grad_rendered, float *__restrict__ grad_rgbs,
    float *__restrict__ grad_weights, int64_t n_rays)
{
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    CompositeGrad up;
    up.load(grad_rendered, bg, r.ray);
    for_lane_samples(r, lane, [&](int64_t i) {
        const float w = weights[i];
        if (grad_rgbs) up.write_rgb(grad_rgbs, i, w);
        if (grad_weights) grad_weights[i] = up.weight(rgbs, i, w);
    });
}

// d/d rendered of  c * sum (rendered - target)^2  and the sum itself (fp64 accumulator), one pass (run.py:252,259)
__global__ __launch_bounds__(256) void mse_grad_kernel(const float *__restrict__ r, const float *__restrict__ t, int64_t n, float cg,
                                                       const float *__restrict__ cg_dev, float *__restrict__ grad, double *__restrict__ sumsq,
                                                       const float *__restrict__ gate)
{
    float c = cg_dev ? cg * cg_dev[0] : cg;
    if (gate != nullptr && !(gate[0] > 0.0f)) c = 0.0f;     // "Empty iteration": the image loss reaches no parameter
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = r[i] - t[i];
        grad[i] = d * c;
        s = fmaf(d, d, s);
    }
    double ds = s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ds;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sumsq, red[0] + red[1] + red[2] + red[3]);
}

// per-sample ray index, contiguous step sizes and per-ray direction out of (packed, info): what the per-ray colour-head
// table and the weights kernels index (one launch instead of repeat_interleave + gathers + copies)
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void ray_aux_kernel(const float *__restrict__ packed, const int32_t *__restrict__ info,
                                                                       int64_t n_rays, int32_t *__restrict__ ray_ids,
                                                                       float *__restrict__ steps, float *__restrict__ dirs)
{
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    if (lane < 3) dirs[3 * r.ray + lane] = r.count > 0 ? packed[7 * (int64_t)r.start + 3 + lane] : 0.0f;
    for_lane_samples(r, lane, [&](int64_t i) {
        ray_ids[i] = (int32_t)r.ray;
        steps[i] = packed[7 * i + 6];
    });
}

// Per-ray opacity, expected depth and median depth from the weights and the sample distances t (tn_sample_pack_t).
// Pass 1: opacity = sum w and sum w t over for_lane_samples and tn::wave_sum -- Composite's `o` term by term, so the opacity is the
// bits composite_fwd_kernel writes.  Pass 2 (median only): inclusive prefix of w over chunks of 64 (wave_scan_add + the carry),
// stopped at the first chunk in which it reaches opacity / 2 -- on a ray that terminated early that is one of its first chunks.
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void ray_maps_kernel(
    const float *__restrict__ weights, const float *__restrict__ t_values, const int32_t *__restrict__ info, int64_t n_rays,
    float *__restrict__ opacity, float *__restrict__ depth, float *__restrict__ median_depth)
{
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    float o = 0.f, wt = 0.f;
    for_lane_samples(r, lane, [&](int64_t i) {
        const float w = weights[i];
        o += w;
        if (depth) wt += w * t_values[i];
    });
    o = tn::wave_sum(o);
    if (depth) wt = tn::wave_sum(wt);
    float med = 0.f;
    if (median_depth && o > 0.f) {
        const float half = 0.5f * o;
        float carry = 0.f;
        int found = -1;
        for (int base = 0; base < r.count; base += 64) {
            const int k = base + lane;
            const float p = carry + wave_scan_add(k < r.count ? weights[r.start + k] : 0.f, lane);
            const uint64_t hit = __ballot(k < r.count && p >= half);
            if (hit) { found = base + __builtin_ctzll(hit); break; }
            carry = wave_last(p);
        }
        // (a prefix that never reaches the mark -- fp32 rounding of a sum whose order differs from the opacity's -- ends on the last sample)
        med = t_values[r.start + (found >= 0 ? found : r.count - 1)];
    }
    if (lane == 0) {
        if (opacity) opacity[r.ray] = o;
        if (depth) depth[r.ray] = o > 0.f ? wt / o : 0.f;
        if (median_depth) median_depth[r.ray] = med;
    }
}

// Ray normal: N = sum w_k n_k in the order of ray_maps_kernel's first pass (for_lane_samples, tn::wave_sum), then N / |N| taken
// relative to the largest component (no overflow or underflow of the squares); 0 when |N| is 0 or not finite.
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void ray_normals_kernel(
    const float *__restrict__ weights, const float *__restrict__ normals, const int32_t *__restrict__ info, int64_t n_rays,
    float *__restrict__ out)
{
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    float a = 0.f, b = 0.f, c = 0.f;
    for_lane_samples(r, lane, [&](int64_t i) {
        const float w = weights[i];
        a += w * normals[3 * i]; b += w * normals[3 * i + 1]; c += w * normals[3 * i + 2];
    });
    a = tn::wave_sum(a); b = tn::wave_sum(b); c = tn::wave_sum(c);
    if (lane == 0) {
        const float mx = fmaxf(fmaxf(fabsf(a), fabsf(b)), fabsf(c));
        const bool ok = mx > 0.f && mx < __builtin_inff() && a == a && b == b && c == c;
        const float u = a / mx, v = b / mx, w = c / mx;
        const float len = sqrtf(u * u + v * v + w * w);
        out[3 * r.ray] = ok ? u / len : 0.f; out[3 * r.ray + 1] = ok ? v / len : 0.f; out[3 * r.ray + 2] = ok ? w / len : 0.f;
    }
}

// Distortion loss of Mip-NeRF 360 on packed rays.  For ray r with weights w_k, normalised positions m_k and widths d_k
//   L = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
// m increases along a ray, so with the exclusive prefixes W_<i = sum_{j<i} w_j and M_<i = sum_{j<i} w_j m_j
//   L = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 d_i
//   dL/dw_i = 2 (m_i W_<i - M_<i) + 2 (M_>i - m_i W_>i) + (2/3) w_i d_i.
// m, d come from the sample's ray parameter t and its step through the warp x = (t - near) / range: m = x, d = step / range
// (TN_DIST_LINEAR) or m = g(x), d = g'(x) step / range with g(x) = x / 2 below 1 and 1 - 1 / (2 x) from there on (TN_DIST_UNBOUNDED:
// the inverse of the unbounded marcher's table).  m is taken RELATIVE TO THE RAY'S FIRST SAMPLE (the loss is shift invariant):
// m W - M cancels, and fp32 prefixes of unshifted positions lose the loss at t ~ 50.  The difference g(x) - g(x_0) is formed in
// fp64 and rounded once -- behind the knee g flattens like 1 / x^2 and neighbouring fp32 values of g(x) coincide; the prefix
// sums are fp32 wave scans (wave_scan_add) with carries across 64-sample chunks, a wave per ray like every kernel here.
struct DistWarp {
    int32_t warp;
    float inv_range_f;
    double near, inv_range;
};

__device__ __forceinline__ double dist_g(int32_t warp, double x) {
    return warp == TN_DIST_UNBOUNDED ? (x < 1.0 ? 0.5 * x : 1.0 - 0.5 / x) : x;
}

// one sample: m (relative to the ray's first sample, g0 = g(x_0)) and the width d
__device__ __forceinline__ void dist_sample(const DistWarp &p, double g0, float t, float step, float &m, float &d) {
    const double x = ((double)t - p.near) * p.inv_range;
    m = (float)(dist_g(p.warp, x) - g0);
    d = step * p.inv_range_f;
    if (p.warp == TN_DIST_UNBOUNDED) {
        const float xf = (float)x;
        d = x < 1.0 ? 0.5f * d : d / (2.0f * xf * xf);
    }
}

// One chunk of 64 samples of a ray: the lane's sample (w, m, d; zeros behind the ray's end) and the prefixes of w and w m over the
// ray so far, inclusive (pw, pm) and exclusive (ew, em).
struct DistChunk {
    float w, m, d, pw, pm, ew, em;
};

// A ray of the distortion kernels, walked in chunks of 64 from its first sample on by chunk().
struct DistRay {
    const float *__restrict__ weights, *__restrict__ t_values, *__restrict__ steps;
    const DistWarp &p;
    int start, count;
    double g0;               // g(x_0) of the ray's first sample
    float cw = 0.f, cm = 0.f;        // carries: the prefixes of w and w m over the chunks walked so far; behind the last chunk the ray's totals

    __device__ __forceinline__ DistRay(const float *__restrict__ weights, const float *__restrict__ t_values, const float *__restrict__ steps,
                                       const DistWarp &p, const WaveRay &r)
        : weights(weights), t_values(t_values), steps(steps), p(p), start(r.start), count(r.count),
          g0(r.count > 0 ? dist_g(p.warp, ((double)t_values[r.start] - p.near) * p.inv_range) : 0.0) {}

    // back to the first sample, for a second walk
    __device__ __forceinline__ void restart() { cw = 0.f; cm = 0.f; }

    // The chunk in which sample k is this lane's; the carries move on behind it.  (A caller that keeps only the inclusive prefixes
    // -- the register path of distortion_bwd_kernel -- leaves ew, em unused and the compiler drops their shuffles.)
    __device__ __forceinline__ DistChunk chunk(int k, int lane) {
        DistChunk c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (k < count) {
            c.w = weights[start + k];
            dist_sample(p, g0, t_values[start + k], steps[start + k], c.m, c.d);
        }
        c.pw = cw + wave_scan_add(c.w, lane);
        c.pm = cm + wave_scan_add(c.w * c.m, lane);
        c.ew = wave_excl(c.pw, lane, cw);
        c.em = wave_excl(c.pm, lane, cm);
        cw = wave_last(c.pw);
        cm = wave_last(c.pm);
        return c;
    }
};

// Waves stride over the rays so that a block adds to `sum` once (22 000 rays would otherwise queue on one address).
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void distortion_fwd_kernel(
    const float *__restrict__ weights, const float *__restrict__ t_values, const float *__restrict__ steps, const int32_t *__restrict__ info,
    int64_t n_rays, DistWarp p, float *__restrict__ loss, double *__restrict__ sum)
{
    const int lane = tn::lane_id();
    const int wave = threadIdx.x >> 6;
    double wave_total = 0.0;
    for (int64_t ray = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave; ray < n_rays; ray += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        DistRay dr(weights, t_values, steps, p, read_ray(info, ray));
        float acc = 0.f;
        for (int base = 0; base < dr.count; base += 64) {
            const DistChunk c = dr.chunk(base + lane, lane);
            acc += 2.0f * c.w * (c.m * c.ew - c.em) + (1.0f / 3.0f) * (c.w * c.w) * c.d;
        }
        acc = tn::wave_sum(acc);
        if (lane == 0) loss[ray] = acc;
        wave_total += (double)acc;
    }
    if (sum != nullptr) {
        __shared__ double red[WAVES_PER_BLOCK];
        if (lane == 0) red[wave] = wave_total;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = red[0];
#pragma unroll
            for (int i = 1; i < WAVES_PER_BLOCK; ++i) s += red[i];
            atomicAdd(sum, s);
        }
    }
}

// Rays of up to 64*MAXC samples: m, w d and both prefixes stay in registers between the totals pass and the sweep (the two paths of
// weights_bwd_kernel); longer rays are read twice.  The totals are the last prefixes themselves, so W_>i and M_>i of a ray's last
// sample are exactly 0.
template <int MAXC>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void distortion_bwd_kernel(
    const float *__restrict__ weights, const float *__restrict__ t_values, const float *__restrict__ steps, const int32_t *__restrict__ info,
    int64_t n_rays, DistWarp p, const float *__restrict__ grad_loss, float scale, const float *__restrict__ scale_dev,
    float *__restrict__ grad_weights)
{
    const int lane = tn::lane_id();
    const int64_t ray = wave_ray_index();
    if (ray >= n_rays) return;
    const WaveRay r = read_ray(info, ray);
    const int start = r.start, count = r.count;
    if (count <= 0) return;
    float c = scale_dev ? scale * scale_dev[0] : scale;
    if (grad_loss) c *= grad_loss[r.ray];
    DistRay dr(weights, t_values, steps, p, r);
    // d L / d w of a sample from its prefixes (ew, em: exclusive, pw, pm: inclusive) and the ray's totals
    auto grad = [&](float m, float wd, float ew, float em, float pw, float pm, float tw, float tm) -> float {
        return c * (2.0f * ((m * ew - em) + ((tm - pm) - m * (tw - pw))) + (2.0f / 3.0f) * wd);
    };
    if (count <= 64 * MAXC) {
        float ms[MAXC], wd[MAXC], pw[MAXC], pm[MAXC];
#pragma unroll
        for (int ch = 0; ch < MAXC; ++ch) {
            ms[ch] = 0.f; wd[ch] = 0.f; pw[ch] = dr.cw; pm[ch] = dr.cm;
            if (ch * 64 < count) {
                const DistChunk k = dr.chunk(ch * 64 + lane, lane);
                ms[ch] = k.m; wd[ch] = k.w * k.d; pw[ch] = k.pw; pm[ch] = k.pm;
            }
        }
        const float tw = dr.cw, tm = dr.cm;          // every chunk walked: the totals
        float cw = 0.f, cm = 0.f;
#pragma unroll
        for (int ch = 0; ch < MAXC; ++ch) {
            if (ch * 64 < count) {
                const int k = ch * 64 + lane;
                // (the exclusive prefixes are formed again: kept from the first pass they would be 2 MAXC more registers)
                if (k < count) grad_weights[start + k] = grad(ms[ch], wd[ch], wave_excl(pw[ch], lane, cw), wave_excl(pm[ch], lane, cm),
                                                              pw[ch], pm[ch], tw, tm);
                cw = wave_last(pw[ch]);
                cm = wave_last(pm[ch]);
            }
        }
    } else {
        float tw = 0.f, tm = 0.f;
        for (int pass = 0; pass < 2; ++pass) {
            dr.restart();
            for (int base = 0; base < count; base += 64) {
                const int k = base + lane;
                const DistChunk s = dr.chunk(k, lane);
                if (pass == 1 && k < count) grad_weights[start + k] = grad(s.m, s.w * s.d, s.ew, s.em, s.pw, s.pm, tw, tm);
            }
            tw = dr.cw; tm = dr.cm;          // the first walk's totals, for the second
        }
    }
}

// rows idx[i] of three [N, 3] ray tables in one launch (the harness' batch draw: origins, directions, target colours)
__global__ __launch_bounds__(256) void gather_rays_kernel(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c,
                                                          const int32_t *__restrict__ idx, int64_t n, float *__restrict__ oa,
                                                          float *__restrict__ ob, float *__restrict__ oc)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // element of the [n, 3] outputs
    if (e >= 3 * n) return;
    const int64_t r = e / 3;
    const int64_t src = (int64_t)idx[r] * 3 + (e - 3 * r);
    oa[e] = a[src];
    ob[e] = b[src];
    if (c != nullptr) oc[e] = c[src];
}

// ---------------------------------------------------------------------------------------------------------------------- host side
inline unsigned ray_blocks(int64_t n_rays) { return (unsigned)((n_rays + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK); }

// the launch of every wave-per-ray kernel: `blocks` blocks of WAVES_PER_BLOCK waves on the caller's stream
template <class K, class... A>
int launch_waves(const char *label, K kernel, unsigned blocks, void *stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(WAVES_PER_BLOCK * 64), 0, (hipStream_t)stream, args...);
    return tn::check_launch(label);
}

// tn::fail of a function that serves two entry points: `fn` is the name of the one that was called
inline int fail_fn(const char *fn, int code, const char *what) {
    tn::set_error("%s: %s", fn, what);
    return code;
}

// tn_weights_fwd (gate NULL) / tn_weights_fwd_gate (gated: the gate is required)
int weights_fwd(const char *fn, const float *sigmas, const float *steps, const int32_t *info, float threshold, float *weights, float *gate,
                bool gated, int64_t n_samples, int64_t n_rays, void *stream)
{
    if (n_samples < 0 || n_rays < 0) return fail_fn(fn, TN_E_SIZE, "negative size");
    if (n_rays == 0 || n_samples == 0) return TN_OK;
    if (!(sigmas && steps && info && weights && (gate || !gated))) return fail_fn(fn, TN_E_NULL, "null pointer");
    if ((uintptr_t)info & 7) return fail_fn(fn, TN_E_ALIGN, "info must be 8-byte aligned");
    return launch_waves("weights_fwd_kernel", weights_fwd_kernel<false>, ray_blocks(n_rays), stream, sigmas, steps, info, threshold, weights,
                        n_rays, gate, nullptr, nullptr, nullptr);
}

// tn_render_rays_bwd (extra NULL) / tn_render_rays_bwd_dw (with_extra: a second gradient of the weights is required and added)
int render_rays_bwd(const char *fn, const float *sigmas, const float *steps, const float *rgbs, const int32_t *info, const float *bg,
                    const float *weights, const float *grad_rendered, const float *extra, bool with_extra, float *grad_rgbs,
                    float *grad_sigmas, int64_t n_samples, int64_t n_rays, void *stream)
{
    if (n_samples < 0 || n_rays < 0) return fail_fn(fn, TN_E_SIZE, "negative size");
    if (n_rays == 0 || n_samples == 0) return TN_OK;
    if (!(sigmas && steps && rgbs && info && weights && grad_rendered && (extra || !with_extra) && grad_rgbs && grad_sigmas))
        return fail_fn(fn, TN_E_NULL, "null pointer");
    if ((uintptr_t)info & 7) return fail_fn(fn, TN_E_ALIGN, "info must be 8-byte aligned");
    return launch_waves(with_extra ? "weights_bwd_kernel(composite, extra)" : "weights_bwd_kernel(composite)",
                        with_extra ? weights_bwd_kernel<16, true, true> : weights_bwd_kernel<16, true, false>, ray_blocks(n_rays), stream,
                        sigmas, steps, info, weights, nullptr, grad_sigmas, n_rays, rgbs, bg, grad_rendered, grad_rgbs, extra);
}

// tn_mse_grad (gate NULL) / tn_mse_grad_gated (gated: the gate is required)
int mse_grad(const char *fn, const float *rendered, const float *target, int64_t n, float scale, const float *scale_dev, const float *gate,
             bool gated, float *grad, double *sumsq, void *stream)
{
    if (n < 0) return fail_fn(fn, TN_E_SIZE, "negative size");
    if (n == 0) return TN_OK;
    if (!(rendered && target && grad && sumsq && (gate || !gated))) return fail_fn(fn, TN_E_NULL, "null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 512);
    hipLaunchKernelGGL(mse_grad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rendered, target, n, scale, scale_dev, grad, sumsq, gate);
    return tn::check_launch("mse_grad_kernel");
}

// tn_distortion_fwd / _bwd: the checks they share (out: the output each requires), the warp, then `launch(p)`
template <class Launch>
int distortion(const char *fn, const float *weights, const float *t_values, const float *steps, const int32_t *info, const void *out,
               int64_t n_rays, int32_t warp, float near, float range, Launch launch)
{
    if (n_rays < 0) return fail_fn(fn, TN_E_SIZE, "negative size");
    if (n_rays == 0) return TN_OK;
    if (!(weights && t_values && steps && info && out)) return fail_fn(fn, TN_E_NULL, "null pointer");
    if (!((warp == TN_DIST_LINEAR || warp == TN_DIST_UNBOUNDED) && range > 0.0f)) return fail_fn(fn, TN_E_CONFIG, "unknown warp or range <= 0");
    if ((uintptr_t)info & 7) return fail_fn(fn, TN_E_ALIGN, "info must be 8-byte aligned");
    DistWarp p;
    p.warp = warp;
    p.near = (double)near;
    p.inv_range = 1.0 / (double)range;
    p.inv_range_f = (float)p.inv_range;
    return launch(p);
}

}  // namespace

extern "C" int tn_ray_maps(const float *weights, const float *t_values, const int32_t *info, int64_t n_rays, float *opacity,
                           float *depth, float *median_depth, void *stream)
{
    TN_REQUIRE(n_rays >= 0, TN_E_SIZE, "tn_ray_maps: negative size");
    if (n_rays == 0 || !(opacity || depth || median_depth)) return TN_OK;
    TN_REQUIRE(weights && info && (t_values || !(depth || median_depth)), TN_E_NULL, "tn_ray_maps: null pointer");
    TN_REQUIRE(((uintptr_t)info & 7) == 0, TN_E_ALIGN, "tn_ray_maps: info must be 8-byte aligned");
    return launch_waves("ray_maps_kernel", ray_maps_kernel, ray_blocks(n_rays), stream, weights, t_values, info, n_rays, opacity, depth,
                        median_depth);
}

extern "C" int tn_ray_normals(const float *weights, const float *normals, const int32_t *info, int64_t n_rays, float *out, void *stream)
{
    TN_REQUIRE(n_rays >= 0, TN_E_SIZE, "tn_ray_normals: negative size");
    if (n_rays == 0) return TN_OK;
    TN_REQUIRE(weights && normals && info && out, TN_E_NULL, "tn_ray_normals: null pointer");
    TN_REQUIRE(((uintptr_t)info & 7) == 0, TN_E_ALIGN, "tn_ray_normals: info must be 8-byte aligned");
    return launch_waves("ray_normals_kernel", ray_normals_kernel, ray_blocks(n_rays), stream, weights, normals, info, n_rays, out);
}

extern "C" int tn_weights_fwd(const float *sigmas, const float *steps, const int32_t *info, float threshold,
                              float *weights, int64_t n_samples, int64_t n_rays, void *stream)
{
    return weights_fwd("tn_weights_fwd", sigmas, steps, info, threshold, weights, nullptr, false, n_samples, n_rays, stream);
}

extern "C" int tn_weights_fwd_gate(const float *sigmas, const float *steps, const int32_t *info, float threshold, float *weights,
                                   float *gate, int64_t n_samples, int64_t n_rays, void *stream)
{
    return weights_fwd("tn_weights_fwd_gate", sigmas, steps, info, threshold, weights, gate, true, n_samples, n_rays, stream);
}

extern "C" int tn_render_rays_fwd(const float *sigmas, const float *steps, const float *rgbs, const int32_t *info, const float *bg,
                                  float threshold, float *weights, float *rendered, float *gate, int64_t n_samples, int64_t n_rays,
                                  void *stream)
{
    TN_REQUIRE(n_samples >= 0 && n_rays >= 0, TN_E_SIZE, "tn_render_rays_fwd: negative size");
    if (n_rays == 0) return TN_OK;
    TN_REQUIRE(info && weights && rendered && (n_samples == 0 || (sigmas && steps && rgbs)), TN_E_NULL, "tn_render_rays_fwd: null pointer");
    TN_REQUIRE(((uintptr_t)info & 7) == 0, TN_E_ALIGN, "tn_render_rays_fwd: info must be 8-byte aligned");
    return launch_waves("weights_fwd_kernel(composite)", weights_fwd_kernel<true>, ray_blocks(n_rays), stream, sigmas, steps, info, threshold,
                        weights, n_rays, gate, rgbs, bg, rendered);
}

extern "C" int tn_render_rays_bwd(const float *sigmas, const float *steps, const float *rgbs, const int32_t *info, const float *bg,
                                  const float *weights, const float *grad_rendered, float *grad_rgbs, float *grad_sigmas,
                                  int64_t n_samples, int64_t n_rays, void *stream)
{
    return render_rays_bwd("tn_render_rays_bwd", sigmas, steps, rgbs, info, bg, weights, grad_rendered, nullptr, false, grad_rgbs, grad_sigmas,
                           n_samples, n_rays, stream);
}

extern "C" int tn_render_rays_bwd_dw(const float *sigmas, const float *steps, const float *rgbs, const int32_t *info, const float *bg,
                                     const float *weights, const float *grad_rendered, const float *grad_weights_extra, float *grad_rgbs,
                                     float *grad_sigmas, int64_t n_samples, int64_t n_rays, void *stream)
{
    return render_rays_bwd("tn_render_rays_bwd_dw", sigmas, steps, rgbs, info, bg, weights, grad_rendered, grad_weights_extra, true, grad_rgbs,
                           grad_sigmas, n_samples, n_rays, stream);
}

extern "C" int tn_distortion_fwd(const float *weights, const float *t_values, const float *steps, const int32_t *info, int64_t n_rays,
                                 int32_t warp, float near, float range, float *loss, double *sum, void *stream)
{
    return distortion("tn_distortion_fwd", weights, t_values, steps, info, loss, n_rays, warp, near, range, [&](const DistWarp &p) {
        return launch_waves("distortion_fwd_kernel", distortion_fwd_kernel, std::min(ray_blocks(n_rays), 2048u), stream, weights, t_values,
                            steps, info, n_rays, p, loss, sum);
    });
}

extern "C" int tn_distortion_bwd(const float *weights, const float *t_values, const float *steps, const int32_t *info, int64_t n_rays,
                                 int32_t warp, float near, float range, const float *grad_loss, float scale, const float *scale_dev,
                                 float *grad_weights, void *stream)
{
    return distortion("tn_distortion_bwd", weights, t_values, steps, info, grad_weights, n_rays, warp, near, range, [&](const DistWarp &p) {
        return launch_waves("distortion_bwd_kernel", distortion_bwd_kernel<8>, ray_blocks(n_rays), stream, weights, t_values, steps, info,
                            n_rays, p, grad_loss, scale, scale_dev, grad_weights);
    });
}

extern "C" int tn_weights_bwd(const float *sigmas, const float *steps, const int32_t *info, const float *weights,
                              const float *grad_weights, float *grad_sigmas, int64_t n_samples, int64_t n_rays, void *stream)
{
    TN_REQUIRE(n_samples >= 0 && n_rays >= 0, TN_E_SIZE, "tn_weights_bwd: negative size");
    if (n_rays == 0 || n_samples == 0) return TN_OK;
    TN_REQUIRE(sigmas && steps && info && weights && grad_weights && grad_sigmas, TN_E_NULL, "tn_weights_bwd: null pointer");
    TN_REQUIRE(((uintptr_t)info & 7) == 0, TN_E_ALIGN, "tn_weights_bwd: info must be 8-byte aligned");
    return launch_waves("weights_bwd_kernel", weights_bwd_kernel<16, false, false>, ray_blocks(n_rays), stream, sigmas, steps, info, weights,
                        grad_weights, grad_sigmas, n_rays, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int tn_composite_fwd(const float *rgbs, const float *weights, const int32_t *info, const float *bg,
                                float *rendered, float *opacity, int64_t n_samples, int64_t n_rays, void *stream)
{
    TN_REQUIRE(n_samples >= 0 && n_rays >= 0, TN_E_SIZE, "tn_composite_fwd: negative size");
    if (n_rays == 0) return TN_OK;
    TN_REQUIRE(info && rendered && (n_samples == 0 || (rgbs && weights)), TN_E_NULL, "tn_composite_fwd: null pointer");
    TN_REQUIRE(((uintptr_t)info & 7) == 0, TN_E_ALIGN, "tn_composite_fwd: info must be 8-byte aligned");
    return launch_waves("composite_fwd_kernel", composite_fwd_kernel, ray_blocks(n_rays), stream, rgbs, weights, info, bg, rendered, opacity,
                        n_rays);
}

extern "C" int tn_composite_bwd(const float *rgbs, const float *weights, const int32_t *info, const float *bg,
                                const float *grad_rendered, float *grad_rgbs, float *grad_weights,
                                int64_t n_samples, int64_t n_rays, void *stream)
{
    TN_REQUIRE(n_samples >= 0 && n_rays >= 0, TN_E_SIZE, "tn_composite_bwd: negative size");
    if (n_rays == 0 || n_samples == 0) return TN_OK;
    TN_REQUIRE(rgbs && weights && info && grad_rendered, TN_E_NULL, "tn_composite_bwd: null pointer");
    TN_REQUIRE(((uintptr_t)info & 7) == 0, TN_E_ALIGN, "tn_composite_bwd: info must be 8-byte aligned");
    return launch_waves("composite_bwd_kernel", composite_bwd_kernel, ray_blocks(n_rays), stream, rgbs, weights, info, bg, grad_rendered,
                        grad_rgbs, grad_weights, n_rays);
}

extern "C" int tn_mse_grad(const float *rendered, const float *target, int64_t n, float scale, const float *scale_dev, float *grad,
                           double *sumsq, void *stream)
{
    return mse_grad("tn_mse_grad", rendered, target, n, scale, scale_dev, nullptr, false, grad, sumsq, stream);
}

extern "C" int tn_mse_grad_gated(const float *rendered, const float *target, int64_t n, float scale, const float *scale_dev, const float *gate,
                                 float *grad, double *sumsq, void *stream)
{
    return mse_grad("tn_mse_grad_gated", rendered, target, n, scale, scale_dev, gate, true, grad, sumsq, stream);
}

extern "C" int tn_gather_rays(const float *rays_o, const float *rays_d, const float *rgbs, const int32_t *idx, int64_t n, float *out_o,
                              float *out_d, float *out_rgb, void *stream)
{
    TN_REQUIRE(n >= 0, TN_E_SIZE, "tn_gather_rays: negative size");
    if (n == 0) return TN_OK;
    TN_REQUIRE(rays_o && rays_d && idx && out_o && out_d && (!rgbs || out_rgb), TN_E_NULL, "tn_gather_rays: null pointer");
    hipLaunchKernelGGL(gather_rays_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, rgbs, idx, n,
                       out_o, out_d, out_rgb);
    return tn::check_launch("gather_rays_kernel");
}

extern "C" int tn_ray_aux(const float *packed, const int32_t *info, int64_t n_rays, int32_t *ray_ids, float *steps, float *dirs,
                          void *stream)
{
    TN_REQUIRE(n_rays >= 0, TN_E_SIZE, "tn_ray_aux: negative size");
    if (n_rays == 0) return TN_OK;
    TN_REQUIRE(packed && info && ray_ids && steps && dirs, TN_E_NULL, "tn_ray_aux: null pointer");
    TN_REQUIRE(((uintptr_t)info & 7) == 0, TN_E_ALIGN, "tn_ray_aux: info must be 8-byte aligned");
    return launch_waves("ray_aux_kernel", ray_aux_kernel, ray_blocks(n_rays), stream, packed, info, n_rays, ray_ids, steps, dirs);
}
