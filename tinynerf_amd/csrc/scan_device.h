// The one-workgroup exclusive scan of per-workgroup counts behind an order-preserving compaction (mesh.hip).  points_scan_kernel
// (points.hip) is the same loop and keeps its own copy: called through this header its instructions come out in another operand order
// (DESIGN 6h), and that file's device code is held fixed.
#pragma once
#include "tn_common.h"

namespace tn {

// group[0..n_groups): counts in, exclusive offsets out; *count = scale x their total (a trip's total stays below 2^31).  Called by ALL
// `THREADS_` threads of ONE workgroup, THREADS_ counts per trip with a carry; ends on a barrier, so it may be called again at once.
template <int THREADS_>
__device__ __forceinline__ void scan_group_counts(int64_t *__restrict__ group, int64_t n_groups, int64_t *__restrict__ count, int64_t scale = 1)
{
    constexpr int SW = THREADS_ / TN_WAVE;
    __shared__ int wave_total[SW];
    const int tid = (int)threadIdx.x, lane = tn::lane_id(), wave = tid / TN_WAVE;
    int64_t carry = 0;
    for (int64_t base = 0; base < n_groups; base += THREADS_) {          // (trip count uniform over the workgroup)
        const int64_t i = base + tid;
        const int v = i < n_groups ? (int)group[i] : 0;
        const int s = tn::wave_scan(v);
        if (lane == TN_WAVE - 1) wave_total[wave] = s;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SW; ++w) {
            const int t = wave_total[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (i < n_groups) group[i] = carry + before + (s - v);
        carry += total;
        __syncthreads();                                                 // wave_total is rewritten by the next trip
    }
    if (tid == 0) *count = scale * carry;
}

}  // namespace tn
