// The order-preserving compaction of the geometry exports (points.hip, mesh.hip, mesh_components.hip), written once: every wave
// stores the ballots of its lanes' predicates and every workgroup its counts (compact_mark), ONE workgroup per count column turns the
// counts into exclusive offsets (scan_group_counts), and a kept lane finds its row (compact_rank).  No atomics.
// Workspace, 8 B a word, for G workgroups of COMPACT_THREADS lanes with BALLOTS predicates each and COLUMNS counts: the ballots at
// [(workgroup * COMPACT_WAVES + wave) * BALLOTS + b], then the counts / offsets column-major at [column * G + workgroup] (compact_group).
// Ballot b counts into column min(b, COLUMNS - 1): with fewer columns than ballots the last column is the sum of the ballots from it on.
#pragma once
#include "tn_common.h"

namespace tn {

constexpr int COMPACT_THREADS = 256;                             // mark and ranked stores: 4 waves
constexpr int COMPACT_WAVES = COMPACT_THREADS / TN_WAVE;

template <int BALLOTS, int COLUMNS>
constexpr int64_t compact_bytes(int64_t n_groups) { return 8 * (COMPACT_WAVES * BALLOTS + COLUMNS) * n_groups; }

template <int BALLOTS>
inline int64_t *compact_group(void *workspace, int64_t n_groups) { return (int64_t *)workspace + COMPACT_WAVES * BALLOTS * n_groups; }

// bit[b]: this lane's predicate b (false in every lane past the end).  Called by ALL threads of a workgroup of COMPACT_THREADS.
template <int BALLOTS, int COLUMNS>
__device__ __forceinline__ void compact_mark(const bool (&bit)[BALLOTS], uint64_t *__restrict__ ballots, int64_t *__restrict__ group, int64_t n_groups)
{
    __shared__ int wave_count[COLUMNS][COMPACT_WAVES];
    const int tid = (int)threadIdx.x, wave = tid / TN_WAVE;
    uint64_t m[BALLOTS];
#pragma unroll
    for (int b = 0; b < BALLOTS; ++b) m[b] = __ballot(bit[b]);
    if (lane_id() == 0) {
        int count[COLUMNS] = {};
#pragma unroll
        for (int b = 0; b < BALLOTS; ++b) {
            ballots[((int64_t)blockIdx.x * COMPACT_WAVES + wave) * BALLOTS + b] = m[b];
            count[b < COLUMNS ? b : COLUMNS - 1] += __popcll(m[b]);
        }
#pragma unroll
        for (int c = 0; c < COLUMNS; ++c) wave_count[c][wave] = count[c];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < COLUMNS; ++c) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < COMPACT_WAVES; ++w) s += wave_count[c][w];
            group[c * n_groups + blockIdx.x] = s;
        }
    }
}

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

// The row of this lane's first set bit among ballots first .. first + RUN - 1 of its workgroup, whose offsets `offsets` holds (a lane
// with several bits set owns as many rows from there on, in ballot order); negative when all RUN bits are clear.  *mine, when asked
// for: the lane's bits, bit k from ballot first + k.
template <int BALLOTS, int RUN = 1>
__device__ __forceinline__ int64_t compact_rank(const uint64_t *__restrict__ ballots, const int64_t *__restrict__ offsets, int first,
                                                uint32_t *mine = nullptr)
{
    const int wave = (int)threadIdx.x / TN_WAVE, lane = lane_id();
    const uint64_t *b = ballots + (int64_t)blockIdx.x * COMPACT_WAVES * BALLOTS + first;
    uint64_t m[RUN];
    uint32_t set = 0;
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        m[k] = b[wave * BALLOTS + k];
        set |= (uint32_t)((m[k] >> lane) & 1) << k;
    }
    if (mine != nullptr) *mine = set;
    if (set == 0u) return -1;
    int64_t rank = offsets[blockIdx.x];
#pragma unroll
    for (int k = 0; k < RUN; ++k) rank += rank_below(m[k]);
    for (int w = 0; w < wave; ++w) {
#pragma unroll
        for (int k = 0; k < RUN; ++k) rank += __popcll(b[w * BALLOTS + k]);
    }
    return rank;
}

}  // namespace tn
