// Dev builds with -DTN_PHASE_TIMERS (scripts/build_dev_lib.sh, scripts/phase_time*.py): where a tile's cycles go.  A file names its
// 16 counters and the exported getter once, TN_PHASE_COUNTERS(array, getter), and wraps the two or three macros below in short names of
// its own.  Without the flag everything here expands to nothing.
#pragma once
#ifdef TN_PHASE_TIMERS
#define TN_PHASE_COUNTERS(arr, getter)                                                                        \
    __device__ unsigned long long arr[16];                                                                    \
    extern "C" int getter(unsigned long long *out, int reset) {                                               \
        hipMemcpyFromSymbol(out, HIP_SYMBOL(arr), sizeof(unsigned long long) * 16);                           \
        if (reset) { unsigned long long z[16] = {}; hipMemcpyToSymbol(HIP_SYMBOL(arr), z, sizeof(z)); }       \
        return 0;                                                                                             \
    }
#define TN_PHASE_BEGIN(t) unsigned long long t = __builtin_amdgcn_s_memtime();
// cycles since `t` to counter k (lane 0 of every wave), then `t` restarts behind the atomic
#define TN_PHASE(arr, t, k) { __builtin_amdgcn_sched_barrier(0); const unsigned long long n_ = __builtin_amdgcn_s_memtime(); if (tn::lane_id() == 0) atomicAdd(&arr[k], n_ - t); t = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
// ... `t` runs on: consecutive phases add up to the whole
#define TN_PHASE_RUNNING(arr, t, k) { __builtin_amdgcn_sched_barrier(0); const unsigned long long n_ = __builtin_amdgcn_s_memtime(); if (tn::lane_id() == 0) atomicAdd(&arr[k], n_ - t); t = n_; }
#else
#define TN_PHASE_COUNTERS(arr, getter)
#define TN_PHASE_BEGIN(t)
#define TN_PHASE(arr, t, k)
#define TN_PHASE_RUNNING(arr, t, k)
#endif
