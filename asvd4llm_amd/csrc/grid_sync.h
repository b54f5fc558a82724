// grid_sync.h — what the persistent two-phase kernels (lowrank_forward.hip: K10; w8_linear.hip: K16) share: the agent-scope accessors of the
// intermediate z and the in-kernel grid barrier with its give-up word.  One protocol, one copy.
#pragma once
#include "common.h"

namespace {

// The intermediate z is the only data that crosses the grid barrier.  It is written with agent-scope (sc1) stores, which go through to
// memory, and read back with agent-scope loads, which do not hit a stale line of another XCD's L2 — so the barrier itself needs NO
// cache-wide fence.  (First version: an agent-scope release + acquire fence in every wave = a write-back / invalidate of the whole L2
// per wave; 1024-2048 of them made the kernel 36-75 us long whatever the data path did.)
__device__ __forceinline__ void z_store(uint16_t* p, uint16_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint4 z_load16(const uint4* p) {
    const uint64_t* q = (const uint64_t*)p;
    const uint64_t lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
}

__device__ __forceinline__ void grid_barrier(unsigned* bar, unsigned nwg) {
    // sense-reversing barrier on three words: bar[0] arrivals, bar[1] generation, bar[2] give-up flag.  Zero-initialised once by the caller;
    // reusable.  The generation is read BEFORE this workgroup arrives: both words sit in one 128-byte line (one L2 channel serves its
    // requests in issue order) and the compiler barrier keeps the program order.  The spin is BOUNDED: the launch is not cooperative, so
    // co-residency of the <= #CUs workgroups is an assumption (another stream's persistent kernel could hold CUs); after ~2^22 polls a
    // waiter sets bar[2] and leaves instead of hanging the GPU.  What it computes next comes from an incomplete z, so the failure is made
    // VISIBLE: every workgroup ends by overwriting the elements of y it stored with NaN when the flag is set (gave_up).  (A waiter gives
    // up only while the barrier is incomplete, so every workgroup that passes normally does so AFTER the flag was set and sees it at its end.)
    // ops.lowrank_forward additionally reads and clears the word under ASVD_STRICT / ASVD_DEBUG and raises.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // this wave's z stores have been acknowledged (s_waitcnt vmcnt(0)); no L2 write-back
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned gen = __hip_atomic_load(&bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        const unsigned prev = __hip_atomic_fetch_add(&bar[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == nwg - 1) {
            __hip_atomic_store(&bar[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_s_waitcnt(0);  // the reset is out before the generation moves
            __hip_atomic_fetch_add(&bar[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            unsigned spins = 0;
            while (__hip_atomic_load(&bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (1u << 22)) {  // seconds: not a slow barrier, a workgroup that never became resident
                    __hip_atomic_store(&bar[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
    }
    __syncthreads();
}

// last statement of the kernels: a launch in which some workgroup left the barrier without its peers has no valid output.  Every workgroup
// overwrites exactly the elements of y IT stored, after its own stores (a slice of all of y would race with the stores of workgroups that
// are still in phase 2: NaN mixed with finite garbage).  The flag is read after the workgroup's last store: a workgroup can only give up
// while the barrier is incomplete, i.e. before any workgroup starts phase 2.
__device__ __forceinline__ bool gave_up(const unsigned* bar) { return __hip_atomic_load(&bar[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u; }

}  // namespace
