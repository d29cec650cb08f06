// Group barrier of the persistent launches (kk_encstack.hip, kk_chain.hip): the workgroups that carry one batch item meet between
// phases at a counter of their own, never at a grid-wide barrier.  Device code only.
//
// Sync words (uint32, zeroed once by the host when they are allocated):
//   [0]               error flag: a spin ran out (a member is not resident or died); every member gives up when it sees it
//   [1]               placement mismatches seen (kk_chain.hip: workgroups that did not land on the XCD of their item)
//   [32 + 32 g]       arrivals of group g
//   [32 + 32 g + 16]  exits of group g
// The counters are zero between launches: the last member to leave a launch resets them (every member has passed every barrier
// by then), so a replayed hipGraph needs no memset node in front of the launch.
#pragma once
#include "kk_common.h"

namespace {

// POLICY, at compile time:
//   XCD_LOCAL  the launch may ask at run time (init's xcd_local) for the XCD-local form: the add executes in this XCD's L2 (no scope
//              bits) and the poll is an L1-bypassing load of the same L2 line; the agent-scope form makes a round trip through the
//              fabric (~1.2 - 2 us per barrier).  Only for groups whose members share an XCD.
//   ACQUIRE    an agent-scope acquire fence (buffer_inv sc1) behind the spin: this CU's L1 forgets what it holds, for launches whose
//              hand-overs are read with plain loads.
//   SPLIT      the launch uses arrive() / wait() apart (see barrier()).
struct GroupSyncAgent { static constexpr bool XCD_LOCAL = false, ACQUIRE = false, SPLIT = true; };

template <typename POLICY>
struct GroupSync {
    unsigned *arrive_ctr, *leave, *err;
    unsigned target, members;
    bool dead, local;
    __device__ __forceinline__ void init(unsigned *words, int group, int nmembers, bool xcd_local = false) {
        err = words;
        arrive_ctr = words + 32 + 32 * group;
        leave = arrive_ctr + 16;
        target = 0;
        members = (unsigned)nmembers;
        dead = false;
        local = POLICY::XCD_LOCAL && xcd_local;
    }
    // Split barrier: arrive() publishes this workgroup's stores (every store issued before it is visible to every member
    // after its wait()); between the two a member may do work that depends on nobody (the encoder stack starts the DMA of the
    // weights of its next GEMM phase there, so that the issue time of up to 96 KB hides behind the arrival of the slowest member).
    __device__ __forceinline__ void arrive() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // each wave: its stores have been acknowledged (by the L2 / written through)
        __syncthreads();
        target += members;
        if (threadIdx.x == 0 && !dead) add();
    }
    __device__ __forceinline__ void wait() {
        if (threadIdx.x == 0 && !dead) {
            unsigned spins = 0;
            while (__hip_atomic_load(arrive_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (1u << 22)) {                        // seconds: a member is not resident / died — give up loudly
                    __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    dead = true;
                    break;
                }
                if ((spins & 1023u) == 0u && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                    dead = true;
                    break;
                }
            }
            if (POLICY::ACQUIRE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
    }
    // POLICY::SPLIT: arrive() then wait().  Otherwise the same operations under ONE test of thread 0, written out: composed from the two
    // halves (or from smaller shared pieces) the chain's kernels come out of the compiler different from what they were, with more
    // scalar spills (docs/LAB_NOTES.md, "Encoder stack: shared sources"); keep the two bodies in step.
    __device__ __forceinline__ void barrier() {
        if constexpr (POLICY::SPLIT) {
            arrive();
            wait();
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            target += members;
            if (threadIdx.x == 0 && !dead) {
                add();
                unsigned spins = 0;
                while (__hip_atomic_load(arrive_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > (1u << 22)) {                        // seconds: a member is not resident / died — give up loudly
                        __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        dead = true;
                        break;
                    }
                    if ((spins & 1023u) == 0u && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                        dead = true;
                        break;
                    }
                }
                if (POLICY::ACQUIRE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            __syncthreads();
        }
    }
    __device__ __forceinline__ void add() {
        if (POLICY::XCD_LOCAL && local) __hip_atomic_fetch_add(arrive_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_fetch_add(arrive_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void exit() {
        if (threadIdx.x == 0) {
            unsigned old;
            if (POLICY::XCD_LOCAL && local) old = __hip_atomic_fetch_add(leave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else old = __hip_atomic_fetch_add(leave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == members - 1u) {
                if (POLICY::XCD_LOCAL && local) {
                    __hip_atomic_fetch_sub(arrive_ctr, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_sub(leave, members, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    __hip_atomic_store(arrive_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(leave, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
};

}  // namespace
