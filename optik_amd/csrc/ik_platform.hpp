// ik_platform.hpp -- the ONE place where the device headers know about tests/emu.
//
// The library is never built with OPTIK_LANE_EMU.  tests/emu/quad_emu.cpp compiles the quad and lane-per-restart
// solvers, and tests/emu/wide_emu.cpp the general solver of ik_wide.hpp, for the host with the wave emulated by one
// thread per lane (tests/emu/lane_emu.hpp): there the HIP runtime header is replaced by the emulation -- every device
// header reaches it through this file -- which also provides the cross-lane builtins this code uses
// (__builtin_amdgcn_update_dpp with quad_perm controls, mbcnt, ballot, shuffles, lane reads, fences, __syncthreads)
// under their device names and with their device semantics, so ik_lane.hpp and everything above it is the same text on
// both sides --
// and the three things below differ: the register class an empty asm statement can launder a value through, how a
// pointer into LDS keeps its address space through that laundering, and the shape of the (partial) wave.
#pragma once

#ifdef OPTIK_LANE_EMU
#include "lane_emu.hpp"
#define OPTIK_REG_INOUT "+r"
#else
#include <hip/hip_runtime.h>
#define OPTIK_REG_INOUT "+v"
#endif
#include <stdint.h>

// wave cycles per phase are only counted on the device (-DOPTIK_PROFILE builds)
#if defined(OPTIK_PROFILE) && !defined(OPTIK_LANE_EMU)
#define OPTIK_DEVICE_PROFILE 1
#endif

namespace optik {

// quads of lanes the wave has, and the number of the wave's workgroup (the emulation runs one partial wave)
__device__ __forceinline__ int wave_quads() {
#ifdef OPTIK_LANE_EMU
    return optik_emu::t_wave->lanes / 4;
#else
    return 16;
#endif
}

// A pointer INTO LDS made opaque to the optimiser: only the offset is laundered, the address space is kept.  (A
// generic pointer laundered whole comes back as FLAT accesses: the LDS is reached through the aperture check of
// the vector-memory path, every access counts on both wait counters, and nothing the LDS returns can be waited for
// selectively.)
template <class T>
__device__ __forceinline__ const T *launder_lds(const T *p) {
#ifdef OPTIK_LANE_EMU
    asm volatile("" : "+r"(p));
    return p;
#else
    typedef const T __attribute__((address_space(3))) *lds_cptr;
    unsigned off = (unsigned)(__UINTPTR_TYPE__)(lds_cptr)p;
    asm volatile("" : "+v"(off));
    return (const T *)(lds_cptr)(__UINTPTR_TYPE__)off;
#endif
}

// A pointer to GLOBAL memory that the compiler cannot see to be one (it was read from a structure in LDS, say), told so:
// the accesses through it become global_* instead of flat_* instructions.  A flat access counts on the LDS wait counter
// as well as on the vector-memory one, so the next wait for ANY LDS result also waits for its round trip to memory; a
// global access leaves the LDS counter alone and its latency can hide behind the work that follows.  (The pointer
// keeps its address space in its type: cast back to a generic one it is a flat pointer again.)
#ifdef OPTIK_LANE_EMU
template <class T>
__device__ __forceinline__ T *global_ptr(T *p) { return p; }
__device__ __forceinline__ unsigned long long global_atomic_add(unsigned long long *p, unsigned long long v) { return atomicAdd(p, v); }
__device__ __forceinline__ unsigned long long global_atomic_min(unsigned long long *p, unsigned long long v) { return atomicMin(p, v); }
#else
#define OPTIK_GLOBAL_AS __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ OPTIK_GLOBAL_AS T *global_ptr(T *p) { return (OPTIK_GLOBAL_AS T *)p; }
// (atomicAdd / atomicMin of the HIP headers on such a pointer: relaxed, device scope)
__device__ __forceinline__ unsigned long long global_atomic_add(OPTIK_GLOBAL_AS unsigned long long *p, unsigned long long v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long global_atomic_min(OPTIK_GLOBAL_AS unsigned long long *p, unsigned long long v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

}  // namespace optik
