// Wave priority of the substep's kernels and the timing build's stamps and phase clocks (included by pn_sim.hip only).
#pragma once
#include "pn_common.h"

// The substep is a chain of ~30 short dependent launches that runs concurrently with the render kernels of other frames
// (harness.capture_pipelined): its waves ask the SIMD arbiter for the highest user priority so the chain's latency does not
// stretch when the CUs are full of march waves.
#ifndef PN_SIM_PRIO_LEVEL
#define PN_SIM_PRIO_LEVEL 3
#endif
#define PN_SIM_PRIO() __builtin_amdgcn_s_setprio(PN_SIM_PRIO_LEVEL)

#ifndef PN_SIM_STAMPS
#define PN_SIM_STAMPS 0
#endif
#if PN_SIM_STAMPS
// Timing build (tools/build_variant.py -DPN_SIM_STAMPS=1 with PN_VARIANT_UNITS=pn_sim.hip): the first thread of every substep kernel notes when its launch
// STARTED (100 MHz wall clock) and which kernel it is, into a ring a tool reads back (pn_sim_stamps_read): start-to-start gaps along the simulator's
// chain of dependent launches — alone, and beside the render lanes.  [0]: next slot; then entries (kernel id << 56 | ticks)
#define PN_SIM_STAMP_CAP 65536
__device__ unsigned long long g_sim_stamps[1 + PN_SIM_STAMP_CAP];
__device__ __forceinline__ void sim_stamp(int id) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long i = atomicAdd(&g_sim_stamps[0], 1ull);
        g_sim_stamps[1 + (i % PN_SIM_STAMP_CAP)] = ((unsigned long long)id << 56) | (__builtin_amdgcn_s_memrealtime() & 0x00ffffffffffffffull);
    }
}
extern "C" int pn_sim_stamps_read(unsigned long long* host, int reset) {
    PN_HIP_CHECK(hipDeviceSynchronize());
    if (host) PN_HIP_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sim_stamps), sizeof(unsigned long long) * (1 + PN_SIM_STAMP_CAP)));
    if (reset) { const unsigned long long z = 0; PN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_sim_stamps), &z, sizeof(z))); }
    return PN_OK;
}
#define PN_SIM_STAMP(id) sim_stamp(id)
// ... and phase clocks inside k_cells_elastic_gather: thread 0 of EVERY workgroup reads the 100 MHz clock at the phase boundaries (a scalar instruction,
// nothing in flight) and adds its differences to g_sim_phase at the very end: [p] ticks from boundary p to p + 1 summed over workgroups, [8] workgroups,
// [9] the largest start-to-end of a workgroup, [10 + p] the largest single difference
__device__ unsigned long long g_sim_phase[24];
#define PN_SIM_PHASE_DECL unsigned long long ph_[8]; int ph_n_ = 0
#define PN_SIM_PHASE_MARK do { if (ph_n_ < 8) ph_[ph_n_++] = __builtin_amdgcn_s_memrealtime(); } while (0)
__device__ __forceinline__ void sim_phase_flush(const unsigned long long* ph, int n) {
    if (threadIdx.x == 0) {
        for (int p = 0; p + 1 < n; p++) { atomicAdd(&g_sim_phase[p], ph[p + 1] - ph[p]); atomicMax(&g_sim_phase[10 + p], ph[p + 1] - ph[p]); }
        atomicAdd(&g_sim_phase[8], 1ull);
        atomicMax(&g_sim_phase[9], ph[n - 1] - ph[0]);
    }
}
extern "C" int pn_sim_phase_read(unsigned long long* host, int reset) {
    PN_HIP_CHECK(hipDeviceSynchronize());
    if (host) PN_HIP_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sim_phase), sizeof(unsigned long long) * 24));
    if (reset) { unsigned long long z[24] = {0}; PN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_sim_phase), z, sizeof(z))); }
    return PN_OK;
}
#define PN_SIM_PHASE(id) PN_SIM_PHASE_MARK
#define PN_SIM_PHASE_FLUSH sim_phase_flush(ph_, ph_n_)
#else
#define PN_SIM_STAMP(id)
#define PN_SIM_PHASE(id)
#define PN_SIM_PHASE_DECL
#define PN_SIM_PHASE_FLUSH
#endif
