// Composite: kernels of the render unit (included by pn_render_ops.hip only).
#pragma once
#include "pn_render_records.h"

// ------------------------------------------------------------------------------------------------ composite
// kernel_composite_rays, raymarching.cu:827-923.  __expf -> the gfx950 fast exponential (v_exp_f32 on x*log2e).
__device__ __forceinline__ bool composite_one(int index, uint32_t slot0, uint32_t n_step, float T_thresh, float* rays_t,
                                              const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
                                              float* weights_sum, float* depth, float* image) {
    sigmas += (size_t)slot0;
    rgbs += (size_t)slot0 * 3;
    deltas += (size_t)slot0 * 2;
    float t = rays_t[index];
    float ws = weights_sum[index], d = depth[index];
    float r = image[index * 3], g = image[index * 3 + 1], b = image[index * 3 + 2];
    uint32_t step = 0;
    while (step < n_step) {
        if (deltas[0] == 0) break;
        const float alpha = 1.0f - __expf(-sigmas[0] * deltas[0]);
        const float T = 1 - ws;
        const float w = alpha * T;
        ws += w;
        t += deltas[1];
        d += w * t;
        r += w * rgbs[0];
        g += w * rgbs[1];
        b += w * rgbs[2];
        if (T < T_thresh) break;
        sigmas++; rgbs += 3; deltas += 2; step++;
    }
    const bool alive = !(step < n_step);
    if (alive) rays_t[index] = t;  // (the caller marks a dead ray in rays_alive)
    weights_sum[index] = ws;
    depth[index] = d;
    image[index * 3] = r; image[index * 3 + 1] = g; image[index * 3 + 2] = b;
    return alive;
}

// One 256-ray chunk per block; in frame-driver mode also records the chunk's survivor count for the compaction pass.
// groups / group_cnt (ray groups, see PnGroup): per-ray schedule, and the survivors counted per group — the alive list is sorted by ray id, so the
// lanes of a wave form a few runs of equal group id and every run costs one atomic (group_cnt == nullptr with a single group: its count is the
// chunk total the compaction computes anyway, and one counter for every wave of the launch would serialise, see PN_SEGS).
__global__ void __launch_bounds__(256) k_composite(uint32_t n_alive_arg, uint32_t n_step_arg, float T_thresh, int* rays_alive, float* rays_t,
                                                   const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                   const float* __restrict__ deltas, float* weights_sum, float* depth, float* image,
                                                   const PnTrip* trip, int* chunk_counts, const PnGroup* __restrict__ groups, uint32_t group_rays,
                                                   int* group_cnt) {
    uint32_t n_alive = n_alive_arg, n_step_trip = n_step_arg;
    if (trip) { n_alive = (uint32_t)trip->n_alive; n_step_trip = (uint32_t)trip->n_step; }
    for (uint32_t chunk = blockIdx.x; chunk * 256u < n_alive; chunk += gridDim.x) {  // bounded grid, see k_march
        const uint32_t n = threadIdx.x + chunk * 256u;
        bool alive = false;
        int grp = -1;
        if (n < n_alive) {
            const int index = rays_alive[n];
            uint32_t n_step = n_step_trip, slot0;
            ray_slots(groups, group_rays, index, n, n_step, slot0);
            if (groups) grp = (int)((uint32_t)index / group_rays);
            // n_step == 0: its group has reached max_steps: the batch's loop is over (renderer.py:836), the ray is dropped
            if (n_step != 0) alive = composite_one(index, slot0, n_step, T_thresh, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image);
            if (!alive) rays_alive[n] = -1;
        }
        if (group_cnt) {
            const int lane = threadIdx.x & 63;
            const unsigned long long am = __ballot(alive);
            const int prev = __shfl_up(grp, 1);
            const bool head = lane == 0 || grp != prev;
            const unsigned long long hm = __ballot(head);
            if (head && grp >= 0) {  // this run: lanes [lane, next head)
                const unsigned long long above = lane == 63 ? 0ull : hm & ~((2ull << lane) - 1ull);
                const unsigned long long upto = above ? ((1ull << (__ffsll((long long)above) - 1)) - 1ull) : ~0ull;
                const int c = (int)__popcll(am & upto & ~((1ull << lane) - 1ull));
                if (c) atomicAdd(group_cnt + grp, c);
            }
        }
        if (chunk_counts) {
            const int c = __syncthreads_count(alive);
            if (threadIdx.x == 0) chunk_counts[chunk] = c;
        }
    }
}
