// One ray of the static (undeformed) march: kernel_march_rays (raymarching.cu:703-810) restated literally, one lane per ray, so that samples are
// bit-identical to the oracle.  Shared by the stand-alone op (pn_ray_ops.hip: k_march_rays_static) and the frame form (pn_march_kernels.h:
// k_march_static_trip); both translation units are built with -ffp-contract=off.
#pragma once
#include "pn_march_math.h"

// Marches the ray at alive slot n into its n_step sample slots and returns the number it filled.  What the two callers differ in is chosen at compile time
// (without fast-math a run-time `* 0.0f` is not folded away):
//   NOISE      the start is jittered by noises[n] (nullptr: 0); without it `t += clamp(...) * noise` is left out — perturb = False leaves t unchanged
//   END_SLOTS  unfilled slots are ended (delta = 0) for the composite; the op-level wrapper zero-fills instead (raymarching.py:415-417)
template <bool NOISE, bool END_SLOTS>
__device__ __forceinline__ uint32_t march_static_one(uint32_t n, uint32_t n_step, const int* __restrict__ rays_alive, const float* __restrict__ rays_t,
                                                     const float* __restrict__ rays_o, const float* __restrict__ rays_d, float bound, float dt_gamma,
                                                     uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* __restrict__ grid,
                                                     const float* __restrict__ fars, float* __restrict__ xyzs, float* __restrict__ dirs,
                                                     float* __restrict__ deltas, const float* __restrict__ noises) {
    using namespace pnm;
    const int index = rays_alive[n];
    const float noise = (NOISE && noises) ? noises[n] : 0.0f;
    rays_o += (size_t)index * 3;
    rays_d += (size_t)index * 3;
    xyzs += (size_t)n * n_step * 3;
    dirs += (size_t)n * n_step * 3;
    deltas += (size_t)n * n_step * 2;
    const float ox = rays_o[0], oy = rays_o[1], oz = rays_o[2];
    const float dx = rays_d[0], dy = rays_d[1], dz = rays_d[2];
    const float rdx = 1 / dx, rdy = 1 / dy, rdz = 1 / dz;
    const float rH = 1 / (float)H;
    const float H3 = (float)(H * H * H);
    float t = rays_t[index];
    const float far = fars[index];
    const float dt_min = 2 * 1.73205080757f / max_steps;
    const float dt_max = 2 * 1.73205080757f * (1 << (C - 1)) / H;
    uint32_t step = 0;
    if (NOISE) t += clampf(t * dt_gamma, dt_min, dt_max) * noise;
    float last_t = t;
    while (t < far && step < n_step) {
        const float x = clampf(ox + t * dx, -bound, bound);
        const float y = clampf(oy + t * dy, -bound, bound);
        const float z = clampf(oz + t * dz, -bound, bound);
        const float dt = clampf(t * dt_gamma, dt_min, dt_max);
        const int level = max(mip_from_pos(x, y, z, (float)C), mip_from_dt(dt, (float)H, (float)C));
        const float mip_bound = fminf(scalbnf(1, level), bound);
        const float mip_rbound = 1 / mip_bound;
        // `0.5 * (x * mip_rbound + 1) * H` is a double product in the reference; (float)(0.5 * (double)v * (double)H) == v * (0.5f * H)
        // for every float v and power-of-two-free H < 2^24 only when the product is exact, so it is kept in double here (cold path)
        const int nx = (int)clampf((float)(0.5 * (double)(x * mip_rbound + 1) * (double)H), 0.0f, (float)(H - 1));
        const int ny = (int)clampf((float)(0.5 * (double)(y * mip_rbound + 1) * (double)H), 0.0f, (float)(H - 1));
        const int nz = (int)clampf((float)(0.5 * (double)(z * mip_rbound + 1) * (double)H), 0.0f, (float)(H - 1));
        const uint32_t vox = (uint32_t)(level * H3 + (float)morton3D(nx, ny, nz));
        const bool occ = grid[vox / 8] & (1 << (vox % 8));
        if (occ) {
            xyzs[0] = x; xyzs[1] = y; xyzs[2] = z;
            dirs[0] = dx; dirs[1] = dy; dirs[2] = dz;
            t += dt;
            deltas[0] = dt;
            deltas[1] = t - last_t;
            last_t = t;
            xyzs += 3; dirs += 3; deltas += 2;
            step++;
        } else {
            const float tx = (((nx + 0.5f + 0.5f * signf(dx)) * rH * 2 - 1) * mip_bound - x) * rdx;
            const float ty = (((ny + 0.5f + 0.5f * signf(dy)) * rH * 2 - 1) * mip_bound - y) * rdy;
            const float tz = (((nz + 0.5f + 0.5f * signf(dz)) * rH * 2 - 1) * mip_bound - z) * rdz;
            const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
            do { t += clampf(t * dt_gamma, dt_min, dt_max); } while (t < tt);
        }
    }
    if (END_SLOTS)
        for (uint32_t s = step; s < n_step; s++) { deltas[0] = 0.0f; deltas[1] = 0.0f; deltas += 2; }
    return step;
}
