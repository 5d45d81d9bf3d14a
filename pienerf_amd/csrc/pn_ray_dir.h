// The direction and origin of one pixel's ray (nerf/utils.py:125-133), shared by k_get_rays (pn_ray_ops.hip: every pixel of a view) and
// k_train_batch (pn_train_batch.hip: the sampled pixels of a training step).  Both units are built with -ffp-contract=off, so the two kernels
// write the same bits for the same pixel.
#pragma once
#include "pn_common.h"

// pixel (col, row) -> (i = col + .5, j = row + .5); pose: device pointer, row-major 4x4 cam2world.  o3 / d3: the ray's slots in rays_o / rays_d.
__device__ __forceinline__ void pn_pixel_ray(const float* __restrict__ pose, float fx, float fy, float cx, float cy, int col, int row,
                                             float* __restrict__ o3, float* __restrict__ d3) {
    const float i = (float)col + 0.5f, j = (float)row + 0.5f;
    const float xs = (i - cx) / fx, ys = (j - cy) / fy, zs = 1.0f;
    const float nrm = sqrtf(xs * xs + ys * ys + zs * zs);
    const float d0 = xs / nrm, d1 = ys / nrm, d2 = zs / nrm;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d3[c] = d0 * pose[c * 4] + d1 * pose[c * 4 + 1] + d2 * pose[c * 4 + 2];
        o3[c] = pose[c * 4 + 3];
    }
}
