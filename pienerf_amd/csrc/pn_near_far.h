// Where a ray enters and leaves an axis-aligned box (kernel_near_far_from_aabb, raymarching.cu:91-159), shared by the stand-alone op
// (pn_ray_ops.hip: k_near_far) and the frame prologue (pn_frame_kernels.h: frame_rays_block): both translation units are built with
// -ffp-contract=off, so the two give the same bits.
#pragma once
#include <float.h>

// aabb = (min, max); a ray that misses the box gets near = far = FLT_MAX
__device__ __forceinline__ void pn_near_far(const float* aabb, float ox, float oy, float oz, float dx, float dy, float dz, float min_near, float& near_out,
                                            float& far_out) {
    const float rdx = 1 / dx, rdy = 1 / dy, rdz = 1 / dz;
    float near = (aabb[0] - ox) * rdx, far = (aabb[3] - ox) * rdx;
    if (near > far) { float c = near; near = far; far = c; }
    float near_y = (aabb[1] - oy) * rdy, far_y = (aabb[4] - oy) * rdy;
    if (near_y > far_y) { float c = near_y; near_y = far_y; far_y = c; }
    bool miss = (near > far_y || near_y > far);
    if (!miss) {
        if (near_y > near) near = near_y;
        if (far_y < far) far = far_y;
        float near_z = (aabb[2] - oz) * rdz, far_z = (aabb[5] - oz) * rdz;
        if (near_z > far_z) { float c = near_z; near_z = far_z; far_z = c; }
        miss = (near > far_z || near_z > far);
        if (!miss) {
            if (near_z > near) near = near_z;
            if (far_z < far) far = far_z;
            if (near < min_near) near = min_near;
        }
    }
    if (miss) near = far = FLT_MAX;
    near_out = near;
    far_out = far;
}
