// Where a ray leaves the sphere of `radius` (the larger root), as (theta, phi) scaled to [-1, 1]: kernel_sph_from_ray, raymarching.cu:165-202 — the texture
// coordinate of the background model (renderer.py:246, bg_radius > 0).  atan2f / sqrtf of the device library, like the reference.  ONE body for the
// stand-alone op (pn_ray_ops.hip: k_sph_from_ray) and the fused background kernel (pn_background.hip): both translation units are built with
// -ffp-contract=off, so the two run the same instructions and the coordinates agree bit for bit (tests/test_gpu_background.py).
#pragma once

__device__ __forceinline__ void pn_sph_coords(float ox, float oy, float oz, float dx, float dy, float dz, float radius, float& u, float& v) {
#pragma clang fp contract(off)
    const float A = dx * dx + dy * dy + dz * dz;
    const float B = ox * dx + oy * dy + oz * dz;  // B / 2 of the quadratic
    const float Cq = ox * ox + oy * oy + oz * oz - radius * radius;
    const float t = (-B + sqrtf(B * B - A * Cq)) / A;
    const float x = ox + t * dx, y = oy + t * dy, z = oz + t * dz;
    const float theta = atan2f(sqrtf(x * x + z * z), y);  // y is up
    const float phi = atan2f(z, x);
    const float rpi = 0.3183098861837907f;
    u = 2 * theta * rpi - 1;
    v = phi * rpi;
}
